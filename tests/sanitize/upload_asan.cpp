// upload_asan.cpp — the host -> HBM copies of padded frames under AddressSanitizer, against the host-only stand-ins of
// hip_stubs.h (copies become memcpy, which ASan checks on both sides). Every frame is a window of a wider image that ENDS
// ON THE LAST BYTE OF ITS HEAP BLOCK — a ROI whose last pixel is the parent buffer's last byte — so a copy of
// row_stride * height bytes runs row_stride - width * channels * el bytes into the red zone behind the block. The frames go
// through AsyncUpload (the whole-stack paths) and through a plain copy of frame_copy_bytes() (context.h: what
// resolve_frames, the quality pass, the frame-by-frame keypoint path and the peer copies of a multi-device context take).
// Checks besides: every pixel arrives at its place in the engine's buffer (frames row_stride * height apart), and a tight
// stack copies what it always did.
#include "hip_stubs.h"

#include <cstdio>
#include <vector>

extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = reinterpret_cast<hipEvent_t>(new int(0)); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { *reinterpret_cast<int*>(e) = 1; return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 1.0f; return hipSuccess; }
}
#include "../../libstacker_rs_amd/csrc/upload.cpp"

struct Case { int w, h, cn, depth; size_t stride; size_t x0_bytes; };   // stride 0 = tight

static int run(const Case& c, int n) {
    const size_t el = (size_t)c.depth / 8, tight = (size_t)c.w * c.cn * el, rb = c.stride ? c.stride : tight;
    const size_t span = rb * (size_t)(c.h - 1) + tight;
    std::vector<unsigned char*> blocks(n);
    std::vector<const void*> ptrs(n);
    for (int i = 0; i < n; i++) {
        blocks[i] = new unsigned char[c.x0_bytes + span];              // the window's last pixel is the block's last byte
        for (size_t k = 0; k < c.x0_bytes + span; k++) blocks[i][k] = (unsigned char)(i * 31 + k * 7 + 1);
        ptrs[i] = blocks[i] + c.x0_bytes;
    }
    stk_frames fr{};
    fr.data = ptrs.data(); fr.n = n; fr.width = c.w; fr.height = c.h; fr.channels = c.cn; fr.depth = c.depth;
    fr.location = STK_HOST; fr.row_stride_bytes = c.stride;
    if (frame_copy_bytes(&fr) != span || frame_copy_bytes(rb, c.w, c.h, c.cn, c.depth) != span) return 10;
    if (!c.stride && frame_copy_bytes(&fr) != tight * (size_t)c.h) return 11;          // a tight frame: all of it, as before
    const size_t fb = rb * (size_t)c.h;                                // the spacing of the engine's own buffer
    std::vector<unsigned char> dev(fb * (size_t)n);
    auto rows_arrived = [&]() {
        for (int i = 0; i < n; i++)
            for (int y = 0; y < c.h; y++)
                if (std::memcmp(dev.data() + fb * (size_t)i + rb * (size_t)y, (const unsigned char*)ptrs[i] + rb * (size_t)y, tight)) return false;
        return true;
    };
    stk_ctx ctx;
    for (int batch : {1, 3, 64}) {
        std::fill(dev.begin(), dev.end(), 0);
        stk::AsyncUpload up;
        if (up.start(&ctx, &fr, dev.data(), fb, batch) != STK_OK) return 20;
        for (int b = 0; b < up.batches(); b++) if (up.wait_batch(b, nullptr) != STK_OK) return 21;
        if (up.finish(nullptr) != STK_OK) return 22;
        if (!rows_arrived()) return 23;
    }
    std::fill(dev.begin(), dev.end(), 0);                              // the copy every other site makes
    for (int i = 0; i < n; i++)
        if (hipMemcpyAsync(dev.data() + fb * (size_t)i, fr.data[i], frame_copy_bytes(&fr), hipMemcpyHostToDevice, nullptr) != hipSuccess) return 30;
    if (!rows_arrived()) return 31;
    for (unsigned char* b : blocks) delete[] b;
    return 0;
}

int main() {
    const Case cases[] = {
        {16, 5, 3, 8, 64, 3},        // u8 BGR ROI at x0 = 1 of a wider image: 16 bytes of padding per row
        {15, 4, 3, 8, 47, 0},        // odd stride, 2 bytes of padding
        {16, 5, 3, 16, 128, 6},      // u16
        {7, 3, 1, 32, 40, 4},        // f32 grey
        {9, 6, 4, 8, 36, 0},         // BGRA, stride == the tight row
        {16, 5, 3, 8, 0, 0},         // tight
        {5, 1, 3, 8, 32, 0},         // one row: the span is the row itself
    };
    for (const Case& c : cases) {
        const int r = run(c, 5);
        if (r) { std::printf("case %dx%dx%d/%d stride %zu: %d\n", c.w, c.h, c.cn, c.depth, c.stride, r); return r; }
    }
    std::printf("ok\n");
    return 0;
}
