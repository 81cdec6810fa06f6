// kernels_warp.hip — warpPerspective / warpAffine (INTER_LINEAR) fused with the u8/u16 -> f32
// convert (x 1/255) and with the running f32 accumulator:
//     acc(p) (+)= sum over frames f of  bilinear( convert(frame_f), Minv_f . p )
// Reference: utils.rs:133 (convert), lib.rs:290-299 / 780-803 (warp), lib.rs:306-316 / 807-814 (add).
// The reference materialises a converted f32 frame (A2), a warped f32 frame (F1) and a fresh sum
// (G1) per frame: 12+12+12+12+12 B/px/channel-triple of traffic. Here one thread owns one
// destination pixel, keeps its three accumulator channels in registers across ALL frames of the
// launch and touches HBM for: the source taps (u8: ~3 B/px/frame, gathered, L2-friendly because the
// maps are near-identity) + one 12-byte accumulator read + one 12-byte accumulator write.
// NOT HBM-bound: 3 bytes per pixel and frame carry ~65 vector instructions (~108 issue slots at gfx950's rates, twelve
// byte conversions alone are 24: tools/valu_rates.hip) — the vector pipe is the limit. No LDS needed for
// the gather (footprints of neighbouring lanes overlap in L1/L2).
// Option "warp_interpolation" = STK_INTER_CUBIC sends every launch to the bicubic kernels of warp_cubic_body.h instead
// (WarpArgs::interp; an extension beyond the reference).
#include "warp_cubic_body.h"

namespace stk {

// 16-bit BGR fast path (16-bit stacks: stk_hybrid_match): the two horizontally adjacent taps of a row are 12 contiguous
// bytes -> one 12-byte load; waves whose footprints are all interior take it, border waves take per-tap conditional loads.
// Same operation sequence as the generic kernel.
__device__ __forceinline__ Tap12 load_tap12(const uint8_t* p) {
    Tap12 t;
    __builtin_memcpy(&t, p, 12);
    return t;
}

template <bool AFFINE>
__global__ __launch_bounds__(256) void warp_accumulate_u16c3_kernel(WarpArgs a) {
    constexpr int WU = 4;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.dw || y >= a.dh) return;
    float* accp = a.acc + (size_t)y * a.acc_stride + (size_t)x * 3;
    float s[3] = {0.f, 0.f, 0.f};
    if (a.accumulate) { s[0] = accp[0]; s[1] = accp[1]; s[2] = accp[2]; }
    const float fx = (float)x, fy = (float)y;
    const int sw = a.sw, sh = a.sh;
    const int stride_el = (int)a.src_stride;               // row stride in 16-bit elements
    const float alpha = a.alpha;
    const float bv[3] = {a.bv[0], a.bv[1], a.bv[2]};

    for (int f0 = 0; f0 < a.n_frames; f0 += WU) {
        float ax[WU], ay[WU];
        int ix[WU], iy[WU];
        bool interior = true;
#pragma unroll
        for (int u = 0; u < WU; u++) {
            const WarpFrame* fr = a.frames + min(f0 + u, a.n_frames - 1);
            // same coordinate arithmetic as the u8 kernel: packed (X, Y), one reciprocal chain shared by X / W and Y / W
            f32x2 XY = pk_fma(f32x2{fr->M[0], fr->M[3]}, f32x2{fx, fx}, pk_fma(f32x2{fr->M[1], fr->M[4]}, f32x2{fy, fy}, f32x2{fr->M[2], fr->M[5]}));
            if (!AFFINE) {
                const float W = __builtin_fmaf(fr->M[6], fx, __builtin_fmaf(fr->M[7], fy, fr->M[8]));
                if (fr->flags & WARPFRAME_DIV_IN_RANGE) XY = div2_shared(XY, W);     // decided per frame on the host (uniform branch)
                else {
                    const float aw = __builtin_fabsf(W);
                    const bool safe = (aw < 1.0995116e12f) & (__builtin_fabsf(XY.x) < 1.0995116e12f) & (__builtin_fabsf(XY.y) < 1.0995116e12f) &
                                      (aw > 9.094947e-13f);                         // compares: a NaN operand fails
                    if (__all(safe)) XY = div2_shared(XY, W);
                    else { XY.x = XY.x / W; XY.y = XY.y / W; }
                }
            }
            const float X = XY.x, Y = XY.y;
            const bool finite = (__builtin_fabsf(X) < 1e9f) & (__builtin_fabsf(Y) < 1e9f);
            const float flx = __builtin_floorf(X), fly = __builtin_floorf(Y);
            ix[u] = finite ? (int)flx : -100000; iy[u] = finite ? (int)fly : -100000;
            ax[u] = finite ? X - flx : 0.0f; ay[u] = finite ? Y - fly : 0.0f;
            // (a row to spare below, as in the u8 kernel: the aligned 16-byte window of the last pixel pair of the last row
            // would end 4 bytes past the frame; rows sh-2 and sh-1 are left to the rim path)
            interior &= ((unsigned)ix[u] < (unsigned)(sw - 1)) & ((unsigned)iy[u] < (unsigned)(sh - 2));
        }
#define STK_LERP16(p00, p01, p10, p11)                                                   \
    __builtin_fmaf(ay[u], __builtin_fmaf(ax[u], (p11) - (p10), (p10)) - __builtin_fmaf(ax[u], (p01) - (p00), (p00)), \
                   __builtin_fmaf(ax[u], (p01) - (p00), (p00)))
        if (__all(interior)) {
            Tap12 r0[WU], r1[WU];
#pragma unroll
            for (int u = 0; u < WU; u++) {
                const uint8_t* src = (const uint8_t*)a.frames[min(f0 + u, a.n_frames - 1)].src;
                const unsigned o = (unsigned)(__mul24(iy[u], stride_el) + ix[u] * 3) * 2u;
                const uint8_t* src1 = src + (unsigned)stride_el * 2u;               // uniform second-row base
                if (a.frames[min(f0 + u, a.n_frames - 1)].flags & WARPFRAME_SRC_ALIGNED4) {
                    // as in the u8 kernel: a dword-aligned 16-byte window instead of a 12-byte gather at a 6-byte lane stride
                    // that starts on an odd word in half of the lanes; v_alignbyte shifts by 0 or 2 bytes
                    const unsigned oa = o & ~3u, sh = o & 3u;
                    uint32_t t0[4], t1[4];
                    __builtin_memcpy(t0, __builtin_assume_aligned(src + oa, 4), 16);
                    __builtin_memcpy(t1, __builtin_assume_aligned(src1 + oa, 4), 16);
                    r0[u] = Tap12{__builtin_amdgcn_alignbyte(t0[1], t0[0], sh), __builtin_amdgcn_alignbyte(t0[2], t0[1], sh), __builtin_amdgcn_alignbyte(t0[3], t0[2], sh)};
                    r1[u] = Tap12{__builtin_amdgcn_alignbyte(t1[1], t1[0], sh), __builtin_amdgcn_alignbyte(t1[2], t1[1], sh), __builtin_amdgcn_alignbyte(t1[3], t1[2], sh)};
                } else {
                    r0[u] = load_tap12(src + o);
                    r1[u] = load_tap12(src1 + o);
                }
            }
#pragma unroll
            for (int u = 0; u < WU; u++) {
                if (f0 + u < a.n_frames) {
                    // same pairing as the u8 kernel: (B, G) of a tap and R of the two rows go through v_pk_mul / v_pk_fma
                    const f32x2 al2 = {alpha, alpha}, ax2 = {ax[u], ax[u]}, ay2 = {ay[u], ay[u]};
#define STK_LO16(d) ((float)((d) & 0xffffu))
#define STK_HI16(d) ((float)((d) >> 16))
                    const f32x2 bg00 = f32x2{STK_LO16(r0[u].a), STK_HI16(r0[u].a)} * al2, bg01 = f32x2{STK_HI16(r0[u].b), STK_LO16(r0[u].c)} * al2;
                    const f32x2 bg10 = f32x2{STK_LO16(r1[u].a), STK_HI16(r1[u].a)} * al2, bg11 = f32x2{STK_HI16(r1[u].b), STK_LO16(r1[u].c)} * al2;
                    const f32x2 rl = f32x2{STK_LO16(r0[u].b), STK_LO16(r1[u].b)} * al2;
                    const f32x2 rr = f32x2{STK_HI16(r0[u].c), STK_HI16(r1[u].c)} * al2;
#undef STK_LO16
#undef STK_HI16
                    const f32x2 t0 = pk_fma(ax2, bg01 - bg00, bg00), t1 = pk_fma(ax2, bg11 - bg10, bg10);
                    const f32x2 tr = pk_fma(ax2, rr - rl, rl);
                    const f32x2 vbg = pk_fma(ay2, t1 - t0, t0);
                    s[0] = s[0] + vbg.x; s[1] = s[1] + vbg.y;
                    s[2] = s[2] + __builtin_fmaf(ay[u], tr.y - tr.x, tr.x);
                }
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < WU; u++) {
            if (f0 + u < a.n_frames) {
                const uint16_t* src = (const uint16_t*)a.frames[f0 + u].src;
                const int x0 = ix[u], y0 = iy[u];
                const bool vx0 = (unsigned)x0 < (unsigned)sw, vx1 = (unsigned)(x0 + 1) < (unsigned)sw;
                const bool vy0 = (unsigned)y0 < (unsigned)sh, vy1 = (unsigned)(y0 + 1) < (unsigned)sh;
                const int xc0 = min(max(x0, 0), sw - 1), xc1 = min(max(x0 + 1, 0), sw - 1);
                const int yc0 = min(max(y0, 0), sh - 1), yc1 = min(max(y0 + 1, 0), sh - 1);
                const uint16_t* q0 = src + (size_t)yc0 * stride_el;
                const uint16_t* q1 = src + (size_t)yc1 * stride_el;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float p00 = (vx0 & vy0) ? (float)q0[xc0 * 3 + c] * alpha : bv[c];
                    const float p01 = (vx1 & vy0) ? (float)q0[xc1 * 3 + c] * alpha : bv[c];
                    const float p10 = (vx0 & vy1) ? (float)q1[xc0 * 3 + c] * alpha : bv[c];
                    const float p11 = (vx1 & vy1) ? (float)q1[xc1 * 3 + c] * alpha : bv[c];
                    s[c] = s[c] + STK_LERP16(p00, p01, p10, p11);
                }
            }
        }
#undef STK_LERP16
    }
    accp[0] = s[0]; accp[1] = s[1]; accp[2] = s[2];
}

// One thread per fold entry. A frame whose ECC failed (status != 0) gets the identity: the host reports the failure and
// discards the sum, the table only has to be harmless.
__global__ void warp_frames_from_ecc_kernel(const EccFrameResult* __restrict__ results, const void* const* __restrict__ src_ptrs,
                                            int n_templates, int add_reference, int is_affine, int w, int h, size_t src_row_bytes,
                                            WarpFrame* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_out = n_templates + (add_reference ? 1 : 0);
    if (i >= n_out) return;
    const int t = add_reference ? i - 1 : i;                // template index, -1: the reference frame itself
    double M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (t >= 0 && results[t].status == 0) {
        for (int k = 0; k < 9; k++) M[k] = (double)results[t].warp[k];
        if (is_affine) { M[6] = 0; M[7] = 0; M[8] = 1; }
    }
    WarpFrame wf;
    warp_frame_make(wf, src_ptrs[t + 1], M, is_affine);
    wf.flags = warp_frame_flags(wf.src, wf.M, src_row_bytes, w, h, is_affine);
    out[i] = wf;
}

hipError_t launch_warp_frames_from_ecc(const EccFrameResult* results, const void* const* src_ptrs, int n_templates, int add_reference,
                                       int is_affine, int w, int h, size_t src_row_bytes, WarpFrame* out, hipStream_t s) {
    const int n_out = n_templates + (add_reference ? 1 : 0);
    if (n_out <= 0) return hipSuccess;
    warp_frames_from_ecc_kernel<<<(n_out + 63) / 64, 64, 0, s>>>(results, src_ptrs, n_templates, add_reference, is_affine, w, h, src_row_bytes, out);
    return hipGetLastError();
}

hipError_t launch_warp_accumulate(const WarpArgs& a, int depth, hipStream_t s) {
    dim3 grid((a.dw + 63) / 64, (a.dh + 3) / 4);
    if (a.interp == STK_INTER_CUBIC) {
        if (warp_u8c3_applies(a, depth)) return launch_warp_cubic_u8c3<false, NoClip>(a, ClipArgs{}, grid, s);
        return launch_warp_cubic<false, NoClipN>(a, ClipArgs{}, depth, grid, s);
    }
    if (warp_u8c3_applies(a, depth)) {
        const int v = a.tune & 0xff;                // tuning: bits 0-1 tile shape, bits 4-5 frames in flight
#define STK_U8C3(WX, WU)                                                                                   \
        do {                                                                                               \
            dim3 g((a.dw + 64 * WX - 1) / (64 * WX), (a.dh + 4 / WX - 1) / (4 / WX));                      \
            if (a.is_affine) warp_accumulate_u8c3_kernel<true, WX, WU, false, NoClip><<<g, 256, 0, s>>>(a, ClipArgs{});              \
            else warp_accumulate_u8c3_kernel<false, WX, WU, false, NoClip><<<g, 256, 0, s>>>(a, ClipArgs{});                         \
        } while (0)
        switch (v) {
            case 0x01: STK_U8C3(2, 4); break;
            case 0x02: STK_U8C3(4, 4); break;
            case 0x10: STK_U8C3(1, 8); break;
            case 0x11: STK_U8C3(2, 8); break;
            case 0x12: STK_U8C3(4, 8); break;
            case 0x20: STK_U8C3(1, 2); break;
            case 0x22: STK_U8C3(4, 2); break;
            default: STK_U8C3(1, 4); break;
        }
#undef STK_U8C3
        return hipGetLastError();
    }
    if (depth == 16 && a.cn == 3 && a.subpixel_bits == 0 && a.border_mode == STK_BORDER_CONSTANT && a.sw >= 2 && a.sh >= 2 &&
        a.src_stride * 2 * (size_t)a.sh < ((size_t)1 << 31) && a.src_stride < (1u << 23) && a.sh < (1 << 23)) {
        if (a.is_affine) warp_accumulate_u16c3_kernel<true><<<grid, 256, 0, s>>>(a);
        else warp_accumulate_u16c3_kernel<false><<<grid, 256, 0, s>>>(a);
        return hipGetLastError();
    }
    return dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) {
        warp_accumulate_kernel<decltype(t), decltype(ch)::value, false, NoClip><<<grid, 256, 0, s>>>(a, ClipArgs{});
    });
}

}  // namespace stk
