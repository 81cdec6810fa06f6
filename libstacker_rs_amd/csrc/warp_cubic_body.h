// warp_cubic_body.h — the bicubic fold (option "warp_interpolation" = STK_INTER_CUBIC; definition: include/stacker.h,
// "Bicubic fold"). A kernel template of its own next to warp_body.h's, speaking the same hooks (begin / entry / coords /
// add / finish) and asking the same traits of its state (FoldTraits; the table of states is at the top of warp_body.h),
// so every combine built on the fold gets the cubic sample from one source; the linear kernels are not touched (no
// run-time branch in them: their instantiations keep their instructions).
//   * warp_accumulate_cubic_kernel<T, CN, CLIP, ClipState>: every depth, 1 / 3 / 4 channels, every border mode and every
//     state of the generic linear kernel, the moments mode's stepped walk included. One thread per destination pixel.
// The coordinates are the linear fold's (warp_coords.inc.h, exact mode only: the host refuses cubic with
// warp_subpixel_bits = 5). Where the 4 x 4 footprint is not wholly inside the frame the thread takes the linear sample —
// warp_linear_sample.inc.h, the linear kernel's own text — so the one-pixel ring, frames below 4 pixels, non-finite
// coordinates and every border rule are the linear fold's bit for bit, and kappa is the linear fold's everywhere (it is
// exactly 1.0f wherever the footprint is inside).
//   * warp_accumulate_cubic_u8c3_kernel<AFFINE, WU, MODE, FastState>: the u8 BGR BORDER_CONSTANT fast kernel, below.
#pragma once
#include "warp_body.h"

namespace stk {

// The four weights of OpenCV's INTER_CUBIC kernel (A = -0.75) in factored form, for the fraction t; every operation is
// rounded on its own except the written fmas. t = 0: (-0, 1, 0, -0); t = 0.5: (-3, 19, 19, -3) / 32, exactly.
__device__ __forceinline__ void cubic_weights(float t, float* w) {
    constexpr float A = -0.75f;
    const float u = 1.0f - t, tt = t * t, uu = u * u;
    w[0] = (A * t) * uu;
    w[1] = __builtin_fmaf(__builtin_fmaf(1.25f, t, -2.25f), tt, 1.0f);
    w[2] = __builtin_fmaf(__builtin_fmaf(1.25f, u, -2.25f), uu, 1.0f);
    w[3] = (A * u) * tt;
}

// (one __global__ template, not a helper shared with the linear kernel: see the note at warp_accumulate_kernel)
template <typename T, int CN, bool CLIP, class ClipState>
__global__ __launch_bounds__(256) void warp_accumulate_cubic_kernel(WarpArgs a, ClipArgs ca) {
    constexpr bool MOMENTS = ClipState::stepped;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if constexpr (ClipState::in_band) y += ca.y0;     // store mode: a band of rows (a.dh = its end)
    if constexpr (!MOMENTS) { if (x >= a.dw || y >= a.dh) return; }
    float* accp = a.acc + (size_t)y * a.acc_stride + (size_t)x * CN;
    float sum[CN];
    ClipState cs;
    if constexpr (CLIP) cs.begin(ca, x, y);
    else {
#pragma unroll
        for (int c = 0; c < CN; c++) sum[c] = a.accumulate ? accp[c] : 0.0f;
    }

    float fx = (float)x, fy = (float)y;
    const int mode = a.border_mode;
    // moments mode: ca.reps stepped rows per thread, each over entry 0 and entry 1 + blockIdx.z (as in the linear kernel)
    int rep = 0;
    do {
    const int px = MOMENTS ? x * ca.step : x, py = MOMENTS ? (y * ca.reps + rep) * ca.step : y;
    if constexpr (MOMENTS) { cs.live = (px < a.dw) & (py < a.dh); fx = (float)px; fy = (float)py; }
    for (int f = 0; f < (MOMENTS ? 2 : a.n_frames); f++) {
        const WarpFrame* fr = a.frames + (MOMENTS ? f * (1 + (int)blockIdx.z) : f);
        const T* __restrict__ src = (const T*)fr->src;
#define STK_SUBPIX 0
#define STK_SAMPLE(c, v) if constexpr (CLIP) cs.add(c, v); else sum[c] = sum[c] + v
#include "warp_coords.inc.h"
        // the 4 x 4 footprint (columns ix - 1 .. ix + 2, rows iy - 1 .. iy + 2) wholly inside the frame; a non-finite
        // coordinate has ix = iy = -100000 and fails by itself
        if (finite & (ix >= 1) & (ix + 2 <= a.sw - 1) & (iy >= 1) & (iy + 2 <= a.sh - 1)) {
            float wx[4], wy[4];
            cubic_weights(ax, wx);
            cubic_weights(ay, wy);
            // every tap is inside the frame: no clamps, no border selects, and kappa is exactly 1
            const T* q = src + (size_t)(iy - 1) * a.src_stride + (size_t)(ix - 1) * CN;
            if constexpr (ClipState::wants_kappa) cs.entry(1.0f);
            // the local mode's weight stays bilinear: the four inner taps of the footprint, all inside
            if constexpr (ClipState::wants_coords) cs.coords(ix, iy, ax, ay, true, false, 0.f, 0.f, 0.f, 0.f, a.sw, a.sh);
#pragma unroll
            for (int c = 0; c < CN; c++) {
                float hr[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const T* qr = q + (size_t)r * a.src_stride + c;
                    const float p0 = (float)qr[0] * a.alpha, p1 = (float)qr[CN] * a.alpha;
                    const float p2 = (float)qr[2 * CN] * a.alpha, p3 = (float)qr[3 * CN] * a.alpha;
                    hr[r] = __builtin_fmaf(wx[3], p3, __builtin_fmaf(wx[2], p2, __builtin_fmaf(wx[1], p1, wx[0] * p0)));
                }
                const float v = __builtin_fmaf(wy[3], hr[3], __builtin_fmaf(wy[2], hr[2], __builtin_fmaf(wy[1], hr[1], wy[0] * hr[0])));
                STK_SAMPLE(c, v);
            }
        } else {
#include "warp_linear_sample.inc.h"
        }
#undef STK_SAMPLE
#undef STK_SUBPIX
    }
    } while (MOMENTS && ++rep < ca.reps);
    if constexpr (CLIP) cs.finish(ca, x, y);
    else {
#pragma unroll
        for (int c = 0; c < CN; c++) accp[c] = sum[c];
    }
}

// -----------------------------------------------------------------------------------------------
// The u8 BGR BORDER_CONSTANT fast kernel of the cubic fold: the generic cubic kernel's bits everywhere, with what the
// linear fast kernel (warp_body.h) does for its instruction count and its loads:
//   * the packed (X, Y) chain and the shared reciprocal chain under WARPFRAME_DIV_IN_RANGE (div2_shared);
//   * a per-wave vote BEFORE any load: the 4 x 4 footprints of all WU frames inside the frame with a row to spare below
//     iy + 2. Such waves load without clamps; a row's four taps are 12 contiguous bytes (B0 G0 R0 B1 | G1 R1 B2 G2 |
//     R2 B3 G3 R3): with WARPFRAME_SRC_ALIGNED4 one 16-byte window from `offset & ~3` covers them wherever they start and
//     v_alignbyte moves them into place (four 16-byte loads per pixel and frame); otherwise a 12-byte unaligned load.
//     The window ends at most 4 bytes behind the row's twelve, hence the spare row: it stays inside the span;
//   * all 4 * WU loads of a group are issued before the first is consumed;
//   * (B, G) of a tap as a register pair through v_pk_mul / v_pk_fma, R apart: per component the generic kernel's
//     operations in the generic kernel's order;
//   * add2 (kappa known to be 1) wherever the footprint is inside, add3 / add3k on the rim.
// Waves that fail the vote go per lane: a lane whose footprint test holds loads its four rows' twelve bytes exactly
// (nothing behind them is read, so the last rows need no back-off) and runs the same arithmetic; a lane whose test fails
// takes the linear sample from warp_linear_sample.inc.h — the text the generic kernels use — through a collecting state.
// -----------------------------------------------------------------------------------------------
struct CubicRows { Tap12 r[4]; };

// the cubic sample of the three channels from four rows of twelve bytes: (B, G) as a pair, R
__device__ __forceinline__ void cubic_u8c3_sample(const CubicRows& w, const float* wx, const float* wy, float alpha, f32x2& vbg, float& vr) {
#define STK_UB(d, k) ((float)(((d) >> (8 * (k))) & 0xffu))                           /* v_cvt_f32_ubyte<k> */
    const f32x2 al2 = {alpha, alpha};
    f32x2 hbg[4];
    float hr[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t A = w.r[r].a, B = w.r[r].b, C = w.r[r].c;
        const f32x2 p0 = f32x2{STK_UB(A, 0), STK_UB(A, 1)} * al2, p1 = f32x2{STK_UB(A, 3), STK_UB(B, 0)} * al2;
        const f32x2 p2 = f32x2{STK_UB(B, 2), STK_UB(B, 3)} * al2, p3 = f32x2{STK_UB(C, 1), STK_UB(C, 2)} * al2;
        hbg[r] = pk_fma(f32x2{wx[3], wx[3]}, p3, pk_fma(f32x2{wx[2], wx[2]}, p2, pk_fma(f32x2{wx[1], wx[1]}, p1, f32x2{wx[0], wx[0]} * p0)));
        const float r0 = STK_UB(A, 2) * alpha, r1 = STK_UB(B, 1) * alpha, r2 = STK_UB(C, 0) * alpha, r3 = STK_UB(C, 3) * alpha;
        hr[r] = __builtin_fmaf(wx[3], r3, __builtin_fmaf(wx[2], r2, __builtin_fmaf(wx[1], r1, wx[0] * r0)));
    }
#undef STK_UB
    vbg = pk_fma(f32x2{wy[3], wy[3]}, hbg[3], pk_fma(f32x2{wy[2], wy[2]}, hbg[2], pk_fma(f32x2{wy[1], wy[1]}, hbg[1], f32x2{wy[0], wy[0]} * hbg[0])));
    vr = __builtin_fmaf(wy[3], hr[3], __builtin_fmaf(wy[2], hr[2], __builtin_fmaf(wy[1], hr[1], wy[0] * hr[0])));
}

// what warp_linear_sample.inc.h hands over, kept for the fast kernel's add3 / add3k hooks; kappa is asked for if the fast
// state asks for it
template <bool KAPPA>
struct LinearCollect : FoldTraits {
    static constexpr bool wants_kappa = KAPPA;
    float v[3], k;
    __device__ __forceinline__ void entry(float kk) { k = kk; }
    __device__ __forceinline__ void add(int c, float s) { v[c] = s; }
};

// WU: frames in flight per lane. MODE = false: the mean fold (running sums into a.acc); true: the hooks of FastState.
template <bool AFFINE, int WU, bool MODE, class FastState>
__global__ __launch_bounds__(256) void warp_accumulate_cubic_u8c3_kernel(WarpArgs a, ClipArgs ca) {
    constexpr bool KAPPA = FastState::wants_kappa;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if constexpr (FastState::in_band) y += ca.y0;      // store mode: a band of rows (a.dh = its end)
    if (x >= a.dw || y >= a.dh) return;
    float* accp = a.acc + (size_t)y * a.acc_stride + (size_t)x * 3;
    f32x2 s01 = {0.f, 0.f};
    float s2 = 0.f;
    FastState st;
    if constexpr (MODE) st.begin(ca, x, y);
    else if (a.accumulate) { s01.x = accp[0]; s01.y = accp[1]; s2 = accp[2]; }
    const float fx = (float)x, fy = (float)y;
    const int sw = a.sw, sh = a.sh;
    const int stride32 = (int)a.src_stride;
    const float alpha = a.alpha;

    for (int f0 = 0; f0 < a.n_frames; f0 += WU) {
        float axs[WU], ays[WU];
        int ixs[WU], iys[WU];
        bool fins[WU];
        bool interior = true;
#pragma unroll
        for (int u = 0; u < WU; u++) {
            const WarpFrame* fr = a.frames + min(f0 + u, a.n_frames - 1);
            // the linear fast kernel's coordinates: packed (X, Y), one reciprocal chain shared by X / W and Y / W
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
            const bool finite = (__builtin_fabsf(X) < 1e9f) & (__builtin_fabsf(Y) < 1e9f);   // false for NaN / inf
            const float flx = __builtin_floorf(X), fly = __builtin_floorf(Y);
            ixs[u] = finite ? (int)flx : -100000; iys[u] = finite ? (int)fly : -100000;
            axs[u] = finite ? X - flx : 0.0f; ays[u] = finite ? Y - fly : 0.0f;
            fins[u] = finite;
            // the footprint inside the frame and a row to spare below it (signed compares: sw - 3 may be negative)
            interior &= (ixs[u] >= 1) & (ixs[u] + 2 <= sw - 1) & (iys[u] >= 1) & (iys[u] + 2 <= sh - 2);
        }
        if (__all(interior)) {
            CubicRows win[WU];
#pragma unroll
            for (int u = 0; u < WU; u++) {
                const WarpFrame* fr = a.frames + min(f0 + u, a.n_frames - 1);
                const uint8_t* __restrict__ src = (const uint8_t*)fr->src;
                // one frame is < 2 GiB (checked by the launcher): 32-bit offsets on the frame's uniform base pointer
                const unsigned o = (unsigned)(__mul24(iys[u] - 1, stride32) + (ixs[u] - 1) * 3);
                if (fr->flags & WARPFRAME_SRC_ALIGNED4) {
                    // (the flag also says that the row stride is a multiple of 4: all four rows' windows are dword-aligned)
                    const unsigned oa = o & ~3u, sft = o & 3u;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        uint32_t t[4];
                        __builtin_memcpy(t, __builtin_assume_aligned(src + (unsigned)(r * stride32) + oa, 4), 16);
                        win[u].r[r] = Tap12{__builtin_amdgcn_alignbyte(t[1], t[0], sft), __builtin_amdgcn_alignbyte(t[2], t[1], sft),
                                            __builtin_amdgcn_alignbyte(t[3], t[2], sft)};
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++) __builtin_memcpy(&win[u].r[r], src + (unsigned)(r * stride32) + o, 12);
                }
            }
#pragma unroll
            for (int u = 0; u < WU; u++) {
                if (f0 + u < a.n_frames) {
                    float wx[4], wy[4], vr;
                    f32x2 vbg;
                    cubic_weights(axs[u], wx);
                    cubic_weights(ays[u], wy);
                    cubic_u8c3_sample(win[u], wx, wy, alpha, vbg, vr);
                    if constexpr (MODE) st.add2(vbg, vr);
                    else { s01 = s01 + vbg; s2 = s2 + vr; }
                }
            }
            continue;
        }
        // rim waves, per lane
#pragma unroll
        for (int u = 0; u < WU; u++) {
            if (f0 + u < a.n_frames) {
                const WarpFrame* fr = a.frames + (f0 + u);
                const int ix = ixs[u], iy = iys[u];
                const float ax = axs[u], ay = ays[u];
                const bool finite = fins[u];
                if (finite & (ix >= 1) & (ix + 2 <= sw - 1) & (iy >= 1) & (iy + 2 <= sh - 1)) {
                    const uint8_t* __restrict__ src = (const uint8_t*)fr->src;
                    const unsigned o = (unsigned)(__mul24(iy - 1, stride32) + (ix - 1) * 3);
                    CubicRows w;
#pragma unroll
                    for (int r = 0; r < 4; r++) __builtin_memcpy(&w.r[r], src + (unsigned)(r * stride32) + o, 12);   // the row's twelve bytes, no more
                    float wx[4], wy[4], vr;
                    f32x2 vbg;
                    cubic_weights(ax, wx);
                    cubic_weights(ay, wy);
                    cubic_u8c3_sample(w, wx, wy, alpha, vbg, vr);
                    if constexpr (MODE) st.add2(vbg, vr);
                    else { s01 = s01 + vbg; s2 = s2 + vr; }
                } else {
                    // the linear sample: the generic kernels' text, collected instead of folded. The names the fragment asks for:
                    typedef uint8_t T;
                    constexpr int CN = 3;
                    constexpr int mode = STK_BORDER_CONSTANT;
                    const T* __restrict__ src = (const T*)fr->src;
                    const float w00 = 0, w01 = 0, w10 = 0, w11 = 0;     // (the classic path's weights: exact coordinates here)
                    LinearCollect<KAPPA> cs;
#define STK_SUBPIX 0
#define STK_SAMPLE(c, v) cs.add(c, v)
#include "warp_linear_sample.inc.h"
#undef STK_SAMPLE
#undef STK_SUBPIX
                    if constexpr (KAPPA) st.add3k(cs.v[0], cs.v[1], cs.v[2], cs.k);
                    else if constexpr (MODE) st.add3(cs.v[0], cs.v[1], cs.v[2]);
                    else { s01.x = s01.x + cs.v[0]; s01.y = s01.y + cs.v[1]; s2 = s2 + cs.v[2]; }
                }
            }
        }
    }
    if constexpr (MODE) st.finish(ca, x, y);
    else { accp[0] = s01.x; accp[1] = s01.y; accp[2] = s2; }
}

// The fast launch: FastState as the linear launcher of the same combine chooses it for its u8 BGR kernel; `grid` is the
// one-wave-per-row-of-64 shape. Two frames in flight: 24 to 32 VGPRs of windows.
template <bool MODE, class FastState>
hipError_t launch_warp_cubic_u8c3(const WarpArgs& a, const ClipArgs& c, dim3 grid, hipStream_t s) {
    if (a.subpixel_bits != 0) return hipErrorInvalidValue;
    if (a.is_affine) warp_accumulate_cubic_u8c3_kernel<true, 2, MODE, FastState><<<grid, 256, 0, s>>>(a, c);
    else warp_accumulate_cubic_u8c3_kernel<false, 2, MODE, FastState><<<grid, 256, 0, s>>>(a, c);
    return hipGetLastError();
}

template <int CN> using NoClipN = NoClip;   // the mean fold's state under the launcher below

// The cubic launch of one fold: State<CN> as the linear launcher of the same combine would choose it for the generic
// kernel, `grid` that launcher's generic grid (the moments pass has a z extent). No launcher hands it a Mesh<> state, and the
// cubic kernel does not ask `displaced`: that there is no cubic mesh fold is a property of the launchers (kernels_mesh.hip
// launches the linear generic kernel only), not of the states.
template <bool CLIP, template <int> class State>
hipError_t launch_warp_cubic(const WarpArgs& a, const ClipArgs& c, int depth, dim3 grid, hipStream_t s) {
    if (a.subpixel_bits != 0) return hipErrorInvalidValue;      // cubic is defined on exact coordinates only
    return dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) {
        constexpr int CN = decltype(ch)::value;
        warp_accumulate_cubic_kernel<decltype(t), CN, CLIP, State<CN>><<<grid, 256, 0, s>>>(a, c);
    });
}

}  // namespace stk
