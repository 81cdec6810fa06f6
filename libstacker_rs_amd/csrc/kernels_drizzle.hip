// kernels_drizzle.hip — drizzle integration onto a finer or larger output grid (include/stacker.h, stk_drizzle_params;
// DESIGN §4.14). A gather: one thread owns one OUTPUT pixel and loops over the frame table in fold order, as every other
// fold here does; no scatter, no atomics, the same bits whatever the launch shape. Launch shape of the fold: 64 x 4
// threads, a wave is 64 consecutive pixels of one output row.
// Per entry:
//   * the coordinates come from the fold's own fragment (warp_coords.inc.h at STK_SUBPIX == 0) with the entry's matrix,
//     which the host composed with the output grid's map;
//   * the three ox and the three oy overlaps are computed once (the weight is separable), with the in-frame test folded
//     into them: a column or row outside the frame has overlap 0;
//   * a wave none of whose pixels has a live column and a live row skips the entry by a vote (an output canvas larger than
//     a frame's image, a frame that does not reach this part of the mosaic);
//   * a tap row or column whose 1-D overlap is 0 is not loaded: at scale 2, pixfrac 0.5 at most two of three per axis are
//     live, under a translation usually one;
//   * affine entries read (hx, hy) from the table; perspective entries compute them from the matrix, (u, v) and W.
// Every live address is inside its frame by construction: ox_a > 0 implies 0 <= jn + a < sw, oy_b > 0 implies
// 0 <= kn + b < sh, and a non-finite coordinate has every overlap 0. The directory compiles with -ffp-contract=off: the
// only fused operations are the fragment's and the field sample's.
// MESH (stk_mesh_drizzle_stack): an entry with a displacement field runs the fragment at the output
// coordinate moved by s x the field's bilinear sample at the pixel's frame-0 coordinate, and takes its footprint from the
// local Jacobian times the displacement's own. What depends on the pixel alone (the clamped frame-0 coordinate, the four
// node offsets, the two fractions) is computed once in front of the frame loop; an entry costs eight f32 loads and the
// lerp chains. Every field address comes from the clamped coordinate: 0 <= k <= k1 <= gw - 1, 0 <= j <= j1 <= gh - 1.
// An entry without a field is the plain kernel's arithmetic.
#include "drizzle.h"
#include "warp_body.h"

namespace stk {

template <typename T, int CN, bool PERSPECTIVE, bool MAPS, bool MESH = false>
__global__ __launch_bounds__(256) void drizzle_kernel(DrizzleArgs da) {
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= da.ow || py >= da.oh) return;
    const float fx0 = (float)px, fy0 = (float)py;
    // MESH: the pixel's place in the node grid. o00 .. o11 index the four nodes' dx; ivx, ivy are 1 / step, or 0 along an
    // axis on which the frame-0 coordinate was clamped (the slope there is 0)
    int o00 = 0, o01 = 0, o10 = 0, o11 = 0;
    float mu = 0.0f, mv = 0.0f, ivx = 0.0f, ivy = 0.0f;
    if constexpr (MESH) {
        const float x0 = fx0 * da.mesh_g + da.mesh_tx, y0 = fy0 * da.mesh_g + da.mesh_ty;
        const float xc = fminf(fmaxf(x0, 0.0f), (float)(da.sw - 1)), yc = fminf(fmaxf(y0, 0.0f), (float)(da.sh - 1));
        const int k = (int)xc >> da.mesh_shift, j = (int)yc >> da.mesh_shift;
        const int k1 = min(k + 1, da.mesh_gw - 1), j1 = min(j + 1, da.mesh_gh - 1);
        mu = (xc - (float)(k << da.mesh_shift)) * da.mesh_inv;
        mv = (yc - (float)(j << da.mesh_shift)) * da.mesh_inv;
        ivx = x0 == xc ? da.mesh_inv : 0.0f;
        ivy = y0 == yc ? da.mesh_inv : 0.0f;
        o00 = (j * da.mesh_gw + k) * 2; o01 = (j * da.mesh_gw + k1) * 2;
        o10 = (j1 * da.mesh_gw + k) * 2; o11 = (j1 * da.mesh_gw + k1) * 2;
    }
    const float hp = da.hp, hmax = da.hmax, alpha = da.alpha;
    const int sw = da.sw, sh = da.sh;
    float num[CN], den = 0.0f;
#pragma unroll
    for (int c = 0; c < CN; c++) num[c] = 0.0f;

    for (int f = 0; f < da.n_frames; f++) {
        const stk_frame_weight* __restrict__ rec = da.coef + f;
        const float wi = rec->weight;
        if (!(wi > 0.0f)) continue;                                  // (uniform)
        const WarpFrame* fr = da.frames + f;
        float fx = fx0, fy = fy0;
        float e00 = 1.0f, e01 = 0.0f, e10 = 0.0f, e11 = 1.0f;        // E = I + grad d: e_cr = the slope of component c along axis r
        bool displaced = false;                                       // (uniform)
        if constexpr (MESH) {
            const float* __restrict__ D = da.fields[f];
            displaced = D != nullptr;
            if (displaced) {
                float dd[2], gx[2], gy[2];
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const float n00 = D[o00 + c], n01 = D[o01 + c], n10 = D[o10 + c], n11 = D[o11 + c];
                    const float ac = n01 - n00, bc = n11 - n10, pc = n10 - n00, qc = n11 - n01;
                    const float t0 = __builtin_fmaf(mu, ac, n00);
                    const float t1 = __builtin_fmaf(mu, bc, n10);
                    dd[c] = __builtin_fmaf(mv, t1 - t0, t0);
                    gx[c] = __builtin_fmaf(mv, bc - ac, ac) * ivx;
                    gy[c] = __builtin_fmaf(mu, qc - pc, pc) * ivy;
                }
                fx = fx0 + da.mesh_s * dd[0]; fy = fy0 + da.mesh_s * dd[1];
                e00 = 1.0f + gx[0]; e01 = gy[0]; e10 = gx[1]; e11 = 1.0f + gy[1];
            }
        }
        // the fragment reads a.is_affine: a constant here, so that the division exists in the perspective kernels only
        constexpr struct { int is_affine; } a{PERSPECTIVE ? 0 : 1};
#define STK_SUBPIX 0
#include "warp_coords.inc.h"
#undef STK_SUBPIX
        (void)w00; (void)w01; (void)w10; (void)w11;
        // local coordinates: the nearest source pixel and the offset from it (exact)
        const bool upx = ax >= 0.5f, upy = ay >= 0.5f;
        const int jn = upx ? ix + 1 : ix, kn = upy ? iy + 1 : iy;
        const float d = upx ? ax - 1.0f : ax, e = upy ? ay - 1.0f : ay;
        float hx, hy;
        if constexpr (PERSPECTIVE) {
            const float uu = (float)jn + d, vv = (float)kn + e;
            const float W = (fr->M[6] * fx + fr->M[7] * fy) + fr->M[8];
            const float rw = 1.0f / __builtin_fabsf(W);
            if (MESH && displaced) {
                const float j00 = fr->M[0] - uu * fr->M[6], j01 = fr->M[1] - uu * fr->M[7];
                const float j10 = fr->M[3] - vv * fr->M[6], j11 = fr->M[4] - vv * fr->M[7];
                hx = fminf(((__builtin_fabsf(j00 * e00 + j01 * e10) + __builtin_fabsf(j00 * e01 + j01 * e11)) * rw) * 0.5f, hmax);
                hy = fminf(((__builtin_fabsf(j10 * e00 + j11 * e10) + __builtin_fabsf(j10 * e01 + j11 * e11)) * rw) * 0.5f, hmax);
            } else {
                hx = fminf(((__builtin_fabsf(fr->M[0] - uu * fr->M[6]) + __builtin_fabsf(fr->M[1] - uu * fr->M[7])) * rw) * 0.5f, hmax);
                hy = fminf(((__builtin_fabsf(fr->M[3] - vv * fr->M[6]) + __builtin_fabsf(fr->M[4] - vv * fr->M[7])) * rw) * 0.5f, hmax);
            }
        } else if (MESH && displaced) {
            const float j00 = fr->M[0], j01 = fr->M[1], j10 = fr->M[3], j11 = fr->M[4];
            hx = fminf((__builtin_fabsf(j00 * e00 + j01 * e10) + __builtin_fabsf(j00 * e01 + j01 * e11)) * 0.5f, hmax);
            hy = fminf((__builtin_fabsf(j10 * e00 + j11 * e10) + __builtin_fabsf(j10 * e01 + j11 * e11)) * 0.5f, hmax);
        } else {
            hx = da.foot[2 * f]; hy = da.foot[2 * f + 1];
        }
        const float lox = d - hx, hix = d + hx, loy = e - hy, hiy = e + hy;
        float ox[3], oy[3];
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const float c = (float)(t - 1);
            const float vx = fmaxf(0.0f, fminf(hix, c + hp) - fmaxf(lox, c - hp));
            const float vy = fmaxf(0.0f, fminf(hiy, c + hp) - fmaxf(loy, c - hp));
            ox[t] = (finite & ((unsigned)(jn + t - 1) < (unsigned)sw)) ? vx : 0.0f;
            oy[t] = (finite & ((unsigned)(kn + t - 1) < (unsigned)sh)) ? vy : 0.0f;
        }
        const bool live = ((ox[0] > 0.0f) | (ox[1] > 0.0f) | (ox[2] > 0.0f)) & ((oy[0] > 0.0f) | (oy[1] > 0.0f) | (oy[2] > 0.0f));
        if (__ballot(live) == 0) continue;                           // no pixel of this wave has a tap in this frame

        const T* __restrict__ src = (const T*)fr->src;
        const float* __restrict__ mp = nullptr;
        if constexpr (MAPS) mp = da.maps[f];
        float s[CN], k = 0.0f;
#pragma unroll
        for (int c = 0; c < CN; c++) s[c] = 0.0f;
#pragma unroll
        for (int b = 0; b < 3; b++) {
            if (!(oy[b] > 0.0f)) continue;
            const int yy = kn + b - 1;
            const T* __restrict__ row = src + (size_t)yy * da.src_stride;
#pragma unroll
            for (int t = 0; t < 3; t++) {
                if (!(ox[t] > 0.0f)) continue;
                const int xx = jn + t - 1;
                float wgt = ox[t] * oy[b];
                if constexpr (MAPS) {
                    if (mp) {
                        const float mv = mp[(size_t)yy * sw + xx];
                        if (!(mv > 0.0f)) continue;
                        wgt = wgt * mv;
                    }
                }
                const T* __restrict__ p = row + (size_t)xx * CN;
#pragma unroll
                for (int c = 0; c < CN; c++) {
                    const float v = (float)p[c] * alpha;
                    s[c] = s[c] + wgt * v;
                }
                k = k + wgt;
            }
        }
        if (k > 0.0f) {
#pragma unroll
            for (int c = 0; c < CN; c++) num[c] = num[c] + wi * (s[c] * rec->gain[c] + rec->offset[c] * k);
            den = den + wi * k;
        }
    }
    float* __restrict__ o = da.out + ((size_t)py * da.ow + px) * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) o[c] = den > 0.0f ? num[c] / den : da.fill;
    if (da.den) da.den[(size_t)py * da.ow + px] = den;
}

template <typename T, int CN>
static void drizzle_launch(const DrizzleArgs& a, dim3 grid, hipStream_t s) {
    const bool persp = !a.is_affine, maps = a.maps != nullptr;
    if (a.fields) {
        if (persp && maps) drizzle_kernel<T, CN, true, true, true><<<grid, 256, 0, s>>>(a);
        else if (persp) drizzle_kernel<T, CN, true, false, true><<<grid, 256, 0, s>>>(a);
        else if (maps) drizzle_kernel<T, CN, false, true, true><<<grid, 256, 0, s>>>(a);
        else drizzle_kernel<T, CN, false, false, true><<<grid, 256, 0, s>>>(a);
        return;
    }
    if (persp && maps) drizzle_kernel<T, CN, true, true><<<grid, 256, 0, s>>>(a);
    else if (persp) drizzle_kernel<T, CN, true, false><<<grid, 256, 0, s>>>(a);
    else if (maps) drizzle_kernel<T, CN, false, true><<<grid, 256, 0, s>>>(a);
    else drizzle_kernel<T, CN, false, false><<<grid, 256, 0, s>>>(a);
}

// A missing kernel is an error: every depth and channel count the entry points admit has its instantiation here.
hipError_t launch_drizzle(const DrizzleArgs& a, int depth, hipStream_t s) {
    if (a.n_frames <= 0 || a.ow <= 0 || a.oh <= 0 || a.ow > 32768 || a.oh > 32768 || !a.frames || !a.coef || !a.out ||
        (a.is_affine && !a.foot))
        return hipErrorInvalidValue;
    if (a.fields && (a.mesh_shift < 3 || a.mesh_shift > 8 || a.mesh_gw != ((a.sw - 1 + (1 << a.mesh_shift) - 1) >> a.mesh_shift) + 1 ||
                     a.mesh_gh != ((a.sh - 1 + (1 << a.mesh_shift) - 1) >> a.mesh_shift) + 1))
        return hipErrorInvalidValue;                                 // the field planes are read on this grid and no other
    const dim3 grid((a.ow + 63) / 64, (a.oh + 3) / 4);
    return dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) { drizzle_launch<decltype(t), decltype(ch)::value>(a, grid, s); });
}

}  // namespace stk
