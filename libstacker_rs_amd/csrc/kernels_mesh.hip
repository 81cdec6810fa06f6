// kernels_mesh.hip — local alignment (include/stacker.h, stk_mesh_params): the residual displacement of every
// frame on a grid of nodes, the hole filling of those fields, the box pyramid and the seeded estimation of the
// coarse-to-fine form, and the launch of the folds that apply the fields (the generic kernel's mesh variant,
// Mesh<State> in warp_body.h).
//
// mesh_lk_kernel: one workgroup per node (blockIdx.x) and four table entries (blockIdx.y), one wave per (node, entry).
//   1. the whole workgroup loads frame 0's patch plus a one-pixel halo into LDS as grey bytes (0 outside the frame: a patch
//      pixel has 1 <= x <= w - 2, so its four neighbours are inside). T, Tx and Ty come from there, as integers.
//   2. each wave iterates on its own: its lanes stride over the patch; a live pixel costs the fold's coordinates
//      (warp_coords.inc.h, the fold's own text), four taps of the entry's frame turned into the integer grey, the fold's
//      lerp chain and two f64 products. n, Sxx, Sxy, Syy are integers below 2^31 and are summed as such (the f64 sums of
//      the definition, exactly); bx and by are f64 sums in a fixed order: the lane's pixels in patch order, then the
//      xor-shuffle tree, after which every lane holds the same bits and solves the 2 x 2 system itself.
//   3. lane 0 writes d and the status. No atomics, no traffic between waves after the load: a wave leaves when it stops.
// Every global address is formed from a coordinate that was tested first: the halo load tests (x, y) against the frame,
// a tap is read only where the pixel is live (0 <= ix, ix + 1 <= w - 1, 0 <= iy, iy + 1 <= h - 1).
#include "grey.h"
#include "warp_body.h"

namespace stk {

constexpr int MESH_RMAX = 32;                    // largest radius
constexpr int MESH_SIDE = 2 * MESH_RMAX + 3;     // patch + halo at the largest radius: 67
constexpr int MESH_LS = 68;                      // bytes per LDS row

template <int CN>
__device__ __forceinline__ int mesh_grey_px(const uint8_t* p) {
    if constexpr (CN == 1) return p[0];
    else return grey_u8(p[0], p[1], p[2]);
}

// SEEDED (one level of stk_local_align_pyramid; MeshLkArgs): the frames, w, h and stride are the level's, the node centre
// is the full-resolution one shifted right by the level, d starts at the seed 2 x fields[e][node] (at the top level: 0),
// and a node that fails keeps its seed and its validity byte. Everything inside the iteration is the one text.
template <int CN, bool SEEDED>
__global__ __launch_bounds__(256) void mesh_lk_kernel(MeshLkArgs a) {
    __shared__ uint8_t g0[MESH_SIDE * MESH_LS];
    const int node = blockIdx.x;
    const int nj = node / a.gw, nk = node - nj * a.gw;
    const int cx = SEEDED ? (nk * a.step) >> a.level : nk * a.step, cy = SEEDED ? (nj * a.step) >> a.level : nj * a.step, R = a.radius;
    const int ox = cx - R - 1, oy = cy - R - 1, side = 2 * R + 3;
    {
        const uint8_t* __restrict__ f0 = static_cast<const uint8_t*>(a.frames[0].src);
        for (int i = threadIdx.x; i < side * side; i += 256) {
            const int r = i / side, c = i - r * side;
            const int x = ox + c, y = oy + r;
            int v = 0;
            if ((unsigned)x < (unsigned)a.w && (unsigned)y < (unsigned)a.h) v = mesh_grey_px<CN>(f0 + (size_t)y * a.stride + (size_t)x * CN);
            g0[r * MESH_LS + c] = (uint8_t)v;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int e = __builtin_amdgcn_readfirstlane(1 + (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6));     // wave-uniform
    if (e >= a.n_entries) return;
    const WarpFrame* fr = a.frames + e;
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(fr->src);
    const int xa = max(cx - R, 1), xb = min(cx + R, a.w - 2), ya = max(cy - R, 1), yb = min(cy + R, a.h - 2);
    const int pw = xb - xa + 1, ph = yb - ya + 1;
    float sx = 0.0f, sy = 0.0f;
    if constexpr (SEEDED) {
        if (!a.top) {
            const float* S = a.fields[e];
            sx = 2.0f * S[(size_t)node * 2]; sy = 2.0f * S[(size_t)node * 2 + 1];
        }
    }
    float dx = sx, dy = sy;
    int status = -1;                                 // an empty patch
    if (pw > 0 && ph > 0) {
        const int np = pw * ph;
        for (int it = 1;; it++) {
            int n = 0, sxx = 0, sxy = 0, syy = 0;
            double bx = 0.0, by = 0.0;
            for (int q = lane; q < np; q += 64) {
                const int yy = q / pw, xx = q - yy * pw;
                const int px = xa + xx, py = ya + yy;
                const float fx = (float)px + dx, fy = (float)py + dy;
#define STK_SUBPIX 0
#include "warp_coords.inc.h"
#undef STK_SUBPIX
                (void)w00; (void)w01; (void)w10; (void)w11;
                const bool live = finite && ix >= 0 && ix + 1 <= a.w - 1 && iy >= 0 && iy + 1 <= a.h - 1;
                if (live) {
                    const uint8_t* r0 = src + (size_t)iy * a.stride + (size_t)ix * CN;
                    const uint8_t* r1 = r0 + a.stride;
                    const float p00 = (float)mesh_grey_px<CN>(r0), p01 = (float)mesh_grey_px<CN>(r0 + CN);
                    const float p10 = (float)mesh_grey_px<CN>(r1), p11 = (float)mesh_grey_px<CN>(r1 + CN);
                    const float t0 = __builtin_fmaf(ax, p01 - p00, p00);
                    const float t1 = __builtin_fmaf(ax, p11 - p10, p10);
                    const float I = __builtin_fmaf(ay, t1 - t0, t0);
                    const uint8_t* t = &g0[(py - oy) * MESH_LS + (px - ox)];
                    const int tx = (int)t[1] - (int)t[-1], ty = (int)t[MESH_LS] - (int)t[-MESH_LS];
                    const float err = I - (float)(int)t[0];
                    n += 1; sxx += tx * tx; sxy += tx * ty; syy += ty * ty;
                    bx = bx + (double)tx * (double)err;
                    by = by + (double)ty * (double)err;
                }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                n += __shfl_xor(n, m, 64); sxx += __shfl_xor(sxx, m, 64); sxy += __shfl_xor(sxy, m, 64); syy += __shfl_xor(syy, m, 64);
                bx = bx + __shfl_xor(bx, m, 64);
                by = by + __shfl_xor(by, m, 64);
            }
            if (2 * n < np) { status = -2; break; }
            const double N = (double)n, Sxx = (double)sxx, Sxy = (double)sxy, Syy = (double)syy;
            const double dif = Sxx - Syy;
            const double lam = 0.5 * ((Sxx + Syy) - __builtin_sqrt(dif * dif + 4.0 * (Sxy * Sxy)));
            const double det = Sxx * Syy - Sxy * Sxy;
            if (det <= 0.0 || lam < a.min_eig4 * N) { status = -3; break; }
            const double ddx = 2.0 * (Syy * bx - Sxy * by) / det;
            const double ddy = 2.0 * (Sxx * by - Sxy * bx) / det;
            dx = (float)((double)dx - ddx);
            dy = (float)((double)dy - ddy);
            if (!((double)dx * (double)dx + (double)dy * (double)dy <= a.max_shift2)) { status = -4; break; }
            status = it;
            if (ddx * ddx + ddy * ddy < a.eps2 || it >= a.max_iters) break;
        }
    }
    if (status < 0) { dx = sx; dy = sy; }
    if (lane == 0) {
        float* D = a.fields[e];
        D[(size_t)node * 2] = dx; D[(size_t)node * 2 + 1] = dy;
        if (a.status && a.status[e]) a.status[e][node] = status;
        if constexpr (SEEDED) {
            if (status > 0) a.valid[e][node] = 1;
            else if (a.top) a.valid[e][node] = 0;
        }
    }
}

hipError_t launch_mesh_lk(const MeshLkArgs& a, int cn, hipStream_t s) {
    if (a.n_entries < 2 || a.radius < 2 || a.radius > MESH_RMAX || a.gw <= 0 || a.gh <= 0 || (size_t)a.gw * a.gh > 0x7fffffffu ||
        (a.n_entries + 2) / 4 > 65535)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.gw * a.gh), (unsigned)((a.n_entries - 1 + 3) / 4));
    if (cn == 1) mesh_lk_kernel<1, false><<<grid, 256, 0, s>>>(a);
    else if (cn == 3) mesh_lk_kernel<3, false><<<grid, 256, 0, s>>>(a);
    else if (cn == 4) mesh_lk_kernel<4, false><<<grid, 256, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_mesh_lk_seeded(const MeshLkArgs& a, int cn, hipStream_t s) {
    if (a.n_entries < 2 || a.radius < 2 || a.radius > MESH_RMAX || a.gw <= 0 || a.gh <= 0 || (size_t)a.gw * a.gh > 0x7fffffffu ||
        (a.n_entries + 2) / 4 > 65535 || !a.valid || !a.fields || a.level < 0 || a.level > 3 || a.w < 3 || a.h < 3)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.gw * a.gh), (unsigned)((a.n_entries - 1 + 3) / 4));
    if (cn == 1) mesh_lk_kernel<1, true><<<grid, 256, 0, s>>>(a);
    else if (cn == 3) mesh_lk_kernel<3, true><<<grid, 256, 0, s>>>(a);
    else if (cn == 4) mesh_lk_kernel<4, true><<<grid, 256, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// Box pyramid of the integer grey: one workgroup owns a 64 x 64 tile of the frame and every level's part below it (32 x 32,
// 16 x 16, 8 x 8). The tile is read once, four pixels per thread and step: with a dword-aligned frame those are CN dword
// loads (12 bytes of BGR are four whole pixels), else byte loads; the greys go to LDS four to a dword. Level 1 is reduced
// four outputs per thread from two 8-byte LDS reads and stored as a dword where the plane's address allows; levels 2 and 3
// are one output per thread. A barrier separates the levels. Every global address is formed from a coordinate that was
// tested against its level's size first; a level pixel inside its plane reads only pixels inside the level above
// (2 (w >> l) <= w >> (l - 1)), so the zeros that stand for pixels outside the frame never reach a stored value.
template <int CN>
__global__ __launch_bounds__(256) void mesh_pyr_kernel(MeshPyrArgs a) {
    __shared__ uint32_t l0[64 * 16];
    __shared__ uint32_t l1w[32 * 8];
    __shared__ uint8_t l2[16 * 16];
    const int e = a.first + (int)blockIdx.z;
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(a.frames[e].src);
    uint8_t* __restrict__ out = a.planes + (size_t)e * a.entry_stride;
    const int x0 = (int)blockIdx.x * 64, y0 = (int)blockIdx.y * 64;
    const bool aligned = (((size_t)src | a.stride) & 3) == 0;
    for (int g = threadIdx.x; g < 64 * 16; g += 256) {
        const int x = x0 + (g & 15) * 4, y = y0 + (g >> 4);
        uint32_t v = 0;
        if (y < a.h && x < a.w) {
            const uint8_t* p = src + (size_t)y * a.stride + (size_t)x * CN;
            if (aligned && x + 3 < a.w) {                 // x is a multiple of 4: p is dword-aligned for every CN
                const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
                if constexpr (CN == 1) v = q[0];
                else if constexpr (CN == 3) {
                    const uint32_t d[3] = {q[0], q[1], q[2]};
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int i = 3 * k;
                        const uint32_t b = (d[i >> 2] >> ((i & 3) * 8)) & 255u, gg = (d[(i + 1) >> 2] >> (((i + 1) & 3) * 8)) & 255u,
                                       r = (d[(i + 2) >> 2] >> (((i + 2) & 3) * 8)) & 255u;
                        v |= (uint32_t)grey_u8(b, gg, r) << (8 * k);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t d = q[k];
                        v |= (uint32_t)grey_u8(d & 255u, (d >> 8) & 255u, (d >> 16) & 255u) << (8 * k);
                    }
                }
            } else {
                for (int k = 0; k < 4; k++)
                    if (x + k < a.w) v |= (uint32_t)mesh_grey_px<CN>(p + (size_t)k * CN) << (8 * k);
            }
        }
        l0[g] = v;
    }
    __syncthreads();
    {
        const int r = threadIdx.x >> 3, cg = threadIdx.x & 7;
        const uint32_t t0 = l0[(2 * r) * 16 + 2 * cg], t1 = l0[(2 * r) * 16 + 2 * cg + 1];
        const uint32_t b0 = l0[(2 * r + 1) * 16 + 2 * cg], b1 = l0[(2 * r + 1) * 16 + 2 * cg + 1];
        auto box = [](uint32_t t, uint32_t b, int sh) {
            return (((t >> sh) & 255u) + ((t >> (sh + 8)) & 255u) + ((b >> sh) & 255u) + ((b >> (sh + 8)) & 255u) + 2u) >> 2;
        };
        const uint32_t v = box(t0, b0, 0) | (box(t0, b0, 16) << 8) | (box(t1, b1, 0) << 16) | (box(t1, b1, 16) << 24);
        l1w[r * 8 + cg] = v;
        const int w1 = a.w >> 1, h1 = a.h >> 1, X = (x0 >> 1) + 4 * cg, Y = (y0 >> 1) + r;
        if (Y < h1 && X < w1) {
            uint8_t* o = out + (size_t)Y * w1 + X;
            if (X + 3 < w1 && ((size_t)o & 3) == 0) *reinterpret_cast<uint32_t*>(o) = v;
            else
                for (int k = 0; k < 4; k++)
                    if (X + k < w1) o[k] = (uint8_t)(v >> (8 * k));
        }
    }
    if (a.levels > 2) {
        __syncthreads();
        const uint8_t* l1 = reinterpret_cast<const uint8_t*>(l1w);
        const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
        const uint32_t v = ((uint32_t)l1[(2 * r) * 32 + 2 * c] + l1[(2 * r) * 32 + 2 * c + 1] + l1[(2 * r + 1) * 32 + 2 * c] +
                            l1[(2 * r + 1) * 32 + 2 * c + 1] + 2u) >> 2;
        l2[threadIdx.x] = (uint8_t)v;
        const int w2 = a.w >> 2, h2 = a.h >> 2, X = (x0 >> 2) + c, Y = (y0 >> 2) + r;
        if (Y < h2 && X < w2) out[mesh_pyr_offset(a.w, a.h, 2) + (size_t)Y * w2 + X] = (uint8_t)v;
    }
    if (a.levels > 3) {
        __syncthreads();
        if (threadIdx.x < 64) {
            const int r = threadIdx.x >> 3, c = threadIdx.x & 7;
            const uint32_t v = ((uint32_t)l2[(2 * r) * 16 + 2 * c] + l2[(2 * r) * 16 + 2 * c + 1] + l2[(2 * r + 1) * 16 + 2 * c] +
                                l2[(2 * r + 1) * 16 + 2 * c + 1] + 2u) >> 2;
            const int w3 = a.w >> 3, h3 = a.h >> 3, X = (x0 >> 3) + c, Y = (y0 >> 3) + r;
            if (Y < h3 && X < w3) out[mesh_pyr_offset(a.w, a.h, 3) + (size_t)Y * w3 + X] = (uint8_t)v;
        }
    }
}

hipError_t launch_mesh_pyr(const MeshPyrArgs& a, int cn, hipStream_t s) {
    if (a.levels < 2 || a.n <= 0) return hipSuccess;
    if (a.levels > 4 || !a.frames || !a.planes || a.first < 0 || a.n > 65535 || (a.w >> (a.levels - 1)) < 1 || (a.h >> (a.levels - 1)) < 1 ||
        a.stride < (size_t)a.w * cn || a.entry_stride < mesh_pyr_offset(a.w, a.h, a.levels))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.w + 63) / 64), (unsigned)((a.h + 63) / 64), (unsigned)a.n);
    if (grid.y > 65535) return hipErrorInvalidValue;
    if (cn == 1) mesh_pyr_kernel<1><<<grid, 256, 0, s>>>(a);
    else if (cn == 3) mesh_pyr_kernel<3><<<grid, 256, 0, s>>>(a);
    else if (cn == 4) mesh_pyr_kernel<4><<<grid, 256, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// Hole filling: one workgroup per field (blockIdx.x + 1 = the table entry). Jacobi passes between the field itself and a
// scratch copy, the validity alongside as bytes; the workgroup's barrier orders a pass's writes before the next pass's
// reads. A node that is valid is copied; a hole takes the [1 2 1]^T [1 2 1] mean of its valid in-grid neighbours, row-major.
// valid != null: the validity comes from valid[e] instead of status > 0 and goes back there after the last pass.
__global__ __launch_bounds__(256) void mesh_fill_kernel(float* const* fields, const int* const* status, uint8_t* const* valid, int gw, int gh,
                                                        int passes, char* scratch, size_t scratch_stride) {
    const int e = 1 + blockIdx.x, nn = gw * gh;
    float* A = fields[e];
    const int* __restrict__ st = valid ? nullptr : status[e];
    float* B = reinterpret_cast<float*>(scratch + (size_t)blockIdx.x * scratch_stride);
    uint8_t* ms = reinterpret_cast<uint8_t*>(B + (size_t)nn * 2);
    uint8_t* md = ms + nn;
    for (int i = threadIdx.x; i < nn; i += 256) ms[i] = valid ? valid[e][i] : (st[i] > 0 ? 1 : 0);
    __syncthreads();
    float* src = A;
    float* dst = B;
    for (int p = 0; p < passes; p++) {
        for (int i = threadIdx.x; i < nn; i += 256) {
            float d0 = src[2 * i], d1 = src[2 * i + 1];
            uint8_t m = ms[i];
            if (!m) {
                const int j = i / gw, k = i - j * gw;
                float den = 0.0f, n0 = 0.0f, n1 = 0.0f;
                for (int dj = -1; dj <= 1; dj++)
                    for (int dk = -1; dk <= 1; dk++) {
                        const int jj = j + dj, kk = k + dk;
                        if ((unsigned)jj >= (unsigned)gh || (unsigned)kk >= (unsigned)gw) continue;
                        const int q = jj * gw + kk;
                        if (!ms[q]) continue;
                        const float wgt = (float)((2 - (dj < 0 ? -dj : dj)) * (2 - (dk < 0 ? -dk : dk)));
                        den = den + wgt;
                        n0 = n0 + wgt * src[2 * q];
                        n1 = n1 + wgt * src[2 * q + 1];
                    }
                if (den > 0.0f) { d0 = n0 / den; d1 = n1 / den; m = 1; }
            }
            dst[2 * i] = d0; dst[2 * i + 1] = d1; md[i] = m;
        }
        __syncthreads();
        float* t = src; src = dst; dst = t;
        uint8_t* u = ms; ms = md; md = u;
    }
    if (src != A)
        for (int i = threadIdx.x; i < 2 * nn; i += 256) A[i] = src[i];
    if (valid)
        for (int i = threadIdx.x; i < nn; i += 256) valid[e][i] = ms[i];
}

hipError_t launch_mesh_fill(float* const* fields, const int* const* status, int n_entries, int gw, int gh, int passes, void* scratch,
                            hipStream_t s) {
    if (n_entries < 2 || passes <= 0) return hipSuccess;
    if (!fields || !status || !scratch || gw <= 0 || gh <= 0) return hipErrorInvalidValue;
    mesh_fill_kernel<<<(unsigned)(n_entries - 1), 256, 0, s>>>(fields, status, nullptr, gw, gh, passes, static_cast<char*>(scratch),
                                                                mesh_fill_scratch_bytes(gw, gh));
    return hipGetLastError();
}

hipError_t launch_mesh_fill_valid(float* const* fields, uint8_t* const* valid, int n_entries, int gw, int gh, int passes, void* scratch,
                                  hipStream_t s) {
    if (n_entries < 2 || passes <= 0) return hipSuccess;
    if (!fields || !valid || !scratch || gw <= 0 || gh <= 0) return hipErrorInvalidValue;
    mesh_fill_kernel<<<(unsigned)(n_entries - 1), 256, 0, s>>>(fields, nullptr, valid, gw, gh, passes, static_cast<char*>(scratch),
                                                                mesh_fill_scratch_bytes(gw, gh));
    return hipGetLastError();
}

// The mesh folds: the generic kernel only (the u8 BGR fast kernels and the bicubic kernels do not serve them).
hipError_t launch_mesh_fold(const WarpArgs& a, const ClipArgs& c, int depth, bool local, hipStream_t s) {
    if (a.n_frames <= 0 || !c.fields || c.mesh_gw <= 0 || c.mesh_gh <= 0 || a.interp != STK_INTER_LINEAR || a.subpixel_bits != 0)
        return hipErrorInvalidValue;
    if (local ? (!c.maps || c.power < 1 || c.power > 4) : !a.acc) return hipErrorInvalidValue;
    const dim3 grid((a.dw + 63) / 64, (a.dh + 3) / 4);
    return dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) {
        constexpr int CN = decltype(ch)::value;
        if (local) warp_accumulate_kernel<decltype(t), CN, true, Mesh<FoldLocal<CN>>><<<grid, 256, 0, s>>>(a, c);
        else warp_accumulate_kernel<decltype(t), CN, false, Mesh<NoClip>><<<grid, 256, 0, s>>>(a, c);
    });
}

}  // namespace stk
