// warp_body.h — the linear warp fold kernels and the states every combine plugs into them. One source for "the sample":
// whatever a combine does with the aligned frames, it does with the mean fold's samples, computed by the same instructions.
//   G   warp_accumulate_kernel<T, CN, CLIP, State>: the generic kernel (any depth, 1 / 3 / 4 channels, every border mode);
//   F   warp_accumulate_u8c3_kernel<AFFINE, WX, WU, CLIP, State>: the u8 BGR BORDER_CONSTANT fast kernel;
//   C / CF   the bicubic fold's two kernels (warp_cubic_body.h), which speak the same hooks.
// CLIP = false is the mean fold (NoClip: running sums into WarpArgs::acc; these instantiations compile to what they were
// before there were states). CLIP = true hands every sample to the state:
//   begin(ca, x, y) ... per table entry, in frame order: [entry(kappa)] [coords(..)] add(c, v) per channel ... finish(ca, x, y)
// and on F / CF add2((B, G), R) where the kernel knows kappa = 1 (interior), add3(B, G, R) or add3k(B, G, R, kappa) on the
// rim. kappa is the entry's coverage weight (fold_kappa below). What else a state needs from its kernel it declares as
// traits (FoldTraits below); the kernels and the sample fragment ask the traits, never which state they run.
//
//   state                traits                       kernels      launched from
//   NoClip               -                            G F C CF     kernels_warp.hip (the mean)
//   FoldStore<CN>        in_band                      G F C CF     kernels_quantile.hip (launch_fold)
//   FoldStoreW<CN>       in_band wants_kappa          G F C CF     kernels_quantile.hip (launch_fold)
//   FoldStoreNorm<CN>    in_band wants_kappa          G C          kernels_local_norm.hip
//   FoldWeighted<CN>     wants_kappa                  G F C CF     kernels_weighted.hip (launch_fold)
//   FoldNorm<CN>         wants_kappa                  G C          kernels_local_norm.hip
//   FoldLocal<CN>        wants_kappa wants_coords     G C          kernels_local.hip
//   FoldMoments<CN>      wants_kappa stepped          G C          kernels_weighted.hip
//   Mesh<NoClip>         displaced                    G            kernels_mesh.hip
//   Mesh<FoldLocal<CN>>  displaced + FoldLocal's      G            kernels_mesh.hip
//   ClipGeneric<CN> / ClipU8C3        -               G C / F CF   kernels_clip.hip (launch_fold)
//   ClipWGeneric<CN> / ClipWU8C3      wants_kappa     G C / F CF   kernels_clip.hip (launch_fold)
//   ClipNorm<CN> / ClipNormU8C3       wants_kappa     G C / F CF   kernels_clip.hip (launch_fold)
//   (CellMoments<CN>     wants_kappa                  local_moments_kernel, kernels_local_norm.hip: the sample fragment only)
// The pairs FoldWeighted / FoldNorm, FoldStoreW / FoldStoreNorm, ClipWGeneric / ClipNorm and ClipWU8C3 / ClipNormU8C3 are
// one state each over two coefficient sources (FromRecord, FromPlane below). A state without add2 / add3 / add3k is for the
// generic kernels only: a fast launch with it does not compile. kernels_clip.hip pins the table as static_asserts.
//
// To add a state: derive from FoldTraits, set the traits, write the hooks; launch it through launch_fold (fold_launch.h) if
// it has a fast form, else as kernels_local.hip does; add its lines to the table and to the asserts.
//
// What the generic kernels share with each other (and with local_moments_kernel) is shared as text, in two fragments that
// they include inside their frame loops: the coordinates and the bilinear sample (warp_coords.inc.h,
// warp_linear_sample.inc.h). Text, not helper functions: see the note at warp_accumulate_kernel.
#pragma once
#include "common.h"

namespace stk {

// What a state asks of the kernel that runs it, as compile-time members; a state overrides the ones it wants. The kernels
// and the sample fragment ask these and nothing else about a state.
struct FoldTraits {
    static constexpr bool wants_kappa = false;    // entry(kappa) before the entry's samples; add3k, not add3, on the fast kernels' rims
    static constexpr bool wants_coords = false;   // coords(..) after entry: the entry's coordinates
    static constexpr bool in_band = false;        // rows start at ClipArgs::y0: a store launch covers a band of the destination
    static constexpr bool stepped = false;        // the moments walk: (x, y) index the stepped grid, entry 0 against entry 1 + blockIdx.z
    static constexpr bool displaced = false;      // coordinates displaced by the entry's field (Mesh<> below)
};

// The mesh variant of the generic kernel (kernels_mesh.hip; definition: include/stacker.h, "Mesh fold"): a state wrapped in
// Mesh<> runs the same hooks at coordinates displaced by the entry's field. A wrapper around the state, not a further
// template parameter: the instantiations without it keep their names and their instructions.
template <class State> struct Mesh : State { static constexpr bool displaced = true; };

// The coverage weight of one sample: what the fold's interpolation (lerp chain, or the classic four-weight sum) gives for a
// frame whose every value is 1.0f under alpha = 1 and BORDER_CONSTANT 0; i00 .. i11 say which taps are inside the frame.
__device__ __forceinline__ float fold_kappa(bool i00, bool i01, bool i10, bool i11, bool classic, float ax, float ay,
                                            float w00, float w01, float w10, float w11) {
    const float p00 = i00 ? 1.0f : 0.0f, p01 = i01 ? 1.0f : 0.0f, p10 = i10 ? 1.0f : 0.0f, p11 = i11 ? 1.0f : 0.0f;
    if (classic) return p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11;
    const float t0 = __builtin_fmaf(ax, p01 - p00, p00);
    const float t1 = __builtin_fmaf(ax, p11 - p10, p10);
    return __builtin_fmaf(ay, t1 - t0, t0);
}

__device__ __forceinline__ int border_interp(int p, int len, int mode) {
    if ((unsigned)p < (unsigned)len) return p;
    if (mode == STK_BORDER_REPLICATE) return p < 0 ? 0 : len - 1;
    if (mode == STK_BORDER_REFLECT || mode == STK_BORDER_REFLECT_101) {
        const int delta = mode == STK_BORDER_REFLECT_101;
        if (len == 1) return 0;
        do {
            if (p < 0) p = -p - 1 + delta;
            else p = len - 1 - (p - len) - delta;
        } while ((unsigned)p >= (unsigned)len);
        return p;
    }
    if (mode == STK_BORDER_WRAP) {
        if (p < 0) p -= ((p - len + 1) / len) * len;
        if (p >= len) p %= len;
        return p;
    }
    return -1;   // BORDER_CONSTANT
}

__device__ __forceinline__ int sat_int_d(double v) {
    if (!(v > -2147483648.0)) return (int)0x80000000;
    if (!(v < 2147483647.0)) return 0x7fffffff;
    return (int)__builtin_rint(v);
}

// The mesh fold's coordinates of destination pixel (x, y) under table entry f (include/stacker.h, "Mesh fold"): the
// bilinear sample of the entry's node field (ClipArgs::fields[f]: mesh_gh x mesh_gw x 2 f32, node spacing 1 << mesh_shift;
// a null plane = no displacement), lerp chain by fma, added to the pixel's own coordinates.
struct MeshXY { float x, y; };
__device__ __forceinline__ MeshXY mesh_displace(const ClipArgs& ca, int f, int x, int y) {
    MeshXY r{(float)x, (float)y};
    const float* __restrict__ D = ca.fields[f];
    if (D) {
        const int k = x >> ca.mesh_shift, j = y >> ca.mesh_shift;
        const int k1 = min(k + 1, ca.mesh_gw - 1), j1 = min(j + 1, ca.mesh_gh - 1);
        const float u = (float)(x - (k << ca.mesh_shift)) * ca.mesh_inv, v = (float)(y - (j << ca.mesh_shift)) * ca.mesh_inv;
        const float* r0 = D + (size_t)j * ca.mesh_gw * 2;
        const float* r1 = D + (size_t)j1 * ca.mesh_gw * 2;
        float d[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const float t0 = __builtin_fmaf(u, r0[k1 * 2 + c] - r0[k * 2 + c], r0[k * 2 + c]);
            const float t1 = __builtin_fmaf(u, r1[k1 * 2 + c] - r1[k * 2 + c], r1[k * 2 + c]);
            d[c] = __builtin_fmaf(v, t1 - t0, t0);
        }
        r.x = r.x + d[0]; r.y = r.y + d[1];
    }
    return r;
}

// The generic fold: any depth, 1 / 3 / 4 channels, every border mode, both subpixel modes. One thread owns one destination
// pixel and loops over the frame table. CLIP = false: the mean fold (running sums, acc (+)= sum of the samples);
// true: one sigma-clipping pass (ClipState, kernels_clip.hip) over the same samples.
// (The two modes are one __global__ template rather than a __device__ helper called from two kernels: pointers loaded
// from a kernel argument are promoted to the global address space before inlining, so a helper's taps and frame-table
// reads compiled to flat loads — a different, slower mean kernel.)
template <typename T, int CN, bool CLIP, class ClipState>
__global__ __launch_bounds__(256) void warp_accumulate_kernel(WarpArgs a, ClipArgs ca) {
    constexpr bool MESH = ClipState::displaced, MOMENTS = ClipState::stepped;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if constexpr (ClipState::in_band) y += ca.y0;     // store mode: a band of rows (a.dh = its end)
    // (moments mode: (x, y) index the stepped grid and every lane stays for the wave reduction; see the loop below)
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
    // moments mode: the thread walks ca.reps stepped rows, each time over entry 0 and entry 1 + blockIdx.z; every other
    // mode runs the body once. (fx, fy are set before the loop and only the moments mode overwrites them: computing them
    // inside the loop changed the register allocation of the other modes' instantiations. The body keeps its indentation.)
    int rep = 0;
    do {
    const int px = MOMENTS ? x * ca.step : x, py = MOMENTS ? (y * ca.reps + rep) * ca.step : y;
    if constexpr (MOMENTS) { cs.live = (px < a.dw) & (py < a.dh); fx = (float)px; fy = (float)py; }
    for (int f = 0; f < (MOMENTS ? 2 : a.n_frames); f++) {
        const WarpFrame* fr = a.frames + (MOMENTS ? f * (1 + (int)blockIdx.z) : f);
        const T* __restrict__ src = (const T*)fr->src;
#define STK_SUBPIX a.subpixel_bits
#define STK_SAMPLE(c, v) if constexpr (CLIP) cs.add(c, v); else sum[c] = sum[c] + v
        if constexpr (MESH) {
            // the entry's field moves the destination coordinate; these two shadow the pixel's own for the fragments below
            const MeshXY mxy = mesh_displace(ca, f, x, y);
            const float fx = mxy.x, fy = mxy.y;
#include "warp_coords.inc.h"
#include "warp_linear_sample.inc.h"
        } else {
#include "warp_coords.inc.h"
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

struct NoClip : FoldTraits {};   // the mean fold's (unused) clip state

// -----------------------------------------------------------------------------------------------
// Fast path for the production configuration: BGR u8 source, BORDER_CONSTANT, exact f32 coordinates.
// Same arithmetic as the generic kernel (bit-identical results). The kernel is bound by VALU issue, not by HBM (3 B
// of source per pixel and frame against ~60 instructions of coordinate, unpack and lerp arithmetic), so the work of
// round 2 went into the instruction count:
//   * X / W and Y / W share ONE v_rcp_f32 + Newton step and then run the exact fma chain the compiler's IEEE division
//     expands to (q = n r; e = n - d q; q += e r; e = n - d q; q += e r): the same bits as two `/` for a W in the normal
//     range — which the interior predicate requires — at 8 instructions (3 shared + 5 that pack into v_pk_*) instead of 22;
//   * whether the 4 taps of ALL frames of the group are inside the frame is voted per wave BEFORE the loads are issued:
//     interior waves (all but the frame's rim) load from the raw coordinates — no clamps, no end-of-buffer back-off, no
//     per-tap border selects; rim waves take the general path below with the same coordinates;
//   * the two horizontally adjacent taps of a row are 6 contiguous bytes -> ONE unaligned 8-byte load, bytes converted
//     with v_cvt_f32_ubyteN (extract + convert in one instruction);
//   * the frame loop is unrolled by WU: all 2*WU loads of a group are issued before the first is consumed;
//   * the accumulator (12 B/px) is read once (if accumulating) and written once per launch, whatever the frame count.
// Round 3, same bits again, ~70 -> ~50 VALU instructions per pixel and frame:
//   * the range test that licenses the shared reciprocal chain is made ONCE per frame on the host (warp_fold: W, X, Y are
//     affine in (x, y), so their extremes over the destination rectangle sit at its corners) and reaches the kernel as a
//     scalar flag; only frames that fail it take the per-pixel test;
//   * the twelve taps are converted straight out of the loaded dwords (v_cvt_f32_ubyte0..3, no shifts) into register
//     PAIRS — (B, G) of a tap, and R of the two rows — so that the x alpha multiplies (12 -> 6 v_pk_mul_f32), the
//     horizontal and vertical lerps (18 -> 10: v_pk_add_f32 with a negated operand + v_pk_fma_f32) and the running sums
//     (3 -> 2) are packed. Per component these are the generic kernel's operations in the generic kernel's order.
// -----------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t load_u64_unaligned(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

struct Tap12 { uint32_t a, b, c; };   // 12 bytes of a row: u8 kernel: an aligned window; u16 kernel: B0 G0 | R0 B1 | G1 R1

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }   // v_pk_fma_f32

// n / d for both components, correctly rounded for d and the quotients in the normal range: the compiler's own expansion
// of an IEEE f32 division without the v_div_scale / v_div_fixup range handling, the reciprocal chain shared by both
// quotients and the five dependent steps as packed instructions.
__device__ __forceinline__ f32x2 div2_shared(f32x2 n, float d) {
    float r = __builtin_amdgcn_rcpf(d);
    const float e0 = __builtin_fmaf(-d, r, 1.0f);
    r = __builtin_fmaf(e0, r, r);
    const f32x2 r2 = {r, r}, md = {-d, -d};
    f32x2 q = n * r2;
    f32x2 e = pk_fma(md, q, n);
    q = pk_fma(e, r2, q);
    e = pk_fma(md, q, n);
    return pk_fma(e, r2, q);
}

// The store mode's state: the sample of table entry i goes to band[((i * band_rows + y - y0) * dw + x) * CN + c]
// (ClipArgs), so a wave's stores for one frame are contiguous. The hooks run in frame order, so the entry index is a
// pointer that moves one frame slab per frame: after channel CN - 1 (add) or once per call (add2 / add3).
template <int CN>
struct FoldStore : FoldTraits {
    static constexpr bool in_band = true;
    float* p;
    size_t slab;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int x, int y) {
        p = ca.band + (size_t)(y - ca.y0) * ca.plane_stride + (size_t)x * CN;
        slab = (size_t)ca.band_rows * ca.plane_stride;
    }
    __device__ __forceinline__ void add(int c, float v) {
        p[c] = v;
        if (c == CN - 1) p += slab;
    }
    __device__ __forceinline__ void add2(f32x2 s01, float s2) { p[0] = s01.x; p[1] = s01.y; p[2] = s2; p += slab; }
    __device__ __forceinline__ void add3(float s0, float s1, float s2) { p[0] = s0; p[1] = s1; p[2] = s2; p += slab; }
    __device__ __forceinline__ void finish(const ClipArgs&, int, int) {}
};

// ---- where an entry's coefficients come from --------------------------------------------------------------------------
// Four combines exist twice: with the entry's gain and offset read from its record (ClipArgs::coef[i], indexed like the
// frame table), and with them interpolated from a node grid (local normalisation; definition: include/stacker.h, "Local
// normalisation"). Each is written once over a source (begin / weight / coef / next). The hooks run in frame
// order, so a source is a pointer, or two, that its state moves on after the entry's last sample.
//
// NormAt is a destination pixel's place on the node grid, computed once per pixel in begin(): the float offsets of its four
// nodes within a plane and the two fractions. The pixel's OWN y addresses the grid, also in the store mode, whose band
// pointer is the only thing that counts rows from ClipArgs::y0. at(P, q) is component q of plane P at the pixel: the mesh
// fold's chain (mesh_displace above), operation by operation.
struct NormAt {
    int o00, o01, o10, o11;
    float u, v;
    __device__ __forceinline__ void set(const ClipArgs& ca, int x, int y, int comps) {
        const int k = x >> ca.norm_shift, j = y >> ca.norm_shift;
        const int k1 = min(k + 1, ca.norm_gw - 1), j1 = min(j + 1, ca.norm_gh - 1);
        u = (float)(x - (k << ca.norm_shift)) * ca.norm_inv; v = (float)(y - (j << ca.norm_shift)) * ca.norm_inv;
        o00 = (j * ca.norm_gw + k) * comps; o01 = (j * ca.norm_gw + k1) * comps;
        o10 = (j1 * ca.norm_gw + k) * comps; o11 = (j1 * ca.norm_gw + k1) * comps;
    }
    __device__ __forceinline__ float at(const float* __restrict__ P, int q) const {
        const float t0 = __builtin_fmaf(u, P[o01 + q] - P[o00 + q], P[o00 + q]);
        const float t1 = __builtin_fmaf(u, P[o11 + q] - P[o10 + q], P[o10 + q]);
        return __builtin_fmaf(v, t1 - t0, t0);
    }
};

// How a source points into the record and plane tables: plainly, or (the store states, see StoreW) through the constant
// address space.
struct PlainTables {
    typedef const stk_frame_weight* Records;
    typedef const float* const* Planes;
};
struct ConstantTables {
    typedef const stk_frame_weight __attribute__((address_space(4))) * Records;
    typedef const float* const __attribute__((address_space(4))) * Planes;
};

// An entry's gain and offset for one channel, and for B, G, R at once (the u8 BGR fast kernels' states), as a source hands
// them over: F = float, or a reference into the entry's record.
template <class F> struct Coef { F g, o; };
template <class F> struct Coef3 { F g0, g1, g2, o0, o1, o2; };

// The record source: w, g, o of the entry from its record. coef hands out references, not values: the reads then happen
// where the state uses them, as when each state read its record itself. (A value is loaded in here, ahead of the state's
// own conditions; the store states' and the fast weighted clip's kernels then compile differently. DESIGN §4.27.)
// (The cast through an integer is what the constant address space needs; on plain pointers it folds away.)
template <class Tables>
struct FromRecord {
    typename Tables::Records e;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int, int) { e = (typename Tables::Records)(uintptr_t)ca.coef; }
    __device__ __forceinline__ float weight() const { return e->weight; }
    __device__ __forceinline__ auto coef(int c) const { return Coef<decltype((e->gain[c]))>{e->gain[c], e->offset[c]}; }
    __device__ __forceinline__ auto coef3() const {
        return Coef3<decltype((e->gain[0]))>{e->gain[0], e->gain[1], e->gain[2], e->offset[0], e->offset[1], e->offset[2]};
    }
    __device__ __forceinline__ void next() { e++; }
};

// The plane source: w from the record; (G, O) = the entry's plane (ClipArgs::norm[i]: per node CN gains, then CN offsets) at
// the pixel, or the record's gain and offset where the entry has no plane (fma(u, 0, g) = g: a constant plane and a
// record give the same bits). The plane pointer moves with the record pointer.
template <class Tables, int CN>
struct FromPlane : FromRecord<Tables> {
    typename Tables::Planes np;
    NormAt at;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int x, int y) {
        FromRecord<Tables>::begin(ca, x, y);
        np = (typename Tables::Planes)(uintptr_t)ca.norm;
        at.set(ca, x, y, 2 * CN);         // y, also in a store launch (not y - y0): the grid is the destination's
    }
    __device__ __forceinline__ Coef<float> coef(int c) const {
        const float* __restrict__ P = *np;
        const float G = P ? at.at(P, c) : this->e->gain[c], O = P ? at.at(P, CN + c) : this->e->offset[c];
        return {G, O};
    }
    __device__ __forceinline__ void next() { this->e++; np++; }
};

// The store mode with participation (the normalised, coverage-aware quantile; definition: include/stacker.h): FoldStore's
// layout, but the value written for entry i is the normalised sample u = s * g_i,c + o_i,c if the entry participates in
// the pixel (w_i > 0 and, with ClipArgs::coverage, kappa_i == 1.0f) and the bit pattern QUANTILE_ABSENT_BITS if not: a
// signalling NaN, which u, the result of an add, never is (common.h), so the selection kernel cannot take a genuine NaN
// for an absent entry. The values of a pixel are stored together, after the last channel's.
// Src reads the tables through constant-address-space pointers: the band's stores (through p) could alias a plain global
// pointer as far as the compiler knows, which turned every record read into a vector load behind the previous frame's
// stores and kept a pixel's three stores apart. The tables are written before the launch only.
template <int CN, class Src>
struct StoreW : FoldTraits {
    static constexpr bool wants_kappa = true, in_band = true;
    float* p;
    size_t slab;
    Src src;
    float v[CN];
    int cov;
    bool part;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int x, int y) {
        p = ca.band + (size_t)(y - ca.y0) * ca.plane_stride + (size_t)x * CN;
        slab = (size_t)ca.band_rows * ca.plane_stride;
        src.begin(ca, x, y); cov = ca.coverage; part = true;
    }
    __device__ __forceinline__ void entry(float k) { part = (src.weight() > 0.0f) & (cov ? k == 1.0f : true); }
    __device__ __forceinline__ float value(int c, float s) const {
        const auto k = src.coef(c);
        const float u = s * k.g + k.o;
        return part ? u : __uint_as_float(QUANTILE_ABSENT_BITS);
    }
    __device__ __forceinline__ void add(int c, float s) {
        v[c] = value(c, s);
        if (c == CN - 1) {
#pragma unroll
            for (int i = 0; i < CN; i++) p[i] = v[i];
            p += slab; src.next();
        }
    }
    __device__ __forceinline__ void finish(const ClipArgs&, int, int) {}
};

// from the records: every kernel
template <int CN>
struct FoldStoreW : StoreW<CN, FromRecord<ConstantTables>> {
    using StoreW<CN, FromRecord<ConstantTables>>::p;
    __device__ __forceinline__ void add2(f32x2 s01, float s2) { add3k(s01.x, s01.y, s2, 1.0f); }
    __device__ __forceinline__ void add3k(float s0, float s1, float s2, float k) {
        this->entry(k);
        const float v0 = this->value(0, s0), v1 = this->value(1, s1), v2 = this->value(2, s2);
        p[0] = v0; p[1] = v1; p[2] = v2;
        p += this->slab; this->src.next();
    }
};

// through the planes: generic kernels only (no add2 / add3k: a fast launch does not compile)
template <int CN> struct FoldStoreNorm : StoreW<CN, FromPlane<ConstantTables, CN>> {};

// The sums and the epilogue of the weighted means (WeightedMean, FoldLocal): num / den, 0 where nothing weighed in, and den
// to its plane.
template <int CN>
struct WeightedSums : FoldTraits {
    float num[CN], den;
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int c = 0; c < CN; c++) num[c] = 0.f;
        den = 0.f;
    }
    __device__ __forceinline__ void finish(const ClipArgs& ca, int x, int y) {
        float* o = ca.out + (size_t)y * ca.out_stride + (size_t)x * CN;
#pragma unroll
        for (int c = 0; c < CN; c++) o[c] = den > 0.f ? num[c] / den : 0.f;
        if (ca.den) ca.den[(size_t)y * ca.den_stride + x] = den;
    }
};

// The weighted mode's state (definition: include/stacker.h, stk_weight_params): per entry i of the frame table
//     v = s * g_i,c + o_i,c * kappa_i;  num_c = num_c + w_i * v;  den = den + w_i * kappa_i
// with g, o, w from Src. ClipArgs::coverage == 0: kappa = 1 by definition.
template <int CN, class Src>
struct WeightedMean : WeightedSums<CN> {
    static constexpr bool wants_kappa = true;
    using WeightedSums<CN>::num;
    using WeightedSums<CN>::den;
    float kap;
    Src src;
    int cov;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int x, int y) {
        this->zero(); kap = 1.0f;
        src.begin(ca, x, y); cov = ca.coverage;
    }
    __device__ __forceinline__ void entry(float k) { kap = cov ? k : 1.0f; }
    __device__ __forceinline__ void add(int c, float s) {
        const auto k = src.coef(c);
        const float v = s * k.g + k.o * kap;
        num[c] = num[c] + src.weight() * v;
        if (c == CN - 1) { den = den + src.weight() * kap; src.next(); }
    }
};

// from the records: every kernel. kappa = 1 makes o * kappa and w * kappa o and w bit for bit: add2 (the u8 fast kernels'
// interior path) multiplies neither, and packs (B, G).
template <int CN>
struct FoldWeighted : WeightedMean<CN, FromRecord<PlainTables>> {
    using WeightedSums<CN>::num;
    using WeightedSums<CN>::den;
    __device__ __forceinline__ void add2(f32x2 s01, float s2) {
        auto& e = this->src.e;
        const float w = e->weight;
        const f32x2 v01 = s01 * f32x2{e->gain[0], e->gain[1]} + f32x2{e->offset[0], e->offset[1]};
        const f32x2 n01 = f32x2{num[0], num[1]} + f32x2{w, w} * v01;
        num[0] = n01.x; num[1] = n01.y;
        num[2] = num[2] + w * (s2 * e->gain[2] + e->offset[2]);
        den = den + w;
        e++;
    }
    __device__ __forceinline__ void add3k(float s0, float s1, float s2, float k) {
        this->entry(k);
        this->add(0, s0); this->add(1, s1); this->add(2, s2);
    }
};

// through the planes (the locally normalised mean): generic kernels only (no add2 / add3k: a fast launch does not compile)
template <int CN> struct FoldNorm : WeightedMean<CN, FromPlane<PlainTables, CN>> {};

// The local mode's state (definition: include/stacker.h, stk_local_params): FoldWeighted with coverage = 1 and a weight per
// pixel. Per entry i of the frame table, in hook order entry(kappa), coords(..), add(0 .. CN - 1):
//     omega = the bilinear sample of plane maps[i] at the entry's coordinates (four clamped loads, 0 where a tap is
//             outside or the coordinate is not finite; the fold's lerp chain, or the classic four-weight sum; always
//             bilinear, also under the cubic fold, whose kernel hands over the same coordinates)
//     b = omega + floor * kappa;  u = b, (power - 1) times u = u * b;  W = w_i * u
//     v = s * g_i,c + o_i,c * kappa;  num_c = num_c + W * v;  den = den + W * kappa
// The table pointers (records, planes) move on after channel CN - 1. Generic kernels only.
template <int CN>
struct FoldLocal : WeightedSums<CN> {
    static constexpr bool wants_kappa = true, wants_coords = true;
    using WeightedSums<CN>::num;
    using WeightedSums<CN>::den;
    float kap, W;
    const stk_frame_weight* e;
    const float* const* mp;
    size_t ms;
    float floor;
    int power;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int, int) {
        this->zero(); kap = 1.0f; W = 0.f;
        e = ca.coef; mp = ca.maps; ms = ca.map_stride; floor = ca.floor; power = ca.power;
    }
    __device__ __forceinline__ void entry(float k) { kap = k; }
    __device__ __forceinline__ void coords(int ix, int iy, float ax, float ay, bool finite, bool classic, float w00, float w01,
                                           float w10, float w11, int sw, int sh) {
        const float* __restrict__ m = *mp;
        const bool ix0 = finite & ((unsigned)ix < (unsigned)sw), ix1 = finite & ((unsigned)(ix + 1) < (unsigned)sw);
        const bool iy0 = (unsigned)iy < (unsigned)sh, iy1 = (unsigned)(iy + 1) < (unsigned)sh;
        // clamped addresses keep every load in bounds; out-of-plane taps are replaced afterwards
        const int cx0 = min(max(ix, 0), sw - 1), cx1 = min(max(ix + 1, 0), sw - 1);
        const int cy0 = min(max(iy, 0), sh - 1), cy1 = min(max(iy + 1, 0), sh - 1);
        const float* r0 = m + (size_t)cy0 * ms;
        const float* r1 = m + (size_t)cy1 * ms;
        const float p00 = (ix0 & iy0) ? r0[cx0] : 0.0f, p01 = (ix1 & iy0) ? r0[cx1] : 0.0f;
        const float p10 = (ix0 & iy1) ? r1[cx0] : 0.0f, p11 = (ix1 & iy1) ? r1[cx1] : 0.0f;
        float om;
        if (classic) om = p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11;
        else {
            const float t0 = __builtin_fmaf(ax, p01 - p00, p00);
            const float t1 = __builtin_fmaf(ax, p11 - p10, p10);
            om = __builtin_fmaf(ay, t1 - t0, t0);
        }
        const float b = om + floor * kap;
        float u = b;
        for (int k = 1; k < power; k++) u = u * b;
        W = e->weight * u;
    }
    __device__ __forceinline__ void add(int c, float s) {
        const float v = s * e->gain[c] + e->offset[c] * kap;
        num[c] = num[c] + W * v;
        if (c == CN - 1) { den = den + W * kap; e++; mp++; }
    }
};

// The overlap moments of entry i against entry 0: private f64 sums n, and per channel sum X, sum Y, sum X^2, sum Y^2,
// sum XY with Y = entry 0's sample and X = entry i's over the pixels where `live` and kappa_i == 1.0f. X and Y are f32
// values, so each product is exact in f64 and only the order of the additions matters. The hooks see entry 0, then entry i.
// MASKED: whether there is a `live` to ask: FoldMoments' kernels set it per stepped row; every pixel CellMoments
// (kernels_local_norm.hip) sees counts.
template <int CN, bool MASKED>
struct MomentSums : FoldTraits {
    static constexpr bool wants_kappa = true;
    static constexpr int NM = 1 + 5 * CN;
    double S[NM];
    float Y[CN], kap;
    int which;
    bool live;
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int k = 0; k < NM; k++) S[k] = 0.0;
        which = 0; kap = 0.f; live = false;
    }
    __device__ __forceinline__ void entry(float k) { kap = k; }
    __device__ __forceinline__ void add(int c, float v) {
        if (which == 0) Y[c] = v;
        else {
            const bool in = MASKED ? live & (kap == 1.0f) : kap == 1.0f;
            const double X = in ? (double)v : 0.0, Yd = in ? (double)Y[c] : 0.0;    // masked terms add +0
            if (c == 0) S[0] = S[0] + (in ? 1.0 : 0.0);
            S[1 + 5 * c] = S[1 + 5 * c] + X;
            S[2 + 5 * c] = S[2 + 5 * c] + Yd;
            S[3 + 5 * c] = S[3 + 5 * c] + X * X;
            S[4 + 5 * c] = S[4 + 5 * c] + Yd * Yd;
            S[5 + 5 * c] = S[5 + 5 * c] + X * Yd;
        }
        if (c == CN - 1) which ^= 1;
    }
};

// The moments mode's state (generic kernels only): MomentSums over the stepped pixels, of which the kernel says per stepped
// row whether they are inside the destination (`live`). The order of the additions is fixed — the thread's rows in order,
// the xor-shuffle tree over the wave, then one partial per wave to ClipArgs::partials, which moments_reduce_kernel
// (kernels_weighted.hip) adds in index order. No atomics.
template <int CN>
struct FoldMoments : MomentSums<CN, true> {
    static constexpr bool stepped = true;
    using MomentSums<CN, true>::NM;
    using MomentSums<CN, true>::S;
    __device__ __forceinline__ void begin(const ClipArgs&, int, int) { this->zero(); }
    __device__ __forceinline__ void finish(const ClipArgs& ca, int, int) {
#pragma unroll
        for (int k = 0; k < NM; k++) {
            double v = S[k];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
            S[k] = v;
        }
        if ((threadIdx.x & 63) == 0) {
            const size_t part = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6);
            double* o = ca.partials + ((size_t)blockIdx.z * ((size_t)gridDim.x * gridDim.y * 4) + part) * NM;
#pragma unroll
            for (int k = 0; k < NM; k++) o[k] = S[k];
        }
    }
};

// WX: waves of a workgroup side by side along x (tile = 64 WX x 4 / WX pixels); WU: frames in flight per lane
// CLIP = false: the mean fold (running sums into a.acc); true: one sigma-clipping pass (ClipU8C3, kernels_clip.hip) — the
// same samples, only the per-sample body and the prologue / epilogue differ
template <bool AFFINE, int WX, int WU, bool CLIP, class ClipState>
__global__ __launch_bounds__(256) void warp_accumulate_u8c3_kernel(WarpArgs a, ClipArgs ca) {
    const int wave = threadIdx.x >> 6;
    const int x = (blockIdx.x * WX + (wave % WX)) * 64 + (threadIdx.x & 63);
    int y = blockIdx.y * (4 / WX) + wave / WX;
    if constexpr (ClipState::in_band) y += ca.y0;      // store mode: a band of rows (a.dh = its end)
    if (x >= a.dw || y >= a.dh) return;
    float* accp = a.acc + (size_t)y * a.acc_stride + (size_t)x * 3;
    f32x2 s01 = {0.f, 0.f};                   // (B, G) running sums as a register pair, R apart
    float s2 = 0.f;
    ClipState cs;
    if constexpr (CLIP) cs.begin(ca, x, y);
    else if (a.accumulate) { s01.x = accp[0]; s01.y = accp[1]; s2 = accp[2]; }
    const float fx = (float)x, fy = (float)y;
    const int sw = a.sw, sh = a.sh;
    const int stride32 = (int)a.src_stride;
    const float alpha = a.alpha, b0 = a.bv[0], b1 = a.bv[1], b2 = a.bv[2];

#define STK_CH(d, sft) ((float)(((d) >> (sft)) & 0xffu) * alpha)
#define STK_UB(d, k) ((float)(((d) >> (8 * (k))) & 0xffu))                           /* v_cvt_f32_ubyte<k> */
#define STK_LERP(p00, p01, p10, p11)                                                   \
    __builtin_fmaf(ay[u], __builtin_fmaf(ax[u], (p11) - (p10), (p10)) - __builtin_fmaf(ax[u], (p01) - (p00), (p00)), \
                   __builtin_fmaf(ax[u], (p01) - (p00), (p00)))
    for (int f0 = 0; f0 < a.n_frames; f0 += WU) {
        float ax[WU], ay[WU], Xs[WU], Ys[WU];
        int ix[WU], iy[WU];
        bool interior = true;
#pragma unroll
        for (int u = 0; u < WU; u++) {
            const WarpFrame* fr = a.frames + min(f0 + u, a.n_frames - 1);
            // (X, Y) as one packed pair: fma(M0, x, fma(M1, y, M2)) and fma(M3, x, fma(M4, y, M5)) — the generic kernel's operations
            bool fin = true;                              // false: X or Y is NaN / inf / absurdly large
            f32x2 XY = pk_fma(f32x2{fr->M[0], fr->M[3]}, f32x2{fx, fx}, pk_fma(f32x2{fr->M[1], fr->M[4]}, f32x2{fy, fy}, f32x2{fr->M[2], fr->M[5]}));
            if (!AFFINE) {
                const float W = __builtin_fmaf(fr->M[6], fx, __builtin_fmaf(fr->M[7], fy, fr->M[8]));
                // |W| in [2^-40, 2^40] (it is ~1 for any real homography) and |X|, |Y| < 2^40: the range in which the IEEE
                // expansion applies no scaling, so the shared chain returns the same bits
                if (fr->flags & WARPFRAME_DIV_IN_RANGE) XY = div2_shared(XY, W);     // decided per frame on the host (uniform branch)
                else {
                    const float aw = __builtin_fabsf(W);
                    // (compares, not max: a NaN operand must fail the test, v_max would drop it)
                    const bool safe = (aw < 1.0995116e12f) & (__builtin_fabsf(XY.x) < 1.0995116e12f) & (__builtin_fabsf(XY.y) < 1.0995116e12f) &
                                      (aw > 9.094947e-13f);
                    if (__all(safe)) XY = div2_shared(XY, W);   // finite operands in range: finite quotients
                    else {
                        XY.x = XY.x / W; XY.y = XY.y / W;
                        fin = (__builtin_fabsf(XY.x) < 1e9f) & (__builtin_fabsf(XY.y) < 1e9f);
                    }
                }
            } else {
                fin = (__builtin_fabsf(XY.x) < 1e9f) & (__builtin_fabsf(XY.y) < 1e9f);
            }
            const float X = XY.x, Y = XY.y;
            Xs[u] = X; Ys[u] = Y;
            const f32x2 fl = {__builtin_floorf(X), __builtin_floorf(Y)};
            ix[u] = (int)fl.x; iy[u] = (int)fl.y;         // saturating conversion; NaN -> 0, caught by the finite test
            const f32x2 fr2 = XY - fl;
            ax[u] = fr2.x; ay[u] = fr2.y;
            // all four taps inside the frame with a row to spare below (the 8-byte load of the last pixel pair of the last
            // row would run 2 bytes past the frame; rows sh-2 and sh-1 are left to the rim path). The int conversion saturates,
            // so huge coordinates fail the unsigned tests by themselves.
            interior &= fin & ((unsigned)ix[u] < (unsigned)(sw - 1)) & ((unsigned)iy[u] < (unsigned)(sh - 2));
        }
        if (__all(interior)) {
            uint64_t raw0[WU], raw1[WU];
#pragma unroll
            for (int u = 0; u < WU; u++) {
                const uint8_t* __restrict__ src = (const uint8_t*)a.frames[min(f0 + u, a.n_frames - 1)].src;
                // one frame is < 2 GiB (checked by the launcher): 32-bit offsets on the frame's uniform base pointer
                unsigned o = (unsigned)(__mul24(iy[u], stride32) + ix[u] * 3);      // rows < 2^24, row stride < 2^24 bytes
                const uint8_t* __restrict__ src1 = src + (unsigned)stride32;        // uniform: the second row's base stays in SGPRs
                if (a.frames[min(f0 + u, a.n_frames - 1)].flags & WARPFRAME_SRC_ALIGNED4) {
                    // The L1's address pipeline, not VALU issue, is what bounds this kernel (round 3: 20 % fewer VALU
                    // instructions changed nothing): an 8-byte gather at a 3-byte lane stride straddles dword boundaries in
                    // most lanes. A 12-byte window from the dword-aligned address below covers the 6 bytes wherever they
                    // start (offset 0..3), and v_alignbyte moves them into place: 1.23 -> 1.01 ms per 64 4K frames. The
                    // window ends at most 11 bytes behind `o`: inside the frame, the interior test keeps a row to spare.
                    const unsigned oa = o & ~3u, sh = o & 3u;
                    Tap12 t0, t1;
                    __builtin_memcpy(&t0, __builtin_assume_aligned(src + oa, 4), 12);
                    __builtin_memcpy(&t1, __builtin_assume_aligned(src1 + oa, 4), 12);
                    // (the flag also says that the row stride is a multiple of 4: both rows' windows are dword-aligned)
                    const uint32_t l0 = __builtin_amdgcn_alignbyte(t0.b, t0.a, sh), h0 = __builtin_amdgcn_alignbyte(t0.c, t0.b, sh);
                    const uint32_t l1 = __builtin_amdgcn_alignbyte(t1.b, t1.a, sh), h1 = __builtin_amdgcn_alignbyte(t1.c, t1.b, sh);
                    raw0[u] = (uint64_t)l0 | ((uint64_t)h0 << 32);
                    raw1[u] = (uint64_t)l1 | ((uint64_t)h1 << 32);
                } else {
                    raw0[u] = load_u64_unaligned(src + o);
                    raw1[u] = load_u64_unaligned(src1 + o);
                }
            }
#pragma unroll
            for (int u = 0; u < WU; u++) {
                if (f0 + u < a.n_frames) {
                    // a row's two taps are bytes B0 G0 R0 B1 | G1 R1 . . of the (lo, hi) dwords
                    const uint32_t l0 = (uint32_t)raw0[u], h0 = (uint32_t)(raw0[u] >> 32);
                    const uint32_t l1 = (uint32_t)raw1[u], h1 = (uint32_t)(raw1[u] >> 32);
                    const f32x2 al2 = {alpha, alpha}, ax2 = {ax[u], ax[u]}, ay2 = {ay[u], ay[u]};
                    const f32x2 bg00 = f32x2{STK_UB(l0, 0), STK_UB(l0, 1)} * al2, bg01 = f32x2{STK_UB(l0, 3), STK_UB(h0, 0)} * al2;
                    const f32x2 bg10 = f32x2{STK_UB(l1, 0), STK_UB(l1, 1)} * al2, bg11 = f32x2{STK_UB(l1, 3), STK_UB(h1, 0)} * al2;
                    const f32x2 rl = f32x2{STK_UB(l0, 2), STK_UB(l1, 2)} * al2;       // R of the left tap, rows (iy, iy + 1)
                    const f32x2 rr = f32x2{STK_UB(h0, 1), STK_UB(h1, 1)} * al2;       // R of the right tap
                    const f32x2 t0 = pk_fma(ax2, bg01 - bg00, bg00), t1 = pk_fma(ax2, bg11 - bg10, bg10);
                    const f32x2 tr = pk_fma(ax2, rr - rl, rl);                        // (row iy, row iy + 1)
                    if constexpr (CLIP) cs.add2(pk_fma(ay2, t1 - t0, t0), __builtin_fmaf(ay[u], tr.y - tr.x, tr.x));
                    else {
                        s01 = s01 + pk_fma(ay2, t1 - t0, t0);
                        s2 = s2 + __builtin_fmaf(ay[u], tr.y - tr.x, tr.x);
                    }
                }
            }
            continue;
        }
        // rim waves: clamped loads, per-tap border selects
#pragma unroll
        for (int u = 0; u < WU; u++) {
            if (f0 + u < a.n_frames) {
                const uint8_t* __restrict__ src = (const uint8_t*)a.frames[f0 + u].src;
                const bool finite = (__builtin_fabsf(Xs[u]) < 1e9f) & (__builtin_fabsf(Ys[u]) < 1e9f);   // false for NaN / inf
                const int jx = finite ? ix[u] : -100000, jy = finite ? iy[u] : -100000;
                if (!finite) { ax[u] = 0.0f; ay[u] = 0.0f; }
                const int xb = min(max(jx, 0), sw - 2);
                const int ox = jx - xb;            // 0 normal, -1 left tap outside, 1 right tap outside, else both outside
                const bool vy0 = (unsigned)jy < (unsigned)sh, vy1 = (unsigned)(jy + 1) < (unsigned)sh;
                const int yb0 = min(max(jy, 0), sh - 1), yb1 = min(max(jy + 1, 0), sh - 1);
                // an 8-byte load at the last pixel pair of the last row would run 2 bytes past the frame: back off, shift
                const int back0 = (yb0 == sh - 1 && xb == sw - 2) ? 2 : 0;
                const int back1 = (yb1 == sh - 1 && xb == sw - 2) ? 2 : 0;
                const uint64_t r0 = load_u64_unaligned(src + (unsigned)(yb0 * stride32 + xb * 3 - back0)) >> (back0 * 8);
                const uint64_t r1 = load_u64_unaligned(src + (unsigned)(yb1 * stride32 + xb * 3 - back1)) >> (back1 * 8);
                // left tap = bytes 0..2, right tap = bytes 3..5 of the pair starting at column xb
                const uint32_t a0 = (uint32_t)r0, a1 = (uint32_t)(r0 >> 24);
                const uint32_t c0 = (uint32_t)r1, c1 = (uint32_t)(r1 >> 24);
                // which dword serves tap x0 = ix and tap x1 = ix+1 (column offset from xb: ox, ox+1)
                const bool l_ok = (ox == 0) | (ox == 1), r_ok = (ox == 0) | (ox == -1);
                const uint32_t tl0 = ox == 0 ? a0 : a1, tr0 = ox == 0 ? a1 : a0;
                const uint32_t tl1 = ox == 0 ? c0 : c1, tr1 = ox == 0 ? c1 : c0;
                const bool v00 = l_ok & vy0, v01 = r_ok & vy0, v10 = l_ok & vy1, v11 = r_ok & vy1;
                float vb = 0.f, vg = 0.f, vr = 0.f;       // (clip mode: the three samples, handed over together)
                {
                    const float p00 = v00 ? STK_CH(tl0, 0) : b0, p01 = v01 ? STK_CH(tr0, 0) : b0;
                    const float p10 = v10 ? STK_CH(tl1, 0) : b0, p11 = v11 ? STK_CH(tr1, 0) : b0;
                    const float v = STK_LERP(p00, p01, p10, p11);
                    if constexpr (CLIP) vb = v; else s01.x = s01.x + v;
                }
                {
                    const float p00 = v00 ? STK_CH(tl0, 8) : b1, p01 = v01 ? STK_CH(tr0, 8) : b1;
                    const float p10 = v10 ? STK_CH(tl1, 8) : b1, p11 = v11 ? STK_CH(tr1, 8) : b1;
                    const float v = STK_LERP(p00, p01, p10, p11);
                    if constexpr (CLIP) vg = v; else s01.y = s01.y + v;
                }
                {
                    const float p00 = v00 ? STK_CH(tl0, 16) : b2, p01 = v01 ? STK_CH(tr0, 16) : b2;
                    const float p10 = v10 ? STK_CH(tl1, 16) : b2, p11 = v11 ? STK_CH(tr1, 16) : b2;
                    const float v = STK_LERP(p00, p01, p10, p11);
                    if constexpr (CLIP) vr = v; else s2 = s2 + v;
                }
                if constexpr (ClipState::wants_kappa)
                    cs.add3k(vb, vg, vr, STK_LERP(v00 ? 1.0f : 0.0f, v01 ? 1.0f : 0.0f, v10 ? 1.0f : 0.0f, v11 ? 1.0f : 0.0f));
                else if constexpr (CLIP) cs.add3(vb, vg, vr);
            }
        }
    }
#undef STK_CH
#undef STK_UB
#undef STK_LERP
    if constexpr (CLIP) cs.finish(ca, x, y);
    else { accp[0] = s01.x; accp[1] = s01.y; accp[2] = s2; }
}

// the launch conditions of the u8 BGR fast kernel (host side): 8-bit BGR, exact coordinates, BORDER_CONSTANT, a frame with
// a pixel pair per row and two rows (a one-row frame takes the generic kernel: the interior bound is (unsigned)(sh - 2)),
// 32-bit offsets within a frame
inline bool warp_u8c3_applies(const WarpArgs& a, int depth) {
    return depth == 8 && a.cn == 3 && a.subpixel_bits == 0 && a.border_mode == STK_BORDER_CONSTANT && a.sw >= 2 && a.sh >= 2 &&
           (size_t)a.sw * a.sh * 3 >= 16 && a.src_stride * (size_t)a.sh < ((size_t)1 << 31) && a.src_stride < (1u << 23) && a.sh < (1 << 23);
}

// the launch conditions of a fold through local-normalisation planes (host side): the tables are there and the grid is the
// destination's (a store launch's a.dh is its band's end; c.norm_gh is the whole destination's, hence the >=)
inline bool norm_args_ok(const WarpArgs& a, const ClipArgs& c) {
    if (a.n_frames <= 0 || !c.norm || !c.coef || c.norm_shift < 3 || c.norm_shift > 8) return false;
    const int step = 1 << c.norm_shift;
    return c.norm_gw == (a.dw - 1 + step - 1) / step + 1 && c.norm_gh >= (a.dh - 1 + step - 1) / step + 1;
}

// The one (depth, cn) ladder of every launcher (host side): launch(T{}, Channels<CN>{}) for the sample type T of `depth`
// (8, 16 or 32 bits) and cn = 1, 3 or 4 (BGRA: the alpha plane is warped and summed like a colour — the reference converts,
// warps and adds whatever imread returned). Returns the launch's error; a missing kernel is an error: any other
// (depth, cn) is hipErrorInvalidValue. `launch` is a generic lambda:
//     [&](auto t, auto ch) { kernel<decltype(t), decltype(ch)::value, ...><<<grid, 256, 0, s>>>(...); }
template <int CN> using Channels = std::integral_constant<int, CN>;
template <class Launch>
hipError_t dispatch_depth_cn(int depth, int cn, Launch&& launch) {
    if (depth == 8 && cn == 3) launch(uint8_t{}, Channels<3>{});
    else if (depth == 8 && cn == 1) launch(uint8_t{}, Channels<1>{});
    else if (depth == 8 && cn == 4) launch(uint8_t{}, Channels<4>{});
    else if (depth == 16 && cn == 3) launch(uint16_t{}, Channels<3>{});
    else if (depth == 16 && cn == 1) launch(uint16_t{}, Channels<1>{});
    else if (depth == 16 && cn == 4) launch(uint16_t{}, Channels<4>{});
    else if (depth == 32 && cn == 3) launch(float{}, Channels<3>{});
    else if (depth == 32 && cn == 1) launch(float{}, Channels<1>{});
    else if (depth == 32 && cn == 4) launch(float{}, Channels<4>{});
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace stk
