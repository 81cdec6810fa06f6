// kernels_clip.hip — kappa-sigma clipping over the aligned frames (stk_clip_stack and the *_clipped entry points).
// One pass is one more fold of the same frames: the fold kernels with a clip state (the table of states is at the top of
// warp_body.h; this file ends with that table as static_asserts), the sample of every frame computed by the very
// instructions the mean fold adds. Per pixel and channel a pass keeps the moments of the
// samples inside [L, U] about the previous centre c (k, a = sum d, b = sum d^2 with d = s - c), and its epilogue turns them
// into the next (c, L, U) — or, on the last pass, into the clipped mean and the count of kept samples. Definition (bit for
// bit, f32, no contraction: the Makefile's -ffp-contract=off; `/` and sqrt are the correctly rounded forms):
//     pass:      d = s - c; if (L <= s && s <= U) { k += 1; a = a + d; b = b + d*d; }
//     update:    if (k >= 3) { ma = a / k; m = c + ma; v = b / k - ma*ma; sigma = sqrt(max(v, 0));
//                              L = max(L, m - kappa_low sigma); U = min(U, m + kappa_high sigma); c = m; }
//     last pass: out = k > 0 ? c + a / k : c; counts = k
// The shifted moments keep the variance accurate (the samples sit close to c). Cost over the mean fold's per-sample work:
// a subtract, a multiply, two adds, two compares and the selects — the c / L / U planes are read once and written once per
// pass, like the accumulator.
#include "fold_launch.h"

namespace stk {

__device__ __forceinline__ bool clip_in(float s, float L, float U) { return (L <= s) & (s <= U); }

// epilogue of one channel: plane index p, output index o
__device__ __forceinline__ void clip_end(const ClipArgs& ca, size_t p, size_t o, float c, float L, float U, int k, float a, float b) {
    if (ca.last) {
        ca.out[o] = k > 0 ? c + a / (float)k : c;
        if (ca.counts) ca.counts[p] = k;
        return;
    }
    if (k >= 3) {
        const float kf = (float)k;
        const float ma = a / kf;
        const float m = c + ma;
        const float v = b / kf - ma * ma;
        const float sigma = __builtin_sqrtf(__builtin_fmaxf(v, 0.0f));
        L = __builtin_fmaxf(L, m - ca.kappa_low * sigma);
        U = __builtin_fminf(U, m + ca.kappa_high * sigma);
        c = m;
    }
    ca.c[p] = c; ca.L[p] = L; ca.U[p] = U;
}

// The prologue of every pass, for the generic kernels' states (CN channels, indexed by the unrolled channel loop): c / L / U
// of the pixel from their planes. A first pass opens the interval; so does the weighted clip's centre pass, which also
// starts from c = 0 (`centre` = ClipArgs::centre there, 0 in the plain clip, which has no such pass). Returns the plane index.
template <int CN>
__device__ __forceinline__ size_t clip_load(const ClipArgs& ca, int x, int y, int centre, float* c, float* L, float* U) {
    const size_t p = (size_t)y * ca.plane_stride + (size_t)x * CN;
    const bool open = ca.first | centre;
#pragma unroll
    for (int i = 0; i < CN; i++) {
        c[i] = centre ? 0.0f : ca.c[p + i];
        L[i] = open ? -__builtin_inff() : ca.L[p + i];
        U[i] = open ? __builtin_inff() : ca.U[p + i];
    }
    return p;
}

// the same for the u8 BGR fast kernels' states: (B, G) as register pairs, R apart
__device__ __forceinline__ size_t clip_load_u8c3(const ClipArgs& ca, int x, int y, int centre, f32x2& c01, f32x2& L01, f32x2& U01,
                                                 float& c2, float& L2, float& U2) {
    const size_t p = (size_t)y * ca.plane_stride + (size_t)x * 3;
    if (centre) { c01 = f32x2{0.f, 0.f}; c2 = 0.f; }
    else { c01 = f32x2{ca.c[p], ca.c[p + 1]}; c2 = ca.c[p + 2]; }
    if (ca.first | centre) {
        L01 = f32x2{-__builtin_inff(), -__builtin_inff()}; L2 = -__builtin_inff();
        U01 = f32x2{__builtin_inff(), __builtin_inff()}; U2 = __builtin_inff();
    } else {
        L01 = f32x2{ca.L[p], ca.L[p + 1]}; L2 = ca.L[p + 2];
        U01 = f32x2{ca.U[p], ca.U[p + 1]}; U2 = ca.U[p + 2];
    }
    return p;
}

// generic kernel's state
template <int CN>
struct ClipGeneric : FoldTraits {
    float c[CN], L[CN], U[CN], a[CN], b[CN];
    int k[CN];
    size_t p;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int x, int y) {
        p = clip_load<CN>(ca, x, y, 0, c, L, U);
#pragma unroll
        for (int i = 0; i < CN; i++) { a[i] = 0.f; b[i] = 0.f; k[i] = 0; }
    }
    __device__ __forceinline__ void add(int i, float s) {
        const float d = s - c[i];
        const bool in = clip_in(s, L[i], U[i]);
        k[i] += in ? 1 : 0;
        a[i] = in ? a[i] + d : a[i];
        b[i] = in ? b[i] + d * d : b[i];
    }
    __device__ __forceinline__ void finish(const ClipArgs& ca, int x, int y) {
        const size_t o = (size_t)y * ca.out_stride + (size_t)x * CN;
#pragma unroll
        for (int i = 0; i < CN; i++) clip_end(ca, p + i, o + i, c[i], L[i], U[i], k[i], a[i], b[i]);
    }
};

// u8 BGR fast kernel's state: v_pk_add / v_pk_mul for the moments of (B, G)
struct ClipU8C3 : FoldTraits {
    f32x2 c01, L01, U01, a01, b01;
    float c2, L2, U2, a2, b2;
    int k0, k1, k2;
    size_t p;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int x, int y) {
        p = clip_load_u8c3(ca, x, y, 0, c01, L01, U01, c2, L2, U2);
        a01 = f32x2{0.f, 0.f}; b01 = f32x2{0.f, 0.f}; a2 = 0.f; b2 = 0.f;
        k0 = k1 = k2 = 0;
    }
    __device__ __forceinline__ void add2(f32x2 s01, float s2) {
        const f32x2 d = s01 - c01;
        const f32x2 an = a01 + d, bn = b01 + d * d;
        const bool i0 = clip_in(s01.x, L01.x, U01.x), i1 = clip_in(s01.y, L01.y, U01.y);
        k0 += i0 ? 1 : 0; k1 += i1 ? 1 : 0;
        a01.x = i0 ? an.x : a01.x; a01.y = i1 ? an.y : a01.y;
        b01.x = i0 ? bn.x : b01.x; b01.y = i1 ? bn.y : b01.y;
        const float d2 = s2 - c2;
        const bool i2 = clip_in(s2, L2, U2);
        k2 += i2 ? 1 : 0;
        a2 = i2 ? a2 + d2 : a2;
        b2 = i2 ? b2 + d2 * d2 : b2;
    }
    __device__ __forceinline__ void add3(float s0, float s1, float s2) { add2(f32x2{s0, s1}, s2); }
    __device__ __forceinline__ void finish(const ClipArgs& ca, int x, int y) {
        const size_t o = (size_t)y * ca.out_stride + (size_t)x * 3;
        clip_end(ca, p, o, c01.x, L01.x, U01.x, k0, a01.x, b01.x);
        clip_end(ca, p + 1, o + 1, c01.y, L01.y, U01.y, k1, a01.y, b01.y);
        clip_end(ca, p + 2, o + 2, c2, L2, U2, k2, a2, b2);
    }
};

hipError_t launch_clip_pass(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (a.n_frames <= 0) return hipErrorInvalidValue;
    return launch_fold<ClipU8C3, ClipGeneric>(a, c, depth, a.dh, s);
}

// ---- the weighted clip: normalised, coverage-aware rejection (stk_clip_stack_weighted and the *_clipped_weighted entry
// points; definition in include/stacker.h) ---------------------------------------------------------------------------
// The same fold kernels, a new state. Per sample over the body above: u = s * g + o (one multiply, one add), the
// participation flag (w > 0, and with coverage kappa == 1.0f; one per pixel and entry) folded into clip_in, the running
// kept weight sw and two multiplies by w:
//     pass:      d = u - c; if (participates && L <= u && u <= U) { k += 1; sw = sw + w; a = a + w*d; b = b + w*(d*d); }
//     update:    as above with sw for k in the divisions (k >= 3 still decides whether there is an update)
//     last pass: out = k > 0 ? c + a / sw : c; counts = k; kept = sw
// The centre pass (ClipArgs::centre) is a mode of the same state: c = 0 makes d = u, the interval test is skipped, and the
// epilogue writes c = sw > 0 ? a / sw : 0 — the weighted mean of the participating samples — to the c plane.
__device__ __forceinline__ void clip_end_w(const ClipArgs& ca, size_t p, size_t o, float c, float L, float U, int k, float sw, float a, float b) {
    if (ca.centre) {
        ca.c[p] = sw > 0.0f ? a / sw : 0.0f;
        return;
    }
    if (ca.last) {
        ca.out[o] = k > 0 ? c + a / sw : c;
        if (ca.counts) ca.counts[p] = k;
        if (ca.kept) ca.kept[p] = sw;
        return;
    }
    if (k >= 3) {
        const float ma = a / sw;
        const float m = c + ma;
        const float v = b / sw - ma * ma;
        const float sigma = __builtin_sqrtf(__builtin_fmaxf(v, 0.0f));
        L = __builtin_fmaxf(L, m - ca.kappa_low * sigma);
        U = __builtin_fminf(U, m + ca.kappa_high * sigma);
        c = m;
    }
    ca.c[p] = c; ca.L[p] = L; ca.U[p] = U;
}

// Written once over the coefficient source Src (warp_body.h): the records, or the local-normalisation planes below.
template <int CN, class Src>
struct ClipW : FoldTraits {
    static constexpr bool wants_kappa = true;
    float c[CN], L[CN], U[CN], a[CN], b[CN], sw[CN];
    int k[CN];
    size_t p;
    Src src;
    int cov;
    bool part, centre;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int x, int y) {
        p = clip_load<CN>(ca, x, y, ca.centre, c, L, U);
#pragma unroll
        for (int i = 0; i < CN; i++) { a[i] = 0.f; b[i] = 0.f; sw[i] = 0.f; k[i] = 0; }
        cov = ca.coverage; centre = ca.centre != 0; part = true; src.begin(ca, x, y);
    }
    __device__ __forceinline__ void entry(float kap) { part = (src.weight() > 0.0f) & (cov ? kap == 1.0f : true); }
    __device__ __forceinline__ void add(int i, float s) {
        const float w = src.weight();
        const auto g = src.coef(i);
        const float u = s * g.g + g.o;
        const float d = u - c[i];
        const bool in = part & (centre | clip_in(u, L[i], U[i]));
        // a sample that is out adds w = 0 times d = 0: +0 to each sum, whatever u is (two selects instead of three)
        const float wi = in ? w : 0.0f, di = in ? d : 0.0f;
        k[i] += in ? 1 : 0;
        sw[i] = sw[i] + wi;
        a[i] = a[i] + wi * di;
        b[i] = b[i] + wi * (di * di);
        if (i == CN - 1) src.next();
    }
    __device__ __forceinline__ void finish(const ClipArgs& ca, int x, int y) {
        const size_t o = (size_t)y * ca.out_stride + (size_t)x * CN;
#pragma unroll
        for (int i = 0; i < CN; i++) clip_end_w(ca, p + i, o + i, c[i], L[i], U[i], k[i], sw[i], a[i], b[i]);
    }
};

// u8 BGR fast kernels' state: (B, G) as register pairs, R apart. add2 is the interior path (kappa = 1: the entry
// participates iff w > 0), add3k the rim path with its kappa. Src hands over the entry's six coefficients at once (coef3).
template <class Src>
struct ClipWFast : FoldTraits {
    static constexpr bool wants_kappa = true;
    f32x2 c01, L01, U01, a01, b01, sw01;
    float c2, L2, U2, a2, b2, sw2;
    int k0, k1, k2;
    size_t p;
    Src src;
    int cov;
    bool centre;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int x, int y) {
        p = clip_load_u8c3(ca, x, y, ca.centre, c01, L01, U01, c2, L2, U2);
        a01 = f32x2{0.f, 0.f}; b01 = f32x2{0.f, 0.f}; sw01 = f32x2{0.f, 0.f}; a2 = 0.f; b2 = 0.f; sw2 = 0.f;
        k0 = k1 = k2 = 0;
        cov = ca.coverage; centre = ca.centre != 0; src.begin(ca, x, y);
    }
    __device__ __forceinline__ void fold(f32x2 s01, float s2, bool part) {
        const float w = src.weight();
        const auto q = src.coef3();
        const f32x2 u01 = s01 * f32x2{q.g0, q.g1} + f32x2{q.o0, q.o1};
        const f32x2 d = u01 - c01;
        const bool i0 = part & (centre | clip_in(u01.x, L01.x, U01.x)), i1 = part & (centre | clip_in(u01.y, L01.y, U01.y));
        // a sample that is out adds w = 0 times d = 0: +0 to each sum, whatever u is (two selects per channel instead of
        // three, and the sums stay packed)
        const f32x2 wi = {i0 ? w : 0.0f, i1 ? w : 0.0f}, di = {i0 ? d.x : 0.0f, i1 ? d.y : 0.0f};
        k0 += i0 ? 1 : 0; k1 += i1 ? 1 : 0;
        sw01 = sw01 + wi;
        a01 = a01 + wi * di;
        b01 = b01 + wi * (di * di);
        const float u2 = s2 * q.g2 + q.o2;
        const float d2 = u2 - c2;
        const bool i2 = part & (centre | clip_in(u2, L2, U2));
        const float w2 = i2 ? w : 0.0f, dd2 = i2 ? d2 : 0.0f;
        k2 += i2 ? 1 : 0;
        sw2 = sw2 + w2;
        a2 = a2 + w2 * dd2;
        b2 = b2 + w2 * (dd2 * dd2);
        src.next();
    }
    __device__ __forceinline__ void add2(f32x2 s01, float s2) { fold(s01, s2, src.weight() > 0.0f); }
    __device__ __forceinline__ void add3k(float s0, float s1, float s2, float kap) {
        fold(f32x2{s0, s1}, s2, (src.weight() > 0.0f) & (cov ? kap == 1.0f : true));
    }
    __device__ __forceinline__ void finish(const ClipArgs& ca, int x, int y) {
        const size_t o = (size_t)y * ca.out_stride + (size_t)x * 3;
        clip_end_w(ca, p, o, c01.x, L01.x, U01.x, k0, sw01.x, a01.x, b01.x);
        clip_end_w(ca, p + 1, o + 1, c01.y, L01.y, U01.y, k1, sw01.y, a01.y, b01.y);
        clip_end_w(ca, p + 2, o + 2, c2, L2, U2, k2, sw2, a2, b2);
    }
};

template <int CN> struct ClipWGeneric : ClipW<CN, FromRecord<PlainTables>> {};
struct ClipWU8C3 : ClipWFast<FromRecord<PlainTables>> {};

hipError_t launch_clip_pass_weighted(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (a.n_frames <= 0 || !c.coef) return hipErrorInvalidValue;
    return launch_fold<ClipWU8C3, ClipWGeneric>(a, c, depth, a.dh, s);
}

// ---- the weighted clip through local-normalisation planes (stk_clip_stack_local_norm, stk_robust_clip_stack_local_norm
// and the *_local_normalized_clipped entry points; definition in include/stacker.h, "Locally normalised clip") ------------
// The weighted clip's states over the plane source: u = s * G + O, (G, O) the entry's plane at the destination pixel, or
// the record's gain and offset where the entry has no plane (FromPlane, warp_body.h, as FoldNorm reads it).
template <int CN> struct ClipNorm : ClipW<CN, FromPlane<PlainTables, CN>> {};

// The plane source of the u8 BGR fast kernels: six chains (three gains, three offsets) per entry. The first fast-kernel
// state that reads the node grid. A wave of the fast kernels is a run of consecutive x in one row, so from a node spacing
// of 64 on its lanes usually share their four nodes: begin() takes a wave vote on the four node offsets (all lanes' equal
// the first lane's; nothing is assumed about the launch shape), and where it holds the plane values are read through the
// first lane's offsets and a constant-address-space pointer, which makes them scalar loads into scalar registers (the
// planes are written before the launch only). Where it does not hold (spacing 8 .. 32, or a wave across a node column)
// every lane loads its own. The arithmetic is NormAt::at's, operation for operation (sub, fma, sub, fma, sub, fma), so the
// two paths and ClipNorm<3> give the same bits.
struct VotedPlane : FromPlane<PlainTables, 3> {
    typedef const float __attribute__((address_space(4))) * UniformPlane;
    int s00, s01, s10, s11;          // the first lane's node offsets (wave-uniform)
    bool uniform;
    __device__ __forceinline__ void begin(const ClipArgs& ca, int x, int y) {
        FromPlane<PlainTables, 3>::begin(ca, x, y);
        s00 = __builtin_amdgcn_readfirstlane(at.o00); s01 = __builtin_amdgcn_readfirstlane(at.o01);
        s10 = __builtin_amdgcn_readfirstlane(at.o10); s11 = __builtin_amdgcn_readfirstlane(at.o11);
        uniform = __all((at.o00 == s00) & (at.o01 == s01) & (at.o10 == s10) & (at.o11 == s11)) != 0;
#ifdef STK_NORM_CLIP_NO_VOTE                                  // measurement only (tools/local_norm_clip_time.py): always per-lane loads
        uniform = false;
#endif
    }
    // NormAt::at on four node values
    __device__ __forceinline__ float chain(float p00, float p01, float p10, float p11) const {
        const float t0 = __builtin_fmaf(at.u, p01 - p00, p00);
        const float t1 = __builtin_fmaf(at.u, p11 - p10, p10);
        return __builtin_fmaf(at.v, t1 - t0, t0);
    }
    __device__ __forceinline__ Coef3<float> coef3() const {
        const float* __restrict__ P = *np;
        float q[6];                      // G of B, G, R, then O of B, G, R
        if (!P) {
#pragma unroll
            for (int i = 0; i < 3; i++) { q[i] = e->gain[i]; q[3 + i] = e->offset[i]; }
        } else if (uniform) {
            const UniformPlane S = (UniformPlane)(uintptr_t)P;
#pragma unroll
            for (int i = 0; i < 6; i++) q[i] = chain(S[s00 + i], S[s01 + i], S[s10 + i], S[s11 + i]);
        } else {
#pragma unroll
            for (int i = 0; i < 6; i++) q[i] = at.at(P, i);
        }
        return {q[0], q[1], q[2], q[3], q[4], q[5]};
    }
};

struct ClipNormU8C3 : ClipWFast<VotedPlane> {};

hipError_t launch_clip_pass_norm(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (!norm_args_ok(a, c)) return hipErrorInvalidValue;
    return launch_fold<ClipNormU8C3, ClipNorm>(a, c, depth, a.dh, s);
}

// ---- what every state asks of its kernel, pinned: one line per (state, trait) that holds, so that a change to a state's
// traits is a change here too. (This unit sees every state: fold_launch.h includes both fold headers.) ------------------
#define STK_ASKS(State, trait) static_assert(State::trait, #State " asks for " #trait)
#define STK_ASKS_NOT(State, trait) static_assert(!State::trait, #State " does not ask for " #trait)
STK_ASKS(FoldWeighted<3>, wants_kappa);   STK_ASKS(FoldNorm<3>, wants_kappa);       STK_ASKS(FoldMoments<3>, wants_kappa);
STK_ASKS(FoldStoreW<3>, wants_kappa);     STK_ASKS(FoldStoreNorm<3>, wants_kappa);  STK_ASKS(FoldLocal<3>, wants_kappa);
STK_ASKS(ClipWGeneric<3>, wants_kappa);   STK_ASKS(ClipNorm<3>, wants_kappa);       STK_ASKS(Mesh<FoldLocal<3>>, wants_kappa);
STK_ASKS(ClipWU8C3, wants_kappa);         STK_ASKS(ClipNormU8C3, wants_kappa);
STK_ASKS(FoldLocal<3>, wants_coords);     STK_ASKS(Mesh<FoldLocal<3>>, wants_coords);
STK_ASKS(FoldStore<3>, in_band);          STK_ASKS(FoldStoreW<3>, in_band);         STK_ASKS(FoldStoreNorm<3>, in_band);
STK_ASKS(FoldMoments<3>, stepped);
STK_ASKS(Mesh<NoClip>, displaced);        STK_ASKS(Mesh<FoldLocal<3>>, displaced);
STK_ASKS_NOT(NoClip, wants_kappa);        STK_ASKS_NOT(ClipGeneric<3>, wants_kappa); STK_ASKS_NOT(ClipU8C3, wants_kappa);
STK_ASKS_NOT(FoldStore<3>, wants_kappa);  STK_ASKS_NOT(FoldLocal<3>, displaced);     STK_ASKS_NOT(FoldWeighted<3>, in_band);
STK_ASKS_NOT(FoldNorm<3>, in_band);       STK_ASKS_NOT(FoldWeighted<3>, stepped);
#undef STK_ASKS
#undef STK_ASKS_NOT

}  // namespace stk
