// common.h — shared declarations of the HIP engine (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/stacker.h"

namespace stk {

// ---------------------------------------------------------------------------------------------
// Device data layout (all in HBM, owned by the context's workspace)
//
//  * frames          interleaved BGR u8/u16/f32 as handed in (OpenCV Mat layout).
//  * reference planes (ECC "input" = frame 0, shared by every frame of the stack):
//        f32 planes  I (blurred grey), gx, gy, an interleaved (gx, gy) copy and an interleaved (I, gx, gy) copy, each (H + 2 REF_PAD) x ref_stride
//        with a REF_PAD-pixel ZERO border on every side, so a bilinear footprint with BORDER_CONSTANT 0 is
//        unconditional loads after clamping the integer coordinate to [-2, W] x [-2, H].
//  * templates       one blurred-grey f32 plane per moving frame, row stride rounded up to a
//        multiple of 4 floats so each lane streams aligned 16-byte quads.
//  * accumulator     f32 W*H*3 running sum (the Rayon fold accumulator, lib.rs:306-316, 807-814).
// ---------------------------------------------------------------------------------------------

// Zero border of the frame-0 planes, on every side. >= 2 makes a bilinear footprint unconditional after
// clamping to [-2, W] x [-2, H]; 24 (a multiple of 4: rows stay 16-byte aligned) additionally lets the
// tiled ECC kernel copy whole 72 x 22 footprints of border tiles with unclamped 16-byte LDS-DMA pieces.
constexpr int REF_PAD = 24;

struct RefPlanes {
    const float* I;   // pointer to pixel (0,0) inside the padded plane
    const float* gx;
    const float* gy;
    const float* gxy; // (gx, gy) interleaved, same padded geometry (2 floats per pixel)
    const float* igg; // (I, gx, gy) interleaved, same padded geometry (3 floats per pixel): what the LDS ring of the column pass streams
    int stride;       // floats per padded row
    int w, h;
};

// One ECC "slot": a frame currently being iterated. Lives in device memory and is advanced
// entirely on the device (solve kernel); the host only polls EccQueue::frames_done.
struct EccSlot {
    int   frame;        // index into the template array, -1 = idle
    int   iter;         // iterations executed so far
    float warp[9];      // current map, row-major 3x3
    float cI, cT;       // centring offsets (previous iteration's f32 means) for the moment sums
    double rho, last_rho;
};

struct EccFrameResult {
    float  warp[9];
    int    iters;
    int    status;      // 0 ok, 1 NaN, 2 lambda_d <= 0, 3 not run
    double rho;
};

struct EccQueue {
    int next_frame;     // next template index to hand to a free slot
    int n_frames;       // number of templates
    int frames_done;
    int ready;          // templates [0, ready) exist; raised by the prep stream while frames are still arriving over PCIe
    int ring_fallbacks; // strips of the iteration pass that left the LDS ring for the gather loop at run time (stk_timing.ecc_ring_fallbacks)
    int first_iter_slots; // slot-iterations of the column pass that took the first-iteration route (stk_get_counter "ecc_first_iter_slots")
#ifdef STK_SOLVE_TIMING
    long long dbg[16];   // wall_clock64 phase deltas of the last solve of slot 0 (10 ns ticks), debug builds only
#endif
};

struct EccCriteria {
    int    n_iter;      // COUNT ? max_count : 200
    double eps;         // EPS ? epsilon : -1
};

// number of moment sums produced per slot and iteration for P warp parameters
__host__ __device__ constexpr int ecc_nsums(int P) { return P * (P + 1) / 2 + 3 * P + 6; }
constexpr int ECC_MAX_SUMS = ecc_nsums(8);   // 66

struct EccIterArgs {
    RefPlanes ref;
    const float* templates;      // n_frames planes
    size_t templ_plane_stride;   // floats between consecutive templates
    int templ_row_stride;        // floats per template row (multiple of 4)
    int tw, th;
    EccSlot* slots;
    int n_slots;                 // slots iterated by this launch: slot0 .. slot0 + n_slots - 1
    int nb;                      // blocks per slot (multiple of 8)
    double* partials;            // [all slots][nsums][nb]
    double* sums;                // [all slots][ECC_MAX_SUMS]: the reduced sums, stage 1 -> stage 2 of the solve kernel
    int* tickets;                // [all slots]: arrival counter of the solve kernel's stage-1 workgroups (self-resetting)
    int slot0;                   // first slot of this launch (0: all slots in one launch)
    int ring;                    // column-walking pass: 1 = frame-0 rows through the per-wave LDS ring where a strip allows it (option ecc_ring)
    int ring_lookahead;          // frame-0 rows the ring keeps ahead of the row being fetched: 5; lower only to provoke the fallback (option ecc_ring_lookahead)
    int* ring_fallbacks;         // device counter: strips whose ring bounds failed the run-time check and were redone by the gather loop (EccQueue::ring_fallbacks)
    int units_q, units_r;        // column-walking pass: (column strip, row) units per wave and the remainder (set by launch_ecc_iter)
    // column-walking homography pass, first iteration of a frame that starts at the identity (option ecc_first_iter): the
    // block partials [ECC_MAX_SUMS][nb] of that iteration as the pass itself computed them once for this call; the sums
    // that do not read the template are copied from here. Null: every iteration takes the general route
    const double* first_sums;
    int* first_iter_slots;       // device counter: slot-iterations that took that route (EccQueue::first_iter_slots)
};

struct WarpFrame {
    const void* src;
    float  M[9];                 // destination -> source map, f32 (subpixel_bits == 0)
    int    flags;                // WARPFRAME_*: set by warp_fold for the destination rectangle of the launch
    double Md[9];                // same in double (classic quantised path)
};
// over the whole destination rectangle |W| lies in [2^-36, 2^36] and |X|, |Y| (before the division) below 2^36: the range
// in which an IEEE f32 division applies no scaling, so X / W and Y / W may share one reciprocal chain (kernels_warp.hip)
constexpr int WARPFRAME_DIV_IN_RANGE = 1;
// the frame's base address and its row stride are multiples of 4: the u8 fast path may gather dword-aligned 12-byte windows
constexpr int WARPFRAME_SRC_ALIGNED4 = 2;

// 3x3 inverse by the adjugate in double (cv::invert on a 3x3 CV_64F) and invertAffineTransform: what warpPerspective /
// warpAffine do to the forward matrix before they map destination pixels (lib.rs:290-299, 780-803). Host and device run
// the same operations (no contraction: -ffp-contract=off), so a warp frame built on either side has the same bits.
__host__ __device__ inline void warp_invert3x3(const double* m, double* o) {
    double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (d == 0.0) { for (int i = 0; i < 9; i++) o[i] = 0; return; }
    d = 1.0 / d;
    double t[9] = {(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
                   (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
                   (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d};
    for (int i = 0; i < 9; i++) o[i] = t[i];
}
__host__ __device__ inline void warp_invert_affine(const double* m, double* o) {
    double D = m[0] * m[4] - m[1] * m[3];
    D = D != 0 ? 1.0 / D : 0;
    const double A11 = m[4] * D, A22 = m[0] * D, A12 = -m[1] * D, A21 = -m[3] * D;
    o[0] = A11; o[1] = A12; o[2] = -A11 * m[2] - A12 * m[5];
    o[3] = A21; o[4] = A22; o[5] = -A21 * m[2] - A22 * m[5];
    o[6] = 0; o[7] = 0; o[8] = 1;
}
// WARPFRAME_* flags of a frame for a w x h destination. Range flag: W, X, Y are affine in (x, y), so their extremes over
// [0, w-1] x [0, h-1] sit at the corners; the kernels' own per-pixel bounds are 2^-40 < |W| and |W|, |X|, |Y| < 2^40; the
// corners are tested in double against 2^-36 / 2^36, which leaves the f32 rounding of the kernels' fma chains (relative
// 1e-7) far inside the margin. A NaN or infinite entry fails every comparison: the flag stays clear and the kernel tests
// pixel by pixel.
__host__ __device__ inline int warp_frame_flags(const void* src, const float* M, size_t src_row_bytes, int w, int h, int is_affine) {
    int flags = (((unsigned long long)(size_t)src | (unsigned long long)src_row_bytes) & 3) == 0 ? WARPFRAME_SRC_ALIGNED4 : 0;
    if (is_affine) return flags;
    bool ok = true;
    double wsign = 0;
    const double cx[2] = {0.0, (double)(w - 1)}, cy[2] = {0.0, (double)(h - 1)};
    for (int k = 0; k < 4 && ok; k++) {
        const double x = cx[k & 1], y = cy[k >> 1];
        const double X = (double)M[0] * x + (double)M[1] * y + (double)M[2];
        const double Y = (double)M[3] * x + (double)M[4] * y + (double)M[5];
        const double W = (double)M[6] * x + (double)M[7] * y + (double)M[8];
        const double lim = 68719476736.0;       // 2^36
        const double aW = W < 0 ? -W : W, aX = X < 0 ? -X : X, aY = Y < 0 ? -Y : Y;
        ok = aW > 1.0 / lim && aW < lim && aX < lim && aY < lim;
        if (k == 0) wsign = W; else ok = ok && (W > 0) == (wsign > 0);       // no zero crossing of W inside the rectangle
    }
    return ok ? flags | WARPFRAME_DIV_IN_RANGE : flags;
}
__host__ __device__ inline void warp_frame_make(WarpFrame& wf, const void* src, const double* M, int is_affine) {
    double inv[9];
    if (is_affine) warp_invert_affine(M, inv); else warp_invert3x3(M, inv);
    wf.src = src;
    wf.flags = 0;
    for (int k = 0; k < 9; k++) { wf.Md[k] = inv[k]; wf.M[k] = (float)inv[k]; }
}

struct WarpArgs {
    const WarpFrame* frames;
    int n_frames;
    int sw, sh, cn;
    size_t src_stride;           // elements per source row
    float alpha;
    int border_mode;
    float bv[4];
    float* acc;
    int dw, dh;
    size_t acc_stride;           // floats per accumulator row
    int accumulate;              // 0: overwrite, 1: acc += sum of warped frames
    int is_affine;
    int subpixel_bits;           // 0 or 5
    int tune;                    // launch shape of the u8 fast path (option "warp_tune")
    int interp;                  // STK_INTER_LINEAR / STK_INTER_CUBIC (option "warp_interpolation"; cubic: warp_cubic_body.h)
};

// One sigma-clipping pass over the fold's frames (kernels_clip.hip; definition: include/stacker.h, stk_clip_params). The
// c / L / U planes are tightly packed dw x dh x cn f32; each pass reads them once and writes them once (pass `last`: out and
// counts instead). first: L = -inf, U = +inf without reading the planes.
struct ClipArgs {
    float* c;
    float* L;
    float* U;
    size_t plane_stride;         // floats per row of the c / L / U planes and of counts (dw x cn)
    float* out;                  // last pass: the clipped mean, row stride out_stride floats
    size_t out_stride;
    int* counts;                 // last pass: samples kept, tightly packed; null = not wanted
    float kappa_low, kappa_high;
    int first, last;
    // the fold's store mode (FoldStore, warp_body.h; kernels_quantile.hip): the samples of destination rows [y0, y0 +
    // band_rows) go to band[((i * band_rows + y - y0) * dw + x) * cn + c] for entry i of the frame table; plane_stride = dw x cn
    float* band;
    int y0, band_rows;
    // the fold's weighted mode (FoldWeighted, warp_body.h; kernels_weighted.hip): per-entry gain / offset / weight, indexed
    // like the frame table; the result goes to out / out_stride, the summed weight den to `den` (dw x dh, optional)
    const stk_frame_weight* coef;
    float* den;
    size_t den_stride;
    int coverage;                // 0: kappa = 1 (border samples count); 1: kappa = the bilinear weight on in-frame taps
    // the generic kernel's moments mode (FoldMoments): stepped pixels (step * k), `reps` stepped rows per thread, one
    // partial of 1 + 5 cn doubles per wave and entry
    double* partials;
    int step, reps;
    // the weighted clip states (ClipWGeneric / ClipWU8C3, kernels_clip.hip; definition: include/stacker.h, "normalised,
    // coverage-aware rejection"): coef / coverage as above; centre = 1: the centre pass (c = the weighted mean of the
    // participating samples, written to the c plane; nothing is read); last pass: the kept weight sw to `kept` (optional)
    int centre;
    float* kept;
    // the fold's local mode (FoldLocal, warp_body.h; kernels_local.hip; definition: include/stacker.h, stk_local_params):
    // coef / out / den as in the weighted mode; maps[i] = the weight plane of table entry i (sw x sh f32, row stride
    // map_stride floats), sampled bilinearly at the entry's coordinates; floor and power shape the weight
    const float* const* maps;
    size_t map_stride;
    float floor;
    int power;
    // the generic kernel's mesh variant (Mesh<State>, warp_body.h; kernels_mesh.hip; definition: include/stacker.h, "Mesh
    // fold"): fields[i] = the node field of table entry i (mesh_gh x mesh_gw x 2 f32, dx and dy interleaved; null = the
    // entry is not displaced), node spacing 1 << mesh_shift destination pixels, mesh_inv = 1.0f / spacing
    const float* const* fields;
    int mesh_shift, mesh_gw, mesh_gh;
    float mesh_inv;
    // local normalisation (FoldNorm / FoldStoreNorm, warp_body.h; kernels_local_norm.hip; definition: include/stacker.h,
    // "Local normalisation"): norm[i] = the gain / offset plane of table entry i (norm_gh x norm_gw x 2 cn f32, per node
    // the cn gains, then the cn offsets; null = the entry's record in coef as constants), node spacing 1 << norm_shift
    // destination pixels, norm_inv = 1.0f / spacing. coef / coverage / out / den / band as in the weighted modes
    const float* const* norm;
    int norm_shift, norm_gw, norm_gh;
    float norm_inv;
    // the cell moments pass (local_moments_kernel): cells = (n_frames - 1) x cell_h x cell_w records of cn x 6 doubles,
    // entry 1 first; a cell is 1 << cell_shift destination pixels wide and high; `step` above is the stat step
    double* cells;
    int cell_shift, cell_w, cell_h;
};

// quantile combines: samples per pixel the selection kernel takes (64 lanes of a wave x 64 keys in registers)
constexpr int QUANTILE_MAX_SAMPLES = 4096;
// the store mode with participation marks an entry that is no sample of a pixel with this bit pattern: a SIGNALLING NaN.
// A sample is the result of a floating-point add, and an arithmetic result that is NaN is always a quiet one (IEEE 754;
// the kernels run with the IEEE mode bit set), so no sample, a genuine NaN of any payload included, has these bits
constexpr unsigned QUANTILE_ABSENT_BITS = 0x7fa00000u;

// ---- kernel launchers (defined in the .hip files) -------------------------------------------
hipError_t launch_grey(const void* bgr, int depth, int w, int h, size_t stride_bytes, void* out, hipStream_t s,
                       int n_frames = 1, size_t src_frame_bytes = 0, size_t out_frame_elems = 0, int cn = 3 /* 3 BGR, 4 BGRA */);
hipError_t launch_convert_f32(const void* src, int depth, size_t n, float alpha, float* out, hipStream_t s);
// BGR (cn==3) or grey (cn==1) image -> GaussianBlur(float(grey), ksize) f32 plane with row stride out_stride
hipError_t launch_bgr16_to_grey8(const void* bgr16, int w, int h, size_t stride_bytes, uint8_t* out, hipStream_t s, int n_frames = 1,
                                 size_t src_frame_bytes = 0, size_t out_frame_elems = 0);
hipError_t launch_grey_blur(const void* src, int depth, int cn, int w, int h, size_t stride_bytes, int ksize,
                            float* out, int out_stride, hipStream_t s);
// the same for n BGR frames (u8 / u16) in one launch (frame z: ptrs_dev[z], or base + z * frame_bytes when ptrs_dev is null),
// plane z written at out + z * out_plane_stride; hipErrorNotSupported if the streaming kernel does not apply
hipError_t launch_grey_blur_batch(const void* const* ptrs_dev, const void* base, size_t frame_bytes, int n, int depth, int w, int h,
                                  size_t stride_bytes, int ksize, float* out, int out_stride, size_t out_plane_stride, hipStream_t s);
// blurred plane (stride in_stride) -> padded I/gx/gy planes
hipError_t launch_ref_planes(const float* blurred, int in_stride, int w, int h, float* I, float* gx, float* gy, float* gxy,
                             float* igg, int ref_stride, hipStream_t s);
// variant: 3 = production kernels, 0 = direct cross-check version
hipError_t launch_ecc_iter_col(const EccIterArgs& a, int motion, hipStream_t s);   // kernels_ecc_col.hip; a.units_q / units_r set
hipError_t launch_ecc_iter(const EccIterArgs& a, int motion, int variant, hipStream_t s);
// one slot at the start of a frame's life — frame 0, iteration 0, the identity, no centring (kernels_ecc_col.hip)
hipError_t launch_ecc_first_slot(EccSlot* slot, hipStream_t s);
hipError_t launch_ecc_solve(const EccIterArgs& a, int motion, EccCriteria crit, EccQueue* queue,
                            EccFrameResult* results, hipStream_t s, const float* init_warps = nullptr);
hipError_t launch_sharpness(const void* grey, int depth, int w, int h, int metric, int ksize, void* partials, int n_blocks,
                            hipStream_t s);
// the four sharpness metrics of n 8-bit frames (cn 1, 3 or 4; frames_dev: device array of n frame pointers) in one pass
// (kernels_quality.hip): per-tile partials (n x quality_tiles(w, h) x 6 int64), reduced to records (n x 6 int64: LAPM x4,
// LAPV sum and sum of squares, TENG, GLVN sum and sum of squares); n <= 65535
int quality_tiles(int w, int h);
hipError_t launch_quality(const void* const* frames_dev, int n, int cn, int w, int h, size_t stride_bytes, int ksize,
                          long long* partials, long long* records, hipStream_t s);
hipError_t launch_ecc_init(EccSlot* slots, int n_slots, int* tickets, EccQueue* queue, int n_frames, EccFrameResult* results,
                           const float* init_warps /* n_frames*9 or null */, hipStream_t s, int ready0 = -1 /* -1: all */);
hipError_t launch_ecc_set_ready(EccQueue* queue, int ready, hipStream_t s);
hipError_t launch_warp_accumulate(const WarpArgs& a, int depth, hipStream_t s);
// one clipping pass over the frames of `a` (a.acc unused); same kernel choice as launch_warp_accumulate
hipError_t launch_clip_pass(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s);
// the store mode over the frames of `a` for one band (c.band, c.y0, c.band_rows, c.plane_stride; a.acc unused); same kernel
// choice as launch_clip_pass
// the weighted fold over the frames of `a` (c.coef, c.coverage, c.out / c.out_stride, c.den / c.den_stride; a.acc unused);
// same kernel choice as launch_clip_pass
hipError_t launch_weighted_fold(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s);
// the local-weighted fold over the frames of `a` (c.coef, c.maps / c.map_stride, c.floor, c.power, c.out / c.out_stride,
// c.den / c.den_stride; a.acc unused): the generic kernels, linear or cubic (kernels_local.hip)
hipError_t launch_local_fold(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s);
// the local quality maps of n 8-bit frames (cn 1, 3 or 4; frames_dev / maps_dev: device arrays of n frame pointers and n
// w x h f32 plane pointers) in one launch (kernels_local.hip; definition: include/stacker.h, stk_local_params); n <= 65535
int local_map_tiles(int w, int h);
hipError_t launch_local_maps(const void* const* frames_dev, float* const* maps_dev, int n, int cn, int w, int h, size_t stride_bytes,
                             int radius, int threshold, hipStream_t s);
// star detection over n 8-bit frames (cn 1, 3 or 4; frames_dev: a device array of n frame pointers) in one launch
// (kernels_star.hip; definition: include/stacker.h, stk_star_params); n <= 65535. Per (frame, tile of 64 x 64): counts[frame *
// tiles + tile] = the tile's peaks, records[(frame * tiles + tile) * STAR_TILE_CAP + rank] = the peak of that rank under the
// key (S descending, py ascending, px ascending), rank < STAR_TILE_CAP; slots from min(count, STAR_TILE_CAP) on are not written
constexpr int STAR_TILE_CAP = 32;            // include/stacker.h: STK_STAR_TILE_CAP
struct StarRecord { int32_t px, py, S, Sx, Sy, peak, npix, pad; };
struct StarDetectArgs {
    const void* const* frames;
    int32_t* counts;
    StarRecord* records;
    int w, h;
    size_t stride;               // bytes per frame row
    int tiles_x, tiles;
    int radius;
    float ks;                    // (float)(kappa * 1.4826), from the host
    int min_contrast, min_pixels;
};
int star_tiles(int w, int h);
hipError_t launch_star_detect(const void* const* frames_dev, int n, int cn, int w, int h, size_t stride_bytes, int radius, float ks,
                              int min_contrast, int min_pixels, int32_t* counts, StarRecord* records, hipStream_t s);
// the same over frames of depth 8, 16 or 32 on the 16-bit key (kernels_star_deep.hip; definition: include/stacker.h,
// stk_star_deep_params): exact median and MAD of 16-bit keys, min_contrast in key units, f32_scale read at depth 32 only. The
// same counts and record slots
hipError_t launch_star_detect_deep(const void* const* frames_dev, int n, int depth, int cn, int w, int h, size_t stride_bytes, int radius,
                                   float ks, int min_contrast, int min_pixels, float f32_scale, int32_t* counts, StarRecord* records,
                                   hipStream_t s);
// star shapes on the same key (kernels_star_measure.hip; definition: include/stacker.h, stk_star_measure_params): one wave per
// star, n <= 65535 frames in one launch. stars: n x max_stars (px, py) pairs, counts[frame] of them in use; records: n x
// max_stars, record k of a frame = the measurement of its k-th pair; slots from counts[frame] on are not written
struct StarMeasureRecord { int64_t S, Sx, Sy, Sxx, Syy, Sxy; int32_t bg, mad, thr, npix, peak, n_ring, flags, pad; };
struct StarMeasureArgs {
    const void* const* frames;
    const int32_t* stars;        // px, py per star
    const int32_t* counts;
    StarMeasureRecord* records;
    int w, h;
    size_t stride;               // bytes per frame row
    int max_stars;
    int radius, ring_inner, ring_outer;
    float ks;                    // (float)(kappa * 1.4826), from the host
    int min_contrast, min_pixels, saturation;
};
hipError_t launch_star_measure(const StarMeasureArgs& a, int n, int depth, int cn, float f32_scale, hipStream_t s);
// the noise histograms of n 8- or 16-bit frames (cn 1, 3 or 4; frames_dev: a device array of n frame pointers) in one launch
// (kernels_noise.hip; definition: include/stacker.h, stk_noise_stat); n <= 65535, w, h >= 3. hist: n x cn x
// noise_hist_bins(depth) uint32, ZEROED by the caller on the same stream: per frame and channel the value histogram (256 /
// 65 536 bins), then the residual histogram (2041 / 65 536 bins). origin: n x cn int32 of scratch (depth 16 only)
size_t noise_hist_bins(int depth);
hipError_t launch_noise_hist(const void* const* frames_dev, int n, int cn, int depth, int w, int h, size_t stride_bytes, uint32_t* hist,
                             int32_t* origin, hipStream_t s);
// frame calibration (kernels_calibrate.hip; definition: include/stacker.h, stk_calibration). One record per frame of the
// launch; a master that is absent is a null pointer. Strides of the frames in bytes, of the masters in floats.
constexpr int CAL_TW = 64, CAL_TH = 4;       // pixels per workgroup tile of calibrate_kernel
constexpr int CAL_CHUNK = 16;                // frames per workgroup (option "calibrate_chunk")
constexpr int DEF_TW = 64, DEF_TH = 16;      // pixels per workgroup tile of defect_map_kernel
struct CalFrame { const void* src; void* dst; float dark_scale; int pad; };
struct CalArgs {
    const CalFrame* frames;
    int n, chunk;
    int w, h;
    size_t in_stride, out_stride;
    const float* bias; const float* dark; const float* flat;
    size_t bias_stride, dark_stride, flat_stride;
    const uint8_t* defects;      // w x h, tightly packed; null = none
    int step;
    float flat_mean[4];
    float flat_min, pedestal;
};
// depth: the frames' (8 / 16 / 32); out_depth: depth or 32; cn 1, 3 or 4; a.n <= a.chunk * 65535
hipError_t launch_calibrate(const CalArgs& a, int depth, int out_depth, int cn, hipStream_t s);
// the defect map of one master (w x h x cn f32, `stride` floats per row) into map (w x h bytes); counts: 4 device counters
// (unsigned long long), zeroed by the caller, that receive the set bits per channel of the bytes written
hipError_t launch_defect_map(const float* master, size_t stride, int w, int h, int cn, int tests, float high_abs, float low_ratio,
                             int step, int accumulate, uint8_t* map, unsigned long long* counts, hipStream_t s);
// per-channel f64 sums of an f32 image: one partial per row and channel into partials (h x 4 doubles), then added in row
// order into sums (4 doubles)
hipError_t launch_image_sums(const float* image, size_t stride, int w, int h, int cn, double* partials, double* sums, hipStream_t s);
// background model (kernels_background.hip; definition: include/stacker.h, stk_background_params). frames: a device array
// of the launch's frame pointers; stride in bytes; mask: w x h bytes on the device, or null; cells: per (frame, node,
// channel < min(cn, 3)) one record, frame-major; ks = (float)(kappa * 1.4826) from the host; n <= 65535
struct BgCellsArgs {
    const void* const* frames;
    const uint8_t* mask;
    stk_bg_cell* cells;
    int w, h;
    size_t stride;
    int step, gw, gh;
    int clip_iters;
    float ks, f32_scale;
};
hipError_t launch_background_cells(const BgCellsArgs& a, int n, int depth, int cn, hipStream_t s);
// the subtraction: one record per frame of the launch (plane: gh x gw x min(cn, 3) f32 on the device, or null = 0); strides
// in bytes; depth: the frames' (8 / 16 / 32); out_depth: depth or 32; cn 1, 3 or 4; a.n <= 65535
constexpr int BG_TW = 64, BG_TH = 16;        // pixels per workgroup tile of background_apply_kernel
constexpr int BG_ROWS = 4;                   // 64-pixel row segments per wave
struct BgFrame { const void* src; void* dst; const float* plane; };
struct BgApplyArgs {
    const BgFrame* frames;
    int n;
    int w, h;
    size_t in_stride, out_stride;
    int shift, gw, gh;           // step = 1 << shift
    float inv;                   // 1.0f / step
    float target[4];
};
hipError_t launch_background_apply(const BgApplyArgs& a, int depth, int out_depth, int cn, hipStream_t s);
// deconvolution (kernels_deconvolve.hip; definition: include/stacker.h, "deconvolution"). The work planes are planar f32,
// w x h tightly packed, `plane` floats apart, one per colour channel (min(cn, 3) of them); strides of the caller's images
// in floats. A workgroup owns a DCV_TW x (DCV_TH DCV_NY) tile of one plane; a thread DCV_NY runs of 4 outputs, 16 rows apart.
#ifndef DCV_NY
#define DCV_NY 2                             // rows of outputs per thread (1 or 2: measured)
#endif
constexpr int DCV_TW = 64, DCV_TH = 16 * DCV_NY;
constexpr int DCV_PITCH = 128;               // floats per staged row: a multiple of 64 keeps ds_read_b128 conflict-free
inline int dcv_halo(int radius) { return radius <= 8 ? 8 : 16; }                  // the staged halo along x, by radius class
inline int dcv_tap_pitch(int radius) { return 2 * dcv_halo(radius) + 8; }         // floats per row of the padded tap table
inline size_t dcv_tap_floats(int radius) { return (size_t)(2 * radius + 1) * dcv_tap_pitch(radius); }
// the padded tap table of a PSF: row j + R, column i + halo + 3 holds P[j + R][i + R]; the rest is 0 and is never multiplied
inline void dcv_pad_taps(const float* psf, int radius, float* table) {
    const int side = 2 * radius + 1, pitch = dcv_tap_pitch(radius), H = dcv_halo(radius);
    for (size_t k = 0; k < dcv_tap_floats(radius); k++) table[k] = 0.0f;
    for (int j = 0; j < side; j++)
        for (int i = 0; i < side; i++) table[(size_t)j * pitch + (i - radius + H + 3)] = psf[j * side + i];
}
// D = in + pedestal, not finite or below 0 -> 0, de-interleaved; cn == 4: the alpha samples go to `out` as they are
struct DeconvInitArgs {
    const float* in; float* out; float* D;
    size_t in_stride, out_stride, plane;
    int w, h;
    float pedestal;
};
hipError_t launch_deconv_init(const DeconvInitArgs& a, int cn, hipStream_t s);
// one pass over the colour planes. Ratio: stage u (src), dst = D / fmaxf(P * u, floor). Update: stage r (src), v = u C, the
// regulariser (lambda > 0), dst = u_{k+1}; last != 0: the output step into `out` (pixel stride cn floats) instead of dst.
struct DeconvPassArgs {
    const float* taps;                       // dcv_pad_taps, on the device
    const float* src; const float* D; const float* u; float* dst;
    float* out; const float* mask;           // mask: one f32 plane or null
    size_t out_stride, mask_stride, plane;
    int w, h, cn, channels, radius, last;    // channels: planes of the launch
    float floor, lambda, e2, amount, pedestal;
};
hipError_t launch_deconv_ratio(const DeconvPassArgs& a, hipStream_t s);
hipError_t launch_deconv_update(const DeconvPassArgs& a, hipStream_t s);
// wavelet layers (post/kernels_wavelet.hip; definition: include/stacker.h, "wavelet layers"). The work planes are planar f32,
// w x h tightly packed, `plane` floats apart, one per colour channel (min(cn, 3) of them); strides of the caller's images
// in floats. A workgroup owns WV_TW columns and, at tap spacing s, four rows of each of four residue classes modulo s: at
// s = 1 a WV_TW x WV_TH tile.
constexpr int WV_TW = 64, WV_TH = 16;
constexpr int WV_FORM_DIRECT = 0, WV_FORM_STAGED = 1;
constexpr int WV_STAGED_MAX_S = 32;          // at s = 64 the halo (2 s a side) outgrows the tile
constexpr int WV_DIGIT_BITS = 8, WV_ROUNDS = 4, WV_BINS = 1 << WV_DIGIT_BITS;     // the radix selection: 4 rounds of 8 bits
// c_0 = the sanitised image, de-interleaved; cn == 4 and `alpha`: the alpha samples go to every image of `alpha` as they are
struct WvInitArgs {
    const float* in; float* c0;
    float* alpha[9]; size_t alpha_stride[9]; int n_alpha;
    size_t in_stride, plane;
    int w, h;
};
hipError_t launch_wavelet_init(const WvInitArgs& a, int cn, hipStream_t s);
// one level over the colour planes: c_{j+1} = the dilated B3 spline of c_j (src -> dst), w_j = c_j - c_{j+1}.
// layers == 0: the layer operation and acc (first: acc = gain w', else acc += gain w'); last: the output step into `out`
// instead of dst and acc, D read again from `in`. layers != 0: w_j into `wout`, and on the last level c_J into `cout`.
struct WvLevelArgs {
    const float* src; float* dst; float* acc;
    const float* in; float* out; const float* mask;
    float* wout; float* cout;
    size_t in_stride, out_stride, mask_stride, wout_stride, cout_stride, plane;
    int w, h, cn, channels, s, mode, first, last, layers;
    int form;                                // WV_FORM_*: the staged form applies up to WV_STAGED_MAX_S, beyond it the direct one runs
    float t[3];                              // the threshold of this level per colour channel
    float keep, layer_amount, gain, residual_gain, amount;
};
hipError_t launch_wavelet_level(const WvLevelArgs& a, hipStream_t s);
// the selection of the ((N + 1) / 2)-th smallest key bits(fabsf(w_0)) per colour channel. state: per channel 2 words (the
// prefix found so far, the rank left inside it), then per channel WV_BINS histogram words. reset: state = (0, rank) and
// zero counts; hist: one round's counts of the digit below the prefix; pick: the digit, into the prefix, counts zeroed.
struct WvSelectArgs {
    const float* c0; uint32_t* state;
    size_t plane;
    int w, h, channels, round;
    uint32_t rank;
};
inline size_t wv_state_words(int channels) { return (size_t)channels * (2 + WV_BINS); }
hipError_t launch_wavelet_select_reset(const WvSelectArgs& a, hipStream_t s);
hipError_t launch_wavelet_select_hist(const WvSelectArgs& a, hipStream_t s);
hipError_t launch_wavelet_select_pick(const WvSelectArgs& a, hipStream_t s);
// display stretch (post/kernels_stretch.hip; definition: include/stacker.h, "display stretch"). Strides of the images in
// ELEMENTS of their depth. The statistics: an exact radix selection of up to ST_SLOTS ranks per colour channel at once, 4
// rounds of 8 bits from the top of an order-preserving 32-bit key. A slot is one rank: slot 0 the median, slots 1 .. 4 the
// quantiles (the values' phase: the key is the sign-flipped value), slot ST_MAD the MAD (its own phase: the key is
// bits(fabsf(v - median)), the median decoded from slot 0). state, in words: per channel ST_HEAD words (the smallest and the
// largest key), then per (channel, slot) 2 words (the prefix found so far, the rank left inside it), then per (channel, slot)
// ST_BINS histogram words. Round 0 of the values' phase has no prefix: one histogram (slot 0's) serves every slot; its sum
// is N, which the host reads to form the ranks.
constexpr int ST_DIGIT_BITS = 8, ST_ROUNDS = 4, ST_BINS = 1 << ST_DIGIT_BITS;
constexpr int ST_SLOTS = 6, ST_MAD = 5, ST_HEAD = 2;
constexpr int ST_FORM_DIRECT = 0, ST_FORM_MERGED = 1;     // the histogram launch: one LDS atomic per key, or per run of equal digits of a thread
// the hist launch's workgroups: rows beyond them are strided by the grid. 4 per CU: every workgroup ends by flushing its bins
// with global atomics on the same few words, and 4096 of them measured 1.54 x slower over the call
constexpr int ST_TARGET_BLOCKS = 1024;
__host__ __device__ inline size_t st_sel_at(int channels, int c, int slot) { return (size_t)channels * ST_HEAD + ((size_t)c * ST_SLOTS + slot) * 2; }
__host__ __device__ inline size_t st_bins_at(int channels, int c, int slot) { return (size_t)channels * (ST_HEAD + 2 * ST_SLOTS) + ((size_t)c * ST_SLOTS + slot) * ST_BINS; }
__host__ __device__ inline size_t st_state_words(int channels) { return (size_t)channels * (ST_HEAD + ST_SLOTS * (2 + ST_BINS)); }
struct StStatArgs {
    const float* in; const float* mask; uint32_t* state;
    size_t in_stride, mask_stride;
    int w, h, cn, channels;
    int form;                                // ST_FORM_*
    int round, slot0, slots;                 // the slots of this phase: slot0 .. slot0 + slots - 1 (values: 0, 1 + quantiles; MAD: ST_MAD, 1)
    uint32_t rank[3][ST_SLOTS];              // read by the pick of round 0
};
hipError_t launch_stretch_stat_reset(const StStatArgs& a, hipStream_t s);
hipError_t launch_stretch_stat_hist(const StStatArgs& a, hipStream_t s);
hipError_t launch_stretch_stat_pick(const StStatArgs& a, hipStream_t s);
struct StStretchArgs {
    const float* in; void* out; const float* table;
    size_t in_stride, out_stride;
    int w, h, cn, depth, curve, colour, knots;
    float black[3], r[3], mid[3], mm1[3], k[3];
    float out_scale;
};
hipError_t launch_stretch(const StStretchArgs& a, hipStream_t s);
// colour-filter mosaics (kernels_demosaic.hip; definition: include/stacker.h, stk_mosaic). One record per frame of the
// launch; strides in bytes; (w, h): the mosaic's size, at least 3 x 3 (superpixel: 2 x 2).
constexpr int DEM_TW = 64, DEM_TH = 16;      // output pixels per workgroup tile of demosaic_kernel (32 x 8 cells of 2 x 2)
constexpr int DEM_SP_TH = 4;                 // output rows per workgroup of the superpixel kernel
struct DemFrame { const void* src; void* dst; };
struct DemArgs {
    const DemFrame* frames;
    int n;
    int w, h;
    int pattern;                 // STK_CFA_*: bit 0 / bit 1 = the column / row parity of the red sites
    size_t in_stride, out_stride;
};
// depth: the mosaic's (8 / 16 / 32); out_depth: depth or 32; method: STK_DEMOSAIC_*; a.n <= 65535
hipError_t launch_demosaic(const DemArgs& a, int depth, int out_depth, int method, hipStream_t s);
// plane (w x h f32, tightly packed): 1 where the site's colour is `channel` (0 = B, 1 = G, 2 = R), else 0
hipError_t launch_cfa_mask(float* plane, int w, int h, int pattern, int channel, hipStream_t s);
// local alignment (kernels_mesh.hip; definition: include/stacker.h, stk_mesh_params). Entry 0 of `frames` is frame 0 (its
// matrix is not read); entries 1 .. n_entries - 1 are the frames that get a field: fields[k] (gh x gw x 2 f32) and status[k]
// (gh x gw int32; the array or an entry may be null) are indexed like the table
struct MeshLkArgs {
    const WarpFrame* frames;
    float* const* fields;
    int* const* status;
    int n_entries;
    int w, h;                    // the frames' size = the destination's
    size_t stride;               // bytes per frame row
    int is_affine;
    int step, gw, gh, radius, max_iters;
    double eps2, max_shift2, min_eig4;   // epsilon^2, max_shift^2, 4 min_eig
    // the seeded form only (launch_mesh_lk_seeded; one level of stk_local_align_pyramid): w, h, stride and the table are the
    // level's, a node's centre is (k step >> level, j step >> level). valid[k]: the validity bytes of entry k (gh x gw).
    // top != 0: the seed is (0, 0) and valid = status > 0; else the seed is 2 x fields[k][node] and a node that fails keeps
    // its byte. A node that fails keeps its seed as d.
    uint8_t* const* valid;
    int level, top;
};
hipError_t launch_mesh_lk(const MeshLkArgs& a, int cn, hipStream_t s);
hipError_t launch_mesh_lk_seeded(const MeshLkArgs& a, int cn, hipStream_t s);
// the hole filling with the validity carried in valid[k] (read first, written back after the last pass) instead of status > 0
hipError_t launch_mesh_fill_valid(float* const* fields, uint8_t* const* valid, int n_entries, int gw, int gh, int passes, void* scratch,
                                  hipStream_t s);
// Box pyramid of the integer grey (include/stacker.h, "Level images"): levels 1 .. levels - 1 of table entries first ..
// first + n - 1 (frames[k].src: w x h x cn u8, `stride` bytes per row) in one pass. Level l of entry k is (w >> l) x
// (h >> l) bytes, tightly packed, at planes + k entry_stride + mesh_pyr_offset(w, h, l).
struct MeshPyrArgs {
    const WarpFrame* frames;
    uint8_t* planes;
    size_t entry_stride, stride;
    int first, n, w, h, levels;
};
__host__ __device__ inline size_t mesh_pyr_offset(int w, int h, int level) {
    size_t o = 0;
    for (int l = 1; l < level; l++) o += (size_t)(w >> l) * (size_t)(h >> l);
    return o;
}
hipError_t launch_mesh_pyr(const MeshPyrArgs& a, int cn, hipStream_t s);
// `passes` hole-filling passes over the fields of entries 1 .. n_entries - 1; scratch: (n_entries - 1) x
// mesh_fill_scratch_bytes(gw, gh) bytes of device memory
inline size_t mesh_fill_scratch_bytes(int gw, int gh) { return ((size_t)gw * gh * (2 * sizeof(float) + 2) + 255) & ~(size_t)255; }
hipError_t launch_mesh_fill(float* const* fields, const int* const* status, int n_entries, int gw, int gh, int passes, void* scratch,
                            hipStream_t s);
// the mesh folds over the frames of `a` (c.fields, c.mesh_*): the generic kernel's mesh variant, linear only; local: the
// local-weighted state (launch_local_fold's fields of c), else the running sums into a.acc
hipError_t launch_mesh_fold(const WarpArgs& a, const ClipArgs& c, int depth, bool local, hipStream_t s);
// stepped grid of the moments pass for a dw x dh destination: columns, rows per thread, workgroups in x and y. Rows per
// thread: at least 8, and enough that an entry has about 1024 partials at most (the second launch adds them one after the other)
struct MomentsPlan { int gw, gh, reps, bx, by; size_t parts() const { return (size_t)bx * by * 4; } };
inline MomentsPlan moments_plan(int dw, int dh, int step) {
    MomentsPlan p;
    p.gw = (dw + step - 1) / step;
    p.gh = (dh + step - 1) / step;
    p.bx = (p.gw + 63) / 64;
    const long long want = ((long long)p.bx * p.gh + 1023) / 1024;
    p.reps = (int)(want < 8 ? 8 : want);
    p.by = (p.gh + 4 * p.reps - 1) / (4 * p.reps);
    return p;
}
// overlap moments of entries 1 .. a.n_frames - 1 against entry 0 (include/stacker.h): per-wave partials into c.partials
// ((n_frames - 1) x plan.parts() x (1 + 5 cn) doubles), then reduced in index order into moments ((n_frames - 1) x cn x 6)
hipError_t launch_overlap_moments(const WarpArgs& a, ClipArgs c, int depth, int step, double* moments, hipStream_t s);
// local normalisation (kernels_local_norm.hip). The cell moments of entries 1 .. a.n_frames - 1 against entry 0 into
// c.cells (c.step, c.cell_shift, c.cell_w, c.cell_h): one wave per (cell, entry), no partials. The two folds through the
// planes of c.norm (c.norm_*; c.coef, c.coverage): the mean into c.out / c.den, and the store mode with participation for
// one band (launch_quantile_store_weighted's fields of c). Generic kernels only, linear or cubic.
hipError_t launch_local_moments(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s);
hipError_t launch_norm_fold(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s);
hipError_t launch_norm_store(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s);
hipError_t launch_quantile_store(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s);
// one pass of the weighted clip (c.coef, c.coverage, c.centre, c.kept besides launch_clip_pass's fields)
hipError_t launch_clip_pass_weighted(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s);
// one pass of the weighted clip through the planes of c.norm (c.norm_* besides launch_clip_pass_weighted's fields;
// ClipNorm / ClipNormU8C3, kernels_clip.hip): every kernel launch_clip_pass_weighted may choose, the u8 BGR fast ones included
hipError_t launch_clip_pass_norm(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s);
// the store mode with participation (c.coef, c.coverage besides launch_quantile_store's fields): the normalised sample
// u = s * g + o, QUANTILE_ABSENT_BITS for an entry that is no sample of the pixel
hipError_t launch_quantile_store_weighted(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s);
// the selection with a per-pixel rank over such a band: per column the number N_p of present keys, j and g from N_p and q,
// the quantile (0 where N_p == 0) into out[k]; counts (optional): N_p of pixel k / cn, written for channel 0
hipError_t launch_quantile_select_masked(const float* band, size_t m, int n, float q, int cn, float* out, int* counts, hipStream_t s);
// per column k < m of the n x m samples of a band (frame-major: band[i * m + k]): the quantile with lo = s_(j) and the
// fraction g (include/stacker.h), into out[k]; n <= QUANTILE_MAX_SAMPLES
hipError_t launch_quantile_select(const float* band, size_t m, int n, int j, float g, float* out, hipStream_t s);
// median / MAD clipping (kernels_robust_clip.hip; definition: include/stacker.h, stk_robust_clip_params): per column k < m
// of such a band the centre and the bounds after p.iterations rounds, into c[k], L[k], U[k]; masked: the band carries
// QUANTILE_ABSENT_BITS marks (launch_quantile_store_weighted); a column without a sample: c = 0, L = -inf, U = +inf
hipError_t launch_robust_select(const float* band, size_t m, int n, int masked, const stk_robust_clip_params& p, float* c, float* L,
                                float* U, hipStream_t s);
// the fold's frame table straight from the ECC results, on the device: entry 0 = the reference frame under the identity
// (if add_reference), then template k under results[k].warp — what the host loop of ecc_shard_impl builds, bit for bit
hipError_t launch_warp_frames_from_ecc(const EccFrameResult* results, const void* const* src_ptrs /* n_templates + 1, device */,
                                       int n_templates, int add_reference, int is_affine, int w, int h, size_t src_row_bytes,
                                       WarpFrame* out, hipStream_t s);
hipError_t launch_scale(const float* in, float* out, size_t n, float scale, hipStream_t s);
hipError_t launch_add(float* acc, const float* in, size_t n, hipStream_t s);

}  // namespace stk
