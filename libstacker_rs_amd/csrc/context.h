// context.h — the engine's per-GPU context (stk_ctx) and host helpers shared by stacker.cpp, keypoint.cpp and the combines
// (whose common front end is combine.h and whose common back end is workspace.h).
#pragma once
#include <cstdlib>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "combine.h"
#include "common.h"
#include "homography.h"
#include "keypoint.h"

// ---------------------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + (bytes >> 3);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T* as() const { return (T*)p; }
};

namespace stk { struct MultiState; }
void multi_destroy(stk_ctx* ctx);
stk_status multi_match(stk_ctx* ctx, int kind, const stk_frames* frames, const stk_keypoint_params* kp, const stk_ecc_params* ep,
                       float scale_down_width, stk_image_f32* out, int32_t* dropped_out, stk_frame_stats* stats);
stk_status set_option_one(stk_ctx* ctx, const char* name, int64_t value);
int multi_member_count(const stk_ctx* ctx);
stk_ctx* multi_member(const stk_ctx* ctx, int i);

// Frames that are still being produced (decoded) while the engine already runs: the uploader asks the gate before it
// copies a frame. `wait` blocks until the frame at `ptr` is complete and returns false if it never will be.
struct FrameGate { std::function<bool(const void* ptr)> wait; };

constexpr int STK_MAX_KP_LANES = 8;

struct stk_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t copy_stream = nullptr;    // host -> HBM copies of host-fed stacks (upload.cpp)
    hipStream_t prep_stream = nullptr;    // grey + blur of frames that arrive while the ECC queue is already running
    hipStream_t tail_stream = nullptr;    // highest priority: the keypoint lanes' descriptor / 2-NN / homography launches (keypoint.cpp)
    hipStream_t ecc_stream2 = nullptr;    // second launch sequence of the ECC queue (option ecc_groups = 2)
    std::vector<hipEvent_t> upload_events;
    hipEvent_t gate_ev = nullptr, gate_ev2 = nullptr;
    const FrameGate* frame_gate = nullptr;   // set by the path-based entry points for the duration of one call
    int opt_warp_tune = 0;
    int opt_prep_overlap = 1;             // ecc_match on a device-resident stack: templates prepared on the prep stream while the first frames iterate
    int opt_prep_stream = 1;              // 1: templates of a run of frames by the streaming grey+blur kernel in one launch; 0: tiled kernel, frame by frame
    int opt_upload_batch = 8;             // frames per host -> HBM batch
    std::string err;
    int opt_ecc_slots = 0;        // 0 = auto
    int opt_subpixel_bits = 0;
    int opt_interp = STK_INTER_LINEAR;    // option "warp_interpolation": the fold's resampling kernel (cubic needs opt_subpixel_bits == 0: check_frames)
    int opt_profile = 1;
    int opt_ecc_chunk = 0;        // (iterate, solve) pairs between two polls of the completion counter; 0 = by frame size (stacker.cpp: ecc_run)
    int opt_profile_stride = 1;   // profile = 2: bracket every n-th ECC pixel pass with an event pair
    bool opt_orb_resize_tables = true; // ORB pyramid steps by the table-driven kernel (false: tables computed per tile, round 2's kernel; same bits)
    bool opt_kp_tail_priority = true; // keypoint lanes: descriptor / 2-NN / homography launches on the highest-priority stream
    bool opt_orb_device_cull = true; // ORB: Harris cull and ordering of the short lists on the device (false: on the host pool); same keypoints
    bool opt_orb_fast_all = true;    // ORB: FAST + short lists of all levels in four launches where the pyramid allows it (false: level by level); same keypoints
    bool opt_orb_patch_blur = true;  // ORB: the descriptor kernel blurs the window it reads (false: blur every level whole, then sample)
    int opt_kp_lanes = 3;         // keypoint path on device-resident stacks: the stack is cut into this many runs of frames that go through the pipeline side by side (helper contexts), 1 = one pipeline
    int opt_kp_workers = 12;      // host threads for the per-frame host steps of the keypoint path (Harris cull, RANSAC)
    int opt_ecc_blocks = 0;       // total workgroups of one ECC iteration launch; 0 = 288 per frame in flight (see ecc_plan)
    int opt_ecc_ring = 1;         // column-walking ECC pass: frame-0 rows through the per-wave LDS ring (0: always gather from global memory)
    int opt_ecc_groups = 0;       // ECC slots in this many groups with their own launch sequences on two streams (stacker.cpp: ecc_run); 0 = by frame size
    int opt_ecc_ring_lookahead = 5;   // debug: frame-0 rows the ring keeps ahead (5 = production; less makes the run-time check fire and the strip fall back)
    int opt_ecc_first_iter = 1;   // column-walking homography pass: a frame's first iteration from the identity takes the short route (stacker.cpp: ecc_run); same bits
    int opt_ecc_variant = 3;      // ECC iteration kernel: 3 = production (column-walking homography pass / pipelined affine family), 0 = direct cross-check
    int opt_quantile_band_rows = 0;   // quantile combines: at most this many rows per band of samples; 0 = as many as fit the band budget
    int opt_calibrate_chunk = 0;      // stk_calibrate: frames per workgroup with the masters in registers; 0 = CAL_CHUNK
    stk_timing timing{};
    int64_t ecc_first_iter_slots = 0;   // stk_get_counter: slot-iterations of the last call that took the first-iteration route (reset by timing_begin)
    hipEvent_t ev[8] = {};
    hipEvent_t poll_ev[2] = {};
    int* host_done = nullptr;     // pinned, 16 ints: [0], [1] completion counters of the two chunks in flight, [2] ring fall-back count, [3] first-iteration slots
    const void* ref_zeroed_ptr = nullptr;   // the frame-0 planes' zero border exists for this buffer and geometry (ecc_prepare_reference)
    int ref_zeroed_w = 0, ref_zeroed_h = 0;
    // test hooks (stk_ecc_prepared, stk_get_counter "prep_stream_frames"): the geometry of the last ECC preparation, as
    // ecc_plan laid it out in ctx->templates / ctx->ref, and how many of its templates the streaming kernel wrote
    struct EccPrepared {
        bool valid = false;
        int w = 0, h = 0, n_templates = 0, templ_row_stride = 0, ref_stride = 0;
        size_t templ_plane_stride = 0, ref_plane_floats = 0;
    } ecc_prepared;
    int64_t prep_stream_frames = 0;     // (reset by timing_begin)
    std::vector<hipEvent_t> prof_ev;   // event pairs for per-launch timing (option profile = 2)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> fold_ev;   // event pairs around the keypoint path's fold launches (grow-only pool)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> select_ev; // event pairs around the median / MAD clip's selection launches, one per band (grow-only pool)
    int64_t robust_select_us = 0;   // stk_get_counter: device time of the last median / MAD clip's selection launches
    // page-locked host block the path-based entry points decode a stack into (imread.cpp: match_files); grow-only, like the
    // device workspaces: locking 6.4 GB of pages for a 256-frame 4K stack costs more than decoding into them
    unsigned char* files_block = nullptr; size_t files_block_cap = 0; bool files_block_pinned = false;
    // workspace
    DevBuf frames, ref, blur_tmp, templates, slots, queue, results, partials, first_sums, warpframes, acc, scratch, init_warps, frameptrs;
    // the combines' workspaces, each laid out by the struct named (workspace.h)
    DevBuf clip;                  // ClipLayout (clip.cpp, robust.cpp, robust_clip.cpp)
    DevBuf weighted;              // WeightedLayout
    DevBuf coef;                  // the rejection combines' per-entry record table (robust.cpp, robust_clip.cpp)
    DevBuf quantile;              // QuantileLayout; the band alone in robust_clip.cpp
    DevBuf local;                 // LocalLayout, NormLayout or DrizzleLayout, one call at a time
    DevBuf mesh;                  // MeshLayout, then PyrLayout; the pyramid planes alone in stk_grey_pyramid
    DevBuf reject;                // RejectLayout
    DevBuf quality;               // the whole-stack passes, one call at a time: sharpness (quality.cpp: frame pointers, per-frame records, tile
                                  // partials) or noise (noise.cpp: frame pointers, window origins, one batch's histograms)
    stk::KeypointWorkspace* kp = nullptr;
    stk::geom::HgWorkspace* hg = nullptr;   // findHomography batch workspace (homography.cpp)
    stk::HostPool* host_pool = nullptr;
    stk::HostPool* shared_pool = nullptr;  // not owned: the pool every member of a multi-device context shares (multi.cpp); overrides host_pool
    stk_ctx* lanes[STK_MAX_KP_LANES - 1] = {};   // hidden helper contexts of the same device: lanes 1.. of keypoint_align_impl (keypoint.cpp)

    stk::MultiState* multi = nullptr;      // non-null: this context spans several devices (multi.cpp); it is member 0 itself   // persistent host threads of the keypoint path (keypoint.cpp)
    std::mutex err_mutex;
    int64_t debug_poison_bytes = 0;        // stk_get_counter: the bytes the last debug_poison filled (this context, its lanes, its multi state)
};

// ---------------------------------------------------------------------------------------------
// The persistent memory of a context, enumerated in ONE place per struct: what stk_destroy (and its siblings) release and
// what the debug_poison option fills is the same list by construction (tests/test_cpu_history.py checks the members
// against it). `dev` sees every DevBuf; `host` every page-locked host block as (pointer, bytes, pinned), a null pointer
// included — files_block alone may be pageable (imread.cpp falls back to malloc), which is what `pinned` says.
using DevBufVisitor = std::function<void(DevBuf&)>;
using HostBlockVisitor = std::function<void(void* p, size_t bytes, bool pinned)>;
inline void for_each_workspace(stk_ctx* ctx, const DevBufVisitor& dev, const HostBlockVisitor& host = nullptr) {
    for (DevBuf* b : {&ctx->frames, &ctx->ref, &ctx->blur_tmp, &ctx->templates, &ctx->slots, &ctx->queue, &ctx->results, &ctx->partials,
                      &ctx->first_sums, &ctx->warpframes, &ctx->acc, &ctx->scratch, &ctx->init_warps, &ctx->frameptrs, &ctx->clip,
                      &ctx->weighted, &ctx->coef, &ctx->quantile, &ctx->local, &ctx->mesh, &ctx->reject, &ctx->quality})
        if (dev) dev(*b);
    if (!host) return;
    host(ctx->host_done, 16 * sizeof(int), true);
    host(ctx->files_block, ctx->files_block_cap, ctx->files_block_pinned);
}
namespace stk {
void for_each_workspace(KeypointWorkspace* k, const DevBufVisitor& dev, const HostBlockVisitor& host = nullptr);    // keypoint.cpp
// the caches of workspace CONTENT (the ORB resize tables' geometry key) forgotten: the next call computes them again
void keypoint_workspace_forget(KeypointWorkspace* k);
namespace geom { void for_each_workspace(HgWorkspace* w, const DevBufVisitor& dev, const HostBlockVisitor& host = nullptr); }   // homography.cpp
// (no host blocks; on_device: each member's device is made current for its buffers, the caller restores its own)
void for_each_workspace(MultiState* ms, const DevBufVisitor& dev, bool on_device = true);                         // multi.cpp
}  // namespace stk
// what every destroy does with the two kinds
inline void workspace_release_dev(DevBuf& b) { b.release(); }
inline void workspace_release_host(void* p, size_t, bool pinned) { if (!p) return; if (pinned) (void)hipHostFree(p); else std::free(p); }
// option debug_poison on a multi-device context's owner: its multi state's buffers, every one on its member's device
stk_status multi_poison(stk_ctx* ctx, int byte, int64_t* bytes);
int multi_workspaces_empty(const stk_ctx* ctx);

inline stk_status fail(stk_ctx* ctx, stk_status st, const std::string& msg) {
    if (!ctx) return st;
    std::lock_guard<std::mutex> lock(ctx->err_mutex);   // keypoint workers may fail concurrently
    ctx->err = msg;
    return st;
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ctx, STK_HIP_ERROR, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)


using stk::WarpFrame;
size_t frame_row_bytes(const stk_frames* f);
// the bytes of one frame that a copy out of the CALLER's memory takes: up to the last pixel of the last row. The padding
// behind that pixel is not the caller's to give (a ROI may end on the last byte of its parent buffer; include/stacker.h,
// row_stride_bytes). The engine's own buffers keep frames row_bytes * h apart; the bytes the copy leaves out are never used.
inline size_t frame_copy_bytes(size_t row_bytes, int w, int h, int cn, int depth) {
    return row_bytes * (size_t)(h - 1) + (size_t)w * cn * (depth / 8);
}
inline size_t frame_copy_bytes(const stk_frames* f) {
    const size_t tight = (size_t)f->width * f->channels * (f->depth / 8);
    return frame_copy_bytes(f->row_stride_bytes ? f->row_stride_bytes : tight, f->width, f->height, f->channels, f->depth);
}
stk_status resolve_frames(stk_ctx* ctx, const stk_frames* f, std::vector<const void*>& dev);
// folds: the call samples frames through warps (every stacking call): the fold's option pair is checked here, at the call
stk_status check_frames(stk_ctx* ctx, const stk_frames* f, bool need_bgr, bool folds = true);
// the bicubic fold is defined on exact coordinates only (include/stacker.h); the two options may be set in either order,
// so the pair is checked by every call that folds (inline: the files calls check it before they read a file)
inline stk_status check_fold_options(stk_ctx* ctx) {
    if (ctx->opt_interp == STK_INTER_CUBIC && ctx->opt_subpixel_bits != 0)
        return fail(ctx, STK_INVALID_PARAMS, "warp_interpolation = 2 (STK_INTER_CUBIC) needs warp_subpixel_bits = 0: the bicubic fold is defined on exact coordinates only");
    return STK_OK;
}
// (w, h): the SOURCE frames' size; (dw, dh): the accumulator's, 0 = the same (a stack of one geometry)
stk_status warp_fold(stk_ctx* ctx, std::vector<WarpFrame>& wf, int depth, int w, int h, int cn,
                     size_t src_row_bytes, double alpha, int border_mode, const double* border_value,
                     int is_affine, float* acc, size_t acc_stride_floats, int accumulate, int dw = 0, int dh = 0);
stk_status warp_fold_enqueue(stk_ctx* ctx, int n_frames, int depth, int w, int h, int cn, size_t src_row_bytes, double alpha,
                             int border_mode, const double* border_value, int is_affine, float* acc, size_t acc_stride_floats,
                             int accumulate, int first_frame = 0, int dw = 0, int dh = 0);
void make_warp_frame(WarpFrame& wf, const void* src, const double* M, int is_affine);
stk_status image_check(stk_ctx* ctx, const stk_image_f32* im, int w, int h, int c);
size_t image_stride_floats(const stk_image_f32* im);
void timing_begin(stk_ctx* ctx);
// closing formula of a sharpness metric from a frame's sums (quality.cpp; shared by stk_sharpness and stk_stack_sharpness)
double sharpness_finish(int metric, double s, double sq, int width, int height);
float ev_ms(hipEvent_t a, hipEvent_t b);

#include "workspace.h"

// shared internals of the entry points (stacker.cpp / keypoint.cpp / hybrid.cpp / clip.cpp / quantile.cpp)
// where the frames of a stack are after a whole-stack call on this context (upload.cpp / keypoint.cpp put host-fed stacks
// at ctx->frames + i * frame bytes)
void resident_frames(stk_ctx* ctx, const stk_frames* f, std::vector<const void*>& dev);
// stk_ecc_match / stk_keypoint_match on the context's own device: what they run on a plain context
stk_status ecc_match_single(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                            stk_image_f32* out, stk_frame_stats* stats);
stk_status keypoint_match_single(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                                 stk_image_f32* out, int32_t* dropped, stk_frame_stats* stats);
// the frame table of a fold into ctx->warpframes (flags for a w x h destination; asynchronous: `wf` must outlive the copy)
stk_status warp_table_upload(stk_ctx* ctx, std::vector<WarpFrame>& wf, size_t src_row_bytes, int w, int h, int is_affine);
// shared by the combines (clip.cpp, quantile.cpp, weighted.cpp; used again by robust.cpp); the frame table, the fold's
// geometry and the whole-stack scaffold they all start from: combine.h
stk_status clip_validate(stk_ctx* ctx, const stk_clip_params* p);
stk_status quantile_validate(stk_ctx* ctx, const stk_quantile_params* p);
stk_status quantile_check_count(stk_ctx* ctx, int n);
size_t quantile_band_rows(const stk_ctx* ctx, int n, int w, int h, int cn);
// the layout of an n-frame w x h x cn stack's quantile combine (n = 0: the image alone), ctx->quantile reserved for it
stk_status quantile_reserve(stk_ctx* ctx, int n, int w, int h, int cn, bool counts, QuantileLayout* L);
stk_status robust_clip_validate(stk_ctx* ctx, const stk_robust_clip_params* p);
// the median / MAD clip over the n_entries entries of ctx->warpframes (robust_clip.cpp): per band a store launch and the
// selection into the clip planes, then one last clip pass. coef: the per-entry records of the participation form (then
// `coverage` and `kept` apply), null = the plain form. Writes out / counts / kept (out's location), adds its device time to *ms.
// norm (with coef): the locally normalised form, the store launch and the last pass through its plane table
struct NormFoldArgs;
stk_status robust_clip_bands(stk_ctx* ctx, int n_entries, const std::vector<stk_frame_weight>* coef, const FoldSpec& spec, int coverage,
                             const stk_robust_clip_params* p, stk_image_f32* out, int32_t* counts, float* kept, double* ms,
                             const NormFoldArgs* norm = nullptr);
stk_status weighted_validate(stk_ctx* ctx, const stk_weight_params* p);
stk_status weighted_check_border(stk_ctx* ctx, int border_mode, const double* border_value, int coverage);
stk_status weighted_check_coefs(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, int cn);
stk_status weighted_moments(stk_ctx* ctx, int n_entries, const FoldSpec& spec, int step, double* host, double* ms);
void weighted_estimate(const double* m /* cn x 6 */, int cn, int mode, stk_frame_weight* e);
// the records of a whole-stack table's entries (entry 0 = frame 0; the table is uploaded), as stk_*_match_weighted makes
// them: the moments pass and the estimator when normalize != 0, the caller's weights by frame index; `applied` (or null) by
// frame index over the n frames (a dropped frame: weight 0, gains 1). Adds the pass's device time to *ms.
stk_status weighted_match_records(stk_ctx* ctx, int n, const EntryTable& table, const FoldSpec& spec, const stk_weight_params* p,
                                  const float* weights, std::vector<stk_frame_weight>& coef, stk_frame_weight* applied, double* ms);
// the weighted fold over the entries of ctx->warpframes under the per-entry records `coef` (weighted.cpp): writes out and
// coverage_out (out's location), adds its device time to *ms
stk_status weighted_fold_records(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, int coverage, stk_image_f32* out,
                                 float* coverage_out, double* ms);
// the pieces of the local-weighted combine (local.cpp) that the mesh folds (mesh.cpp) are built from
stk_status local_validate(stk_ctx* ctx, const stk_local_params* p);
stk_status local_check_border(stk_ctx* ctx, int border_mode, const double* border_value);
stk_status local_maps_enqueue(stk_ctx* ctx, const LocalLayout& L, const std::vector<const void*>& frames, const std::vector<float*>& planes);
stk_status local_maps_launch(stk_ctx* ctx, const LocalLayout& L, size_t first, size_t n, int cn, int w, int h, size_t rb,
                             const stk_local_params* p);
// the field table of a mesh fold, in device memory and indexed like the frame table (null entry: not displaced)
struct MeshFoldArgs { const float* const* fields; int step, gw, gh; };
void mesh_fold_clip_args(const MeshFoldArgs& m, stk::ClipArgs& ca);
// (the fold runs under BORDER_CONSTANT 0 whatever the spec's border: local_check_border)
stk_status local_fold(stk_ctx* ctx, const LocalLayout& L, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, float floor,
                      int power, stk_image_f32* out, float* den_out, double* ms, const MeshFoldArgs* mesh = nullptr);
// stk_local_weighted_stack, and with `fields` (n planes by frame index, in frames->location) stk_mesh_local_weighted_stack
stk_status local_weighted_stack_impl(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                     int32_t border_mode, const double* border_value, double alpha, const stk_frame_weight* per_frame,
                                     const float* const* maps, float floor, int32_t power, const float* const* fields, int32_t step,
                                     stk_image_f32* out, float* den_out);
// the checks of a mesh fold's step and of the fold options it runs under (mesh.cpp)
stk_status mesh_check_fold(stk_ctx* ctx, int step);
// uploads the fields of the table's entries (host planes into ctx->mesh) and their pointer table; frame 0 and an entry
// whose plane is null get no field. Synchronises.
stk_status mesh_fold_table(stk_ctx* ctx, const stk_frames* frames, const EntryTable& table, const float* const* fields, int step,
                           MeshFoldArgs* out);
// the field pass of the whole-stack forms for a combine outside mesh.cpp (drizzle.cpp): the checks of the mesh parameters
// and of the frames' depth; ctx->mesh reserved for frames->n entries; the pass over the n_entries entries of ctx->warpframes
// (entry 0 = frame 0; the table is uploaded), which leaves the fold's field table in *out, synchronises and adds its device
// time to *ms
stk_status mesh_match_fields_check(stk_ctx* ctx, const stk_frames* frames, const stk_mesh_params* mp);
stk_status mesh_match_fields_reserve(stk_ctx* ctx, const stk_frames* frames, const stk_mesh_params* mp);
stk_status mesh_match_fields(stk_ctx* ctx, const stk_frames* frames, int n_entries, int is_affine, const stk_mesh_params* mp,
                             MeshFoldArgs* out, double* ms);
// local normalisation (local_norm.cpp): the plane table of a locally normalised fold, in device memory and indexed like
// the frame table (null entry: the entry's record as constants)
struct NormFoldArgs { const float* const* planes; int step, gw, gh; };
void norm_fold_clip_args(const NormFoldArgs& n, stk::ClipArgs& ca);
// quantile_bands_weighted (robust.cpp) with the locally normalised store launch: same bands, workspaces and selection
stk_status quantile_bands_norm(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, int coverage,
                               const stk_quantile_params* p, const NormFoldArgs& norm, stk_image_f32* out, int32_t* counts, double* ms);
// clip_passes_weighted (robust.cpp) with the locally normalised clip pass: same planes, workspaces and passes
stk_status clip_passes_norm(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, int coverage,
                            const stk_clip_params* p, const NormFoldArgs& norm, stk_image_f32* out, int32_t* counts, float* kept, double* ms);
// rejection maps (reject.cpp) and the pieces of the combines that the rejected drizzle (drizzle.cpp) is built from
stk_status reject_validate(stk_ctx* ctx, const stk_reject_params* p);
stk_status reject_run(stk_ctx* ctx, const RejectLayout& L, const stk_frames* frames, const std::vector<const void*>& dev,
                      const EntryTable& table, int is_affine, double alpha, const std::vector<stk_frame_weight>& coef, const float* clean,
                      const int32_t* counts, const stk_reject_params* p, const std::vector<const float*>& in,
                      const std::vector<float*>& out, int64_t* rejected, int64_t* judged, double* ms);
// after a plain whole-stack call (robust.cpp): the frame table of frame 0 and the kept frames (`table`) into
// ctx->warpframes and the records as stk_*_match_weighted makes them under `spec`; then the coverage-aware median
// (quantile 0.5, coverage 1, BORDER_CONSTANT 0, alpha 1 / 255) of that table with its counts, both device memory. Each adds
// its device time to *ms.
stk_status robust_match_records(stk_ctx* ctx, const stk_frames* frames, const stk_frame_stats* stats, bool keypoint, const FoldSpec& spec,
                                const stk_weight_params* weight, const float* weights, EntryTable& table,
                                std::vector<stk_frame_weight>& coef, stk_frame_weight* applied, double* ms);
stk_status robust_match_median(stk_ctx* ctx, const stk_frames* frames, const std::vector<stk_frame_weight>& coef, int is_affine,
                               float* clean, int32_t* counts, double* ms);
stk_status ecc_shard_impl(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                          int32_t add_reference, stk_image_f32* sum, int32_t* n_added, stk_frame_stats* stats,
                          const float* seeds, double alpha, bool allow16);
// called with consecutive frame ranges [lo, hi) in increasing order, each once, as soon as the results of those frames (and
// of every frame before them) are final — possibly from a helper lane's thread, never from two threads at once
using KpFramesFinal = std::function<stk_status(int lo, int hi)>;
struct KpAlign { bool ok = false; double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; int n_keypoints = 0, n_matches = 0, n_inliers = 0; };
// keypoint_match's alignment half: ORB + 2-NN + ratio / sort / truncate + homography per moving frame (no fold).
// reduce16: 16-bit frames are matched on their 8-bit reduction (g + 128) / 257 (hybrid extension only).
stk_status keypoint_align_impl(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                               bool reduce16, std::vector<KpAlign>& out, int* n_ref_keypoints, std::vector<const void*>& dev,
                               const KpFramesFinal* on_final = nullptr);
