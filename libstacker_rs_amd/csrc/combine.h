// combine.h — the host front end every combine shares (combine.cpp): which frames of a stack are samples and under which
// matrix (EntryTable), the geometry of the fold that samples them (FoldSpec), the upload of the frame table, the unit
// record, two argument checks, and the scaffold of the whole-stack forms (plain call first, then the combine over the
// frames it kept). Included from context.h. The selection rules are inline and touch no HIP type and no stk_ctx, so a
// host-only program can call them (tests/sanitize/entries_harness.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/stacker.h"

namespace stk { struct WarpArgs; }

// ---------------------------------------------------------------------------------------------
// Entry k of a frame table is frame `frame[k]` under the forward matrix `M[k]` (9 doubles, not owned).
struct EntryTable {
    std::vector<int> frame;
    std::vector<const double*> M;
    int size() const { return (int)frame.size(); }
};

// the matrix of frame 0 in the whole-stack forms (one object in the whole library)
inline const double IDENTITY3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

// The caller-held-warps forms: every frame i with !include || include[i], under M + 9 i — frame 0 under its own matrix
// too. Leaves the table empty when nothing is included; the message is the caller's.
inline void entries_from_include(int n, const double* M, const int32_t* include, EntryTable& table) {
    table.frame.clear(); table.M.clear();
    for (int i = 0; i < n; i++) {
        if (include && !include[i]) continue;
        table.frame.push_back(i);
        table.M.push_back(M + 9 * (size_t)i);
    }
}

// The whole-stack forms, from the plain call's stats: frame 0 under the identity, always (its status is not asked); then
// every frame i >= 1 under stats[i].warp. ECC keeps them all (a failed frame fails the plain call); `keypoint` keeps those
// with a homography (status 0), what stk_keypoint_match_shard folded.
inline void entries_from_stats(int n, const stk_frame_stats* stats, bool keypoint, EntryTable& table) {
    table.frame.clear(); table.M.clear();
    for (int i = 0; i < n; i++) {
        if (i > 0 && keypoint && stats[i].status != 0) continue;
        table.frame.push_back(i);
        table.M.push_back(i == 0 ? IDENTITY3 : stats[i].warp);
    }
}

// ---------------------------------------------------------------------------------------------
// What a fold over the frame table needs beside the table: (w, h) is the SOURCE frames' size and the destination's.
struct FoldSpec {
    int depth, w, h, cn;
    size_t src_row_bytes;
    double alpha;
    int border_mode;
    const double* border_value;     // null = 0
    int is_affine;
};
// the caller-held-warps forms: the frames' geometry with the caller's fold parameters
FoldSpec fold_spec(const stk_frames* frames, double alpha, int border_mode, const double* border_value, int is_affine);
// the whole-stack forms fold as the plain call did. ECC: the frames' depth, alpha 1 / 255, BORDER_CONSTANT 0, affine unless
// the motion is a homography. Keypoint: depth 8, alpha 1 / 255, the params' border, never affine.
FoldSpec fold_spec_ecc(const stk_frames* frames, const stk_ecc_params* params);
FoldSpec fold_spec_keypoint(const stk_frames* frames, const stk_keypoint_params* params);
// the kernels' argument block over the first n_entries entries of ctx->warpframes, no accumulator (the only place in the
// combines that fills one)
stk::WarpArgs fold_warp_args(stk_ctx* ctx, int n_entries, const FoldSpec& spec);

// The table into ctx->warpframes with the flags for the frames' own w x h destination; dev: the frames by frame index.
// Synchronises: on return no host vector has to outlive anything.
stk_status entry_table_upload(stk_ctx* ctx, const stk_frames* frames, const std::vector<const void*>& dev, const EntryTable& table,
                              int is_affine);
// the opening of a caller-held-warps form once its arguments are checked: the context's device, the call's timing, host
// frames uploaded, then entry_table_upload
stk_status entry_table_begin(stk_ctx* ctx, const stk_frames* frames, const EntryTable& table, int is_affine);

// gains 1, offsets 0, weight 1, no flags
stk_frame_weight unit_record();
// coef[k] = the record of the table's entry k: per_frame by frame index, or (null) the unit record
void gather_records(const EntryTable& table, const stk_frame_weight* per_frame, std::vector<stk_frame_weight>& coef);

stk_status check_border_mode(stk_ctx* ctx, int border_mode);
// an output of the frames' geometry, tightly packed
stk_status combine_check_out(stk_ctx* ctx, const stk_image_f32* out, const stk_frames* frames);

// ---------------------------------------------------------------------------------------------
// The whole-stack forms, after the caller has checked its arguments and reserved its workspace. Supplies `stats` when
// null; runs the plain call on this context's own device with its mean into `mean` (w x h x cn f32 of device memory; the
// mean is not used); the frames are then still resident in HBM (device stacks in place, host-fed stacks in ctx->frames), so
// nothing is uploaded again. Builds the table of the kept frames, uploads it, and calls `finish` with the table, the frames
// by frame index, the plain call's fold and the stats; `finish` adds its device time to *ms. The timing stays the plain
// call's but for finalize_ms: *ms, or 0 when the combine failed.
using CombineFinish = std::function<stk_status(const EntryTable& table, const std::vector<const void*>& dev, const FoldSpec& spec,
                                               const stk_frame_stats* stats, double* ms)>;
stk_status ecc_match_then(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width, float* mean,
                          stk_frame_stats* stats, const CombineFinish& finish);
stk_status keypoint_match_then(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                               float* mean, int32_t* dropped, stk_frame_stats* stats, const CombineFinish& finish);
