// clip.cpp — sigma-clipped stacking: stk_clip_stack, stk_ecc_match_clipped, stk_keypoint_match_clipped (an extension
// beyond the reference; definition in include/stacker.h, kernels in kernels_clip.hip).
// The combine starts from the plain mean c and runs iterations + 1 passes over the frames the fold added, each pass one
// launch of the fold kernel in its clip mode reading and rewriting the c / L / U planes (ctx->clip, 3 x 4 B per pixel and
// channel: 300 MB at 4K BGR, grow-only like the other workspaces). The whole-stack forms run the plain call first — its
// output IS c — and take the warps and the kept set from its stats; the frames are still resident in HBM (device stacks
// in place, host-fed stacks in ctx->frames where the upload left them), so nothing is uploaded again. That sequence, the
// frame table and the fold's geometry are combine.h's (ecc_match_then / keypoint_match_then, EntryTable, FoldSpec), shared
// by every combine.
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

// (shared with robust.cpp: context.h)
stk_status clip_validate(stk_ctx* ctx, const stk_clip_params* p) {
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null clip parameters");
    if (!(p->kappa_low > 0.0f) || !std::isfinite(p->kappa_low) || !(p->kappa_high > 0.0f) || !std::isfinite(p->kappa_high))
        return fail(ctx, STK_INVALID_PARAMS, "sigma clipping: kappa_low and kappa_high must be finite and > 0");
    if (p->iterations < 1 || p->iterations > 16)
        return fail(ctx, STK_INVALID_PARAMS, "sigma clipping: iterations must be 1 .. 16, got " + std::to_string(p->iterations));
    return STK_OK;
}

namespace {

// The clip passes over the n_frames entries of ctx->warpframes; the c plane (ctx->clip) holds the plain mean. Writes `out`
// and `counts` (out's location); adds the passes' device time to *ms.
stk_status clip_passes(stk_ctx* ctx, int n_frames, const FoldSpec& spec, const stk_clip_params* p, stk_image_f32* out, int32_t* counts,
                       double* ms) {
    const int w = spec.w, cn = spec.cn, depth = spec.depth;
    const size_t nel = (size_t)w * spec.h * cn;
    const ClipLayout L = clip_layout(nel);
    char* base = ctx->clip.as<char>();
    const WarpArgs a = fold_warp_args(ctx, n_frames, spec);
    ClipArgs ca{};
    ca.c = (float*)(base + L.c); ca.L = (float*)(base + L.L); ca.U = (float*)(base + L.U);
    ca.plane_stride = (size_t)w * cn;
    // a host output goes through the planes themselves: each thread reads its c, L, U before it writes out / counts there
    const CombineOutputs o(out, ca.c, nel, {counts, ca.L, nel});
    ca.out = o.image();
    ca.out_stride = (size_t)w * cn;
    ca.counts = o.side<int>(0);
    ca.kappa_low = p->kappa_low; ca.kappa_high = p->kappa_high;
    if (stk_status st = combine_begin(ctx)) return st;
    for (int t = 1; t <= p->iterations + 1; t++) {
        ca.first = t == 1;
        ca.last = t == p->iterations + 1;
        HIP_TRY(launch_clip_pass(a, ca, depth, ctx->stream));
    }
    return combine_end(ctx, ms, &o);
}

// the checks and the workspace of the two whole-stack forms: the plain call writes its mean straight into the c plane
stk_status clip_match_begin(stk_ctx* ctx, const stk_frames* frames, const stk_clip_params* clip, const stk_image_f32* out) {
    stk_status st = clip_validate(ctx, clip);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    (void)hipSetDevice(ctx->device);
    return workspace_reserve(ctx, ctx->clip, clip_layout((size_t)frames->width * frames->height * frames->channels).total, "sigma clipping");
}

// and their combine over the kept frames
CombineFinish clip_match_finish(stk_ctx* ctx, const stk_clip_params* clip, stk_image_f32* out, int32_t* counts) {
    return [=](const EntryTable& table, const std::vector<const void*>&, const FoldSpec& spec, const stk_frame_stats*, double* ms) {
        return clip_passes(ctx, table.size(), spec, clip, out, counts, ms);
    };
}

}  // namespace

extern "C" {

stk_status stk_clip_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                          int32_t border_mode, const double* border_value, double alpha, const stk_clip_params* clip,
                          stk_image_f32* out, int32_t* counts) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if ((st = check_border_mode(ctx, border_mode))) return st;
    if ((st = clip_validate(ctx, clip))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    EntryTable table;
    entries_from_include(frames->n, M, include, table);
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "sigma clipping: no frame included");
    if ((st = entry_table_begin(ctx, frames, table, is_affine))) return st;
    const FoldSpec spec = fold_spec(frames, alpha, border_mode, border_value, is_affine);
    const size_t nel = (size_t)spec.w * spec.h * spec.cn;
    if ((st = workspace_reserve(ctx, ctx->clip, clip_layout(nel).total, "sigma clipping"))) return st;
    // c = the plain mean: the fold, then stk_finalize_mean's scale
    float* c = ctx->clip.as<float>();
    HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
    if ((st = warp_fold_enqueue(ctx, table.size(), spec.depth, spec.w, spec.h, spec.cn, spec.src_row_bytes, spec.alpha, spec.border_mode,
                                spec.border_value, spec.is_affine, c, (size_t)spec.w * spec.cn, 0)))
        return st;
    HIP_TRY(launch_scale(c, c, nel, (float)(1.0 / (double)table.size()), ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));
    double ms = 0.0;
    if ((st = clip_passes(ctx, table.size(), spec, clip, out, counts, &ms))) return st;
    ctx->timing.finalize_ms = ms;
    ctx->timing.warp_ms = ev_ms(ctx->ev[2], ctx->ev[3]);
    return STK_OK;
}

stk_status stk_ecc_match_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                 const stk_clip_params* clip, stk_image_f32* out, int32_t* counts, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = clip_match_begin(ctx, frames, clip, out);
    if (st) return st;
    return ecc_match_then(ctx, frames, params, scale_down_width, ctx->clip.as<float>(), stats, clip_match_finish(ctx, clip, out, counts));
}

stk_status stk_keypoint_match_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                                      const stk_clip_params* clip, stk_image_f32* out, int32_t* dropped, int32_t* counts,
                                      stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = clip_match_begin(ctx, frames, clip, out);
    if (st) return st;
    return keypoint_match_then(ctx, frames, params, scale_down_width, ctx->clip.as<float>(), dropped, stats,
                               clip_match_finish(ctx, clip, out, counts));
}

}  // extern "C"

