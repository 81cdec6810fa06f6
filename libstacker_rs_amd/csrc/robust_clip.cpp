// robust_clip.cpp — median / MAD sigma clipping: stk_robust_clip_stack, stk_ecc_match_robust_clipped,
// stk_keypoint_match_robust_clipped (an extension beyond the reference; definition in include/stacker.h, the selection
// kernel in kernels_robust_clip.hip) and robust_clip_bands, the combine itself, which the participation forms of
// robust.cpp share.
// The centre and the scale are order statistics, so the samples go band by band through the quantile combine's buffer
// (ctx->quantile, here the band alone; quantile.cpp's band geometry and option quantile_band_rows): per band the fold
// kernel in its store mode, then the selection, which writes c, L and U of the band's rows into the clipped combine's
// planes (ctx->clip). When every band has filled its rows, one last clip pass over the whole frame sums the kept samples in
// fold order: the output is the clipped combine's sequential sum, with no summation order of its own. Like clip.cpp, the
// whole-stack forms run the plain call first (its mean lands in the c plane and is overwritten) and take the warps and
// the kept set from its stats (combine.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

stk_status robust_clip_validate(stk_ctx* ctx, const stk_robust_clip_params* p) {
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null robust clip parameters");
    if (!(p->kappa_low > 0.0f) || !std::isfinite(p->kappa_low) || !(p->kappa_high > 0.0f) || !std::isfinite(p->kappa_high))
        return fail(ctx, STK_INVALID_PARAMS, "robust clipping: kappa_low and kappa_high must be finite and > 0");
    if (!(p->sigma_floor >= 0.0f) || !std::isfinite(p->sigma_floor))
        return fail(ctx, STK_INVALID_PARAMS, "robust clipping: sigma_floor must be finite and >= 0");
    if (p->iterations < 1 || p->iterations > 16)
        return fail(ctx, STK_INVALID_PARAMS, "robust clipping: iterations must be 1 .. 16, got " + std::to_string(p->iterations));
    return STK_OK;
}

stk_status robust_clip_bands(stk_ctx* ctx, int n_entries, const std::vector<stk_frame_weight>* coef, const FoldSpec& spec, int coverage,
                             const stk_robust_clip_params* p, stk_image_f32* out, int32_t* counts, float* kept, double* ms,
                             const NormFoldArgs* norm) {
    if (norm && !coef) return fail(ctx, STK_INVALID_PARAMS, "robust clipping: a plane table needs the record table");
    const int w = spec.w, h = spec.h, cn = spec.cn, depth = spec.depth;
    stk_status st = quantile_check_count(ctx, n_entries);
    if (st) return st;
    const size_t row = (size_t)w * cn, nel = row * h;
    const size_t R = quantile_band_rows(ctx, n_entries, w, h, cn);
    const ClipLayout L = clip_layout(nel);
    if ((st = workspace_reserve(ctx, ctx->clip, L.total, "robust clipping"))) return st;
    if ((st = workspace_reserve(ctx, ctx->quantile, R * n_entries * row * sizeof(float), "robust clipping band"))) return st;
    char* base = ctx->clip.as<char>();
    float* band = ctx->quantile.as<float>();
    WarpArgs a = fold_warp_args(ctx, n_entries, spec);
    ClipArgs ca{};
    ca.c = (float*)(base + L.c); ca.L = (float*)(base + L.L); ca.U = (float*)(base + L.U);
    ca.plane_stride = row;
    // a host output goes through the planes themselves, as in clip.cpp: the last pass reads c, L, U before it writes there
    const CombineOutputs o(out, ca.c, nel, {counts, ca.L, nel}, {coef ? kept : nullptr, ca.U, nel});
    ca.out = o.image();
    ca.out_stride = row;
    ca.counts = o.side<int>(0);
    ca.kept = o.side<float>(1);
    ca.kappa_low = p->kappa_low; ca.kappa_high = p->kappa_high;
    ca.band = band;
    if (coef) {
        if ((st = workspace_reserve(ctx, ctx->coef, coef->size() * sizeof(stk_frame_weight), "record table"))) return st;
        if ((st = records_upload(ctx, ctx->coef.p, *coef))) return st;
        ca.coef = ctx->coef.as<stk_frame_weight>();
        ca.coverage = coverage;
    }
    if (norm) norm_fold_clip_args(*norm, ca);        // the locally normalised form (local_norm.cpp): its own store launch and last pass
    const size_t n_bands = ((size_t)h + R - 1) / R;
    while (ctx->select_ev.size() < n_bands) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
        ctx->select_ev.emplace_back(e0, e1);
    }
    if ((st = combine_begin(ctx))) return st;
    size_t b = 0;
    for (size_t y0 = 0; y0 < (size_t)h; y0 += R, b++) {
        const size_t rows = std::min(R, (size_t)h - y0);
        ca.y0 = (int)y0; ca.band_rows = (int)rows;
        a.dh = (int)(y0 + rows);
        HIP_TRY(norm   ? launch_norm_store(a, ca, depth, ctx->stream)
                : coef ? launch_quantile_store_weighted(a, ca, depth, ctx->stream)
                       : launch_quantile_store(a, ca, depth, ctx->stream));
        HIP_TRY(hipEventRecord(ctx->select_ev[b].first, ctx->stream));
        HIP_TRY(launch_robust_select(band, rows * row, n_entries, coef ? 1 : 0, *p, ca.c + y0 * row, ca.L + y0 * row, ca.U + y0 * row,
                                     ctx->stream));
        HIP_TRY(hipEventRecord(ctx->select_ev[b].second, ctx->stream));
    }
    // the planes are complete: the last pass of the (weighted) clip over the whole frame
    a.dh = h;
    ca.first = 0; ca.last = 1; ca.centre = 0;
    HIP_TRY(norm   ? launch_clip_pass_norm(a, ca, depth, ctx->stream)
            : coef ? launch_clip_pass_weighted(a, ca, depth, ctx->stream)
                   : launch_clip_pass(a, ca, depth, ctx->stream));
    if ((st = combine_end(ctx, ms, &o))) return st;
    double sel = 0.0;
    for (size_t k = 0; k < n_bands; k++) sel += ev_ms(ctx->select_ev[k].first, ctx->select_ev[k].second);
    ctx->robust_select_us = (int64_t)std::llround(sel * 1000.0);
    return STK_OK;
}

namespace {

// the checks and the workspace of the two whole-stack forms: the plain call's mean lands in the c plane (unused: the
// selection overwrites it)
stk_status robust_clip_match_begin(stk_ctx* ctx, const stk_frames* frames, const stk_robust_clip_params* clip, const stk_image_f32* out) {
    stk_status st = robust_clip_validate(ctx, clip);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    if ((st = quantile_check_count(ctx, frames->n))) return st;
    (void)hipSetDevice(ctx->device);
    return workspace_reserve(ctx, ctx->clip, clip_layout((size_t)frames->width * frames->height * frames->channels).total, "robust clipping");
}

// and their combine over the kept frames
CombineFinish robust_clip_match_finish(stk_ctx* ctx, const stk_robust_clip_params* clip, stk_image_f32* out, int32_t* counts) {
    return [=](const EntryTable& table, const std::vector<const void*>&, const FoldSpec& spec, const stk_frame_stats*, double* ms) {
        return robust_clip_bands(ctx, table.size(), nullptr, spec, 0, clip, out, counts, nullptr, ms);
    };
}

}  // namespace

extern "C" {

stk_status stk_robust_clip_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                 int32_t border_mode, const double* border_value, double alpha, const stk_robust_clip_params* clip,
                                 stk_image_f32* out, int32_t* counts) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if ((st = check_border_mode(ctx, border_mode))) return st;
    if ((st = robust_clip_validate(ctx, clip))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    EntryTable table;
    entries_from_include(frames->n, M, include, table);
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "robust clipping: no frame included");
    if ((st = quantile_check_count(ctx, table.size()))) return st;
    if ((st = entry_table_begin(ctx, frames, table, is_affine))) return st;
    double ms = 0.0;
    st = robust_clip_bands(ctx, table.size(), nullptr, fold_spec(frames, alpha, border_mode, border_value, is_affine), 0, clip, out, counts,
                           nullptr, &ms);
    ctx->timing.finalize_ms = st ? 0.0 : ms;
    return st;
}

stk_status stk_ecc_match_robust_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                        const stk_robust_clip_params* clip, stk_image_f32* out, int32_t* counts,
                                        stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = robust_clip_match_begin(ctx, frames, clip, out);
    if (st) return st;
    return ecc_match_then(ctx, frames, params, scale_down_width, ctx->clip.as<float>(), stats,
                          robust_clip_match_finish(ctx, clip, out, counts));
}

stk_status stk_keypoint_match_robust_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                             float scale_down_width, const stk_robust_clip_params* clip, stk_image_f32* out,
                                             int32_t* dropped, int32_t* counts, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = robust_clip_match_begin(ctx, frames, clip, out);
    if (st) return st;
    return keypoint_match_then(ctx, frames, params, scale_down_width, ctx->clip.as<float>(), dropped, stats,
                               robust_clip_match_finish(ctx, clip, out, counts));
}

}  // extern "C"
