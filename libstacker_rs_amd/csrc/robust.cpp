// robust.cpp — normalised, coverage-aware rejection: stk_clip_stack_weighted, stk_quantile_stack_weighted,
// stk_robust_clip_stack_weighted and the *_clipped_weighted / *_quantile_weighted / *_robust_clipped_weighted whole-stack
// forms (an extension beyond the reference; definition in include/stacker.h, kernels in kernels_clip.hip,
// kernels_quantile.hip and kernels_robust_clip.hip; the median / MAD clip's combine itself is robust_clip.cpp's).
// The rejection combines with the per-entry gain / offset / weight records and the coverage flag of the weighted
// mean: an entry is a sample of a pixel only if its weight is > 0 and (coverage = 1) the frame covers the pixel, and the
// samples are compared after each frame has been mapped onto frame 0's level. The workspaces are the plain combines'
// (ctx->clip: the c, L and U planes; ctx->quantile: an image, then the band); the record table lives in ctx->coef. The
// whole-stack forms run the plain call first, like clip.cpp (combine.h's scaffold), then the moments pass and the estimator
// of weighted.cpp (weighted_match_records) when normalize != 0, then the combine.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

namespace {

stk_status robust_check_border(stk_ctx* ctx, int border_mode, int coverage) {
    stk_status st = check_border_mode(ctx, border_mode);
    if (st) return st;
    if (coverage < 0 || coverage > 1) return fail(ctx, STK_INVALID_PARAMS, "weighted: coverage must be 0 or 1");
    return STK_OK;
}

// the record table into ctx->coef (asynchronous: `coef` must outlive the copy)
stk_status coef_upload(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef) {
    stk_status st = workspace_reserve(ctx, ctx->coef, coef.size() * sizeof(stk_frame_weight), "record table");
    return st ? st : records_upload(ctx, ctx->coef.p, coef);
}

// The weighted clip over the entries of ctx->warpframes with the records `coef`: the centre pass, then iterations + 1
// passes. Writes `out`, `counts` and `kept` (out's location); adds its device time to *ms. norm: the locally normalised clip
// (local_norm.cpp): the same planes and passes through its plane table.
stk_status clip_passes_weighted(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, int coverage,
                                const stk_clip_params* p, stk_image_f32* out, int32_t* counts, float* kept, double* ms,
                                const NormFoldArgs* norm = nullptr) {
    const int w = spec.w, cn = spec.cn, depth = spec.depth;
    const size_t nel = (size_t)w * spec.h * cn;
    const ClipLayout L = clip_layout(nel);
    stk_status st = workspace_reserve(ctx, ctx->clip, L.total, "sigma clipping");
    if (st) return st;
    char* base = ctx->clip.as<char>();
    const WarpArgs a = fold_warp_args(ctx, (int)coef.size(), spec);
    if ((st = coef_upload(ctx, coef))) return st;
    ClipArgs ca{};
    ca.c = (float*)(base + L.c); ca.L = (float*)(base + L.L); ca.U = (float*)(base + L.U);
    ca.plane_stride = (size_t)w * cn;
    // a host output goes through the planes themselves: each thread reads its c, L, U before it writes out / counts / kept
    const CombineOutputs o(out, ca.c, nel, {counts, ca.L, nel}, {kept, ca.U, nel});
    ca.out = o.image();
    ca.out_stride = (size_t)w * cn;
    ca.counts = o.side<int>(0);
    ca.kept = o.side<float>(1);
    ca.kappa_low = p->kappa_low; ca.kappa_high = p->kappa_high;
    ca.coef = ctx->coef.as<stk_frame_weight>();
    ca.coverage = coverage;
    if (norm) norm_fold_clip_args(*norm, ca);
    const auto launch_pass = norm ? launch_clip_pass_norm : launch_clip_pass_weighted;
    if ((st = combine_begin(ctx))) return st;
    ca.centre = 1; ca.first = 1; ca.last = 0;
    HIP_TRY(launch_pass(a, ca, depth, ctx->stream));
    ca.centre = 0;
    for (int t = 1; t <= p->iterations + 1; t++) {
        ca.first = t == 1;
        ca.last = t == p->iterations + 1;
        HIP_TRY(launch_pass(a, ca, depth, ctx->stream));
    }
    return combine_end(ctx, ms, &o);
}

// The quantile with participation over the entries of ctx->warpframes: per band a store launch (normalised samples and
// absent marks), then the selection with a per-pixel rank. `counts` (w x h, out's location) is optional.
stk_status quantile_bands_weighted(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, int coverage,
                                   const stk_quantile_params* p, stk_image_f32* out, int32_t* counts, double* ms,
                                   const NormFoldArgs* norm = nullptr) {
    const int n_entries = (int)coef.size(), w = spec.w, h = spec.h, cn = spec.cn, depth = spec.depth;
    stk_status st = quantile_check_count(ctx, n_entries);
    if (st) return st;
    const size_t R = quantile_band_rows(ctx, n_entries, w, h, cn), row = (size_t)w * cn;
    QuantileLayout L;
    if ((st = quantile_reserve(ctx, n_entries, w, h, cn, out->location != STK_DEVICE && counts, &L))) return st;
    char* base = ctx->quantile.as<char>();
    float* band = (float*)(base + L.band);
    const CombineOutputs o(out, (float*)(base + L.image), (size_t)h * row, {counts, base + L.counts, (size_t)w * h});
    float* dst = o.image();
    int* cdst = o.side<int>(0);
    WarpArgs a = fold_warp_args(ctx, n_entries, spec);
    if ((st = coef_upload(ctx, coef))) return st;
    ClipArgs ca{};
    ca.band = band;
    ca.plane_stride = row;
    ca.coef = ctx->coef.as<stk_frame_weight>();
    ca.coverage = coverage;
    if (norm) norm_fold_clip_args(*norm, ca);        // the locally normalised quantile (local_norm.cpp): the same bands, its own store launch
    if ((st = combine_begin(ctx))) return st;
    for (size_t y0 = 0; y0 < (size_t)h; y0 += R) {
        const size_t rows = std::min(R, (size_t)h - y0);
        ca.y0 = (int)y0; ca.band_rows = (int)rows;
        a.dh = (int)(y0 + rows);
        if (norm) HIP_TRY(launch_norm_store(a, ca, depth, ctx->stream));
        else HIP_TRY(launch_quantile_store_weighted(a, ca, depth, ctx->stream));
        HIP_TRY(launch_quantile_select_masked(band, rows * row, n_entries, p->quantile, cn, dst + y0 * row,
                                              cdst ? cdst + y0 * (size_t)w : nullptr, ctx->stream));
    }
    return combine_end(ctx, ms, &o);
}

int count_included(const stk_frames* frames, const int32_t* include) {
    int n_in = 0;
    for (int i = 0; i < frames->n; i++) n_in += (!include || include[i]) ? 1 : 0;
    return n_in;
}

// the caller-held-warps forms: the last argument checks, the records of the included frames, the frame table
stk_status robust_stack_begin(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int is_affine,
                              const stk_frame_weight* per_frame, const char* what, std::vector<stk_frame_weight>& coef) {
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (!per_frame) return fail(ctx, STK_INVALID_PARAMS, "null per-frame records");
    EntryTable table;
    entries_from_include(frames->n, M, include, table);
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, std::string(what) + ": no frame included");
    gather_records(table, per_frame, coef);
    stk_status st = weighted_check_coefs(ctx, coef, frames->channels);
    if (st) return st;
    return entry_table_begin(ctx, frames, table, is_affine);
}

struct RobustCombine {
    const stk_clip_params* clip = nullptr;            // exactly one of the three
    const stk_quantile_params* quantile = nullptr;
    const stk_robust_clip_params* mad = nullptr;      // the median / MAD clip (robust_clip.cpp)
    int32_t* counts = nullptr;
    float* kept = nullptr;
};

stk_status robust_validate(stk_ctx* ctx, const RobustCombine& rc, const stk_weight_params* weight, const stk_frames* frames,
                           const stk_image_f32* out) {
    stk_status st = rc.clip ? clip_validate(ctx, rc.clip) : rc.mad ? robust_clip_validate(ctx, rc.mad) : quantile_validate(ctx, rc.quantile);
    if (st) return st;
    if ((st = weighted_validate(ctx, weight))) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    if (!rc.clip && (st = quantile_check_count(ctx, frames->n))) return st;
    return STK_OK;
}

// the combine's workspace image, which takes the plain call's mean (unused)
stk_status robust_reserve(stk_ctx* ctx, const RobustCombine& rc, const stk_frames* frames, float** mean) {
    (void)hipSetDevice(ctx->device);
    const int w = frames->width, h = frames->height, cn = frames->channels;
    const bool planes = rc.clip || rc.mad;
    if (stk_status st = planes ? workspace_reserve(ctx, ctx->clip, clip_layout((size_t)w * h * cn).total, "sigma clipping")
                               : quantile_reserve(ctx, 0, w, h, cn, false, nullptr))
        return st;
    *mean = planes ? ctx->clip.as<float>() : ctx->quantile.as<float>();
    return STK_OK;
}

// the combine of the whole-stack forms over the kept frames: records, then the combine; finalize_ms = moments + combine
CombineFinish robust_finish(stk_ctx* ctx, int n, const stk_weight_params* weight, const float* weights, const RobustCombine& rc,
                            stk_image_f32* out, stk_frame_weight* applied) {
    return [=](const EntryTable& table, const std::vector<const void*>&, const FoldSpec& spec, const stk_frame_stats*, double* ms) {
        std::vector<stk_frame_weight> coef;
        stk_status st = weighted_match_records(ctx, n, table, spec, weight, weights, coef, applied, ms);
        if (st) return st;
        if (rc.clip) return clip_passes_weighted(ctx, coef, spec, weight->coverage, rc.clip, out, rc.counts, rc.kept, ms);
        if (rc.mad) return robust_clip_bands(ctx, (int)coef.size(), &coef, spec, weight->coverage, rc.mad, out, rc.counts, rc.kept, ms);
        return quantile_bands_weighted(ctx, coef, spec, weight->coverage, rc.quantile, out, rc.counts, ms);
    };
}

stk_status robust_ecc(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                      const stk_weight_params* weight, const float* weights, const RobustCombine& rc, stk_image_f32* out,
                      stk_frame_weight* applied, stk_frame_stats* stats) {
    stk_status st = robust_validate(ctx, rc, weight, frames, out);
    if (st) return st;
    float* mean = nullptr;
    if ((st = robust_reserve(ctx, rc, frames, &mean))) return st;
    return ecc_match_then(ctx, frames, params, scale_down_width, mean, stats, robust_finish(ctx, frames->n, weight, weights, rc, out, applied));
}

stk_status robust_keypoint(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                           const stk_weight_params* weight, const float* weights, const RobustCombine& rc, stk_image_f32* out,
                           int32_t* dropped, stk_frame_weight* applied, stk_frame_stats* stats) {
    stk_status st = robust_validate(ctx, rc, weight, frames, out);
    if (st) return st;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null parameters");
    float* mean = nullptr;
    if ((st = robust_reserve(ctx, rc, frames, &mean))) return st;
    return keypoint_match_then(ctx, frames, params, scale_down_width, mean, dropped, stats,
                               robust_finish(ctx, frames->n, weight, weights, rc, out, applied));
}

}  // namespace

// (shared with drizzle.cpp: context.h)
stk_status robust_match_records(stk_ctx* ctx, const stk_frames* frames, const stk_frame_stats* stats, bool keypoint, const FoldSpec& spec,
                                const stk_weight_params* weight, const float* weights, EntryTable& table,
                                std::vector<stk_frame_weight>& coef, stk_frame_weight* applied, double* ms) {
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    entries_from_stats(frames->n, stats, keypoint, table);
    stk_status st = entry_table_upload(ctx, frames, dev, table, spec.is_affine);
    if (st) return st;
    return weighted_match_records(ctx, frames->n, table, spec, weight, weights, coef, applied, ms);
}

stk_status quantile_bands_norm(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, int coverage,
                               const stk_quantile_params* p, const NormFoldArgs& norm, stk_image_f32* out, int32_t* counts, double* ms) {
    return quantile_bands_weighted(ctx, coef, spec, coverage, p, out, counts, ms, &norm);
}

stk_status clip_passes_norm(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, int coverage,
                            const stk_clip_params* p, const NormFoldArgs& norm, stk_image_f32* out, int32_t* counts, float* kept, double* ms) {
    return clip_passes_weighted(ctx, coef, spec, coverage, p, out, counts, kept, ms, &norm);
}

stk_status robust_match_median(stk_ctx* ctx, const stk_frames* frames, const std::vector<stk_frame_weight>& coef, int is_affine,
                               float* clean, int32_t* counts, double* ms) {
    const stk_quantile_params qp{0.5f, 0};
    stk_image_f32 img{clean, frames->width, frames->height, frames->channels, STK_DEVICE, 0};
    return quantile_bands_weighted(ctx, coef, fold_spec(frames, 1.0 / 255.0, STK_BORDER_CONSTANT, nullptr, is_affine), 1, &qp, &img, counts, ms);
}

extern "C" {

stk_status stk_clip_stack_weighted(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                   int32_t border_mode, const double* border_value, double alpha, const stk_clip_params* clip,
                                   const stk_frame_weight* per_frame, int32_t coverage, stk_image_f32* out, int32_t* counts,
                                   float* kept_weight) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if ((st = robust_check_border(ctx, border_mode, coverage))) return st;
    if ((st = clip_validate(ctx, clip))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    std::vector<stk_frame_weight> coef;
    if ((st = robust_stack_begin(ctx, frames, M, include, is_affine, per_frame, "sigma clipping", coef))) return st;
    double ms = 0.0;
    st = clip_passes_weighted(ctx, coef, fold_spec(frames, alpha, border_mode, border_value, is_affine), coverage, clip, out, counts,
                              kept_weight, &ms);
    ctx->timing.finalize_ms = st ? 0.0 : ms;
    return st;
}

stk_status stk_quantile_stack_weighted(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include,
                                       int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                       const stk_quantile_params* quantile, const stk_frame_weight* per_frame, int32_t coverage,
                                       stk_image_f32* out, int32_t* counts) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if ((st = robust_check_border(ctx, border_mode, coverage))) return st;
    if ((st = quantile_validate(ctx, quantile))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    if ((st = quantile_check_count(ctx, count_included(frames, include)))) return st;
    std::vector<stk_frame_weight> coef;
    if ((st = robust_stack_begin(ctx, frames, M, include, is_affine, per_frame, "quantile", coef))) return st;
    double ms = 0.0;
    st = quantile_bands_weighted(ctx, coef, fold_spec(frames, alpha, border_mode, border_value, is_affine), coverage, quantile, out, counts, &ms);
    ctx->timing.finalize_ms = st ? 0.0 : ms;
    return st;
}

stk_status stk_robust_clip_stack_weighted(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include,
                                          int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                          const stk_robust_clip_params* clip, const stk_frame_weight* per_frame, int32_t coverage,
                                          stk_image_f32* out, int32_t* counts, float* kept_weight) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if ((st = robust_check_border(ctx, border_mode, coverage))) return st;
    if ((st = robust_clip_validate(ctx, clip))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    if ((st = quantile_check_count(ctx, count_included(frames, include)))) return st;
    std::vector<stk_frame_weight> coef;
    if ((st = robust_stack_begin(ctx, frames, M, include, is_affine, per_frame, "robust clipping", coef))) return st;
    double ms = 0.0;
    st = robust_clip_bands(ctx, (int)coef.size(), &coef, fold_spec(frames, alpha, border_mode, border_value, is_affine), coverage, clip, out,
                           counts, kept_weight, &ms);
    ctx->timing.finalize_ms = st ? 0.0 : ms;
    return st;
}

stk_status stk_ecc_match_robust_clipped_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                                 float scale_down_width, const stk_robust_clip_params* clip,
                                                 const stk_weight_params* weight, const float* weights, stk_image_f32* out,
                                                 int32_t* counts, float* kept_weight, stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!clip) return fail(ctx, STK_INVALID_PARAMS, "null robust clip parameters");
    RobustCombine rc;
    rc.mad = clip; rc.counts = counts; rc.kept = kept_weight;
    return robust_ecc(ctx, frames, params, scale_down_width, weight, weights, rc, out, applied, stats);
}

stk_status stk_keypoint_match_robust_clipped_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                                      float scale_down_width, const stk_robust_clip_params* clip,
                                                      const stk_weight_params* weight, const float* weights, stk_image_f32* out,
                                                      int32_t* dropped, int32_t* counts, float* kept_weight,
                                                      stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!clip) return fail(ctx, STK_INVALID_PARAMS, "null robust clip parameters");
    RobustCombine rc;
    rc.mad = clip; rc.counts = counts; rc.kept = kept_weight;
    return robust_keypoint(ctx, frames, params, scale_down_width, weight, weights, rc, out, dropped, applied, stats);
}

stk_status stk_ecc_match_clipped_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                          const stk_clip_params* clip, const stk_weight_params* weight, const float* weights,
                                          stk_image_f32* out, int32_t* counts, float* kept_weight, stk_frame_weight* applied,
                                          stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!clip) return fail(ctx, STK_INVALID_PARAMS, "null clip parameters");
    RobustCombine rc;
    rc.clip = clip; rc.counts = counts; rc.kept = kept_weight;
    return robust_ecc(ctx, frames, params, scale_down_width, weight, weights, rc, out, applied, stats);
}

stk_status stk_keypoint_match_clipped_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                               float scale_down_width, const stk_clip_params* clip, const stk_weight_params* weight,
                                               const float* weights, stk_image_f32* out, int32_t* dropped, int32_t* counts,
                                               float* kept_weight, stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!clip) return fail(ctx, STK_INVALID_PARAMS, "null clip parameters");
    RobustCombine rc;
    rc.clip = clip; rc.counts = counts; rc.kept = kept_weight;
    return robust_keypoint(ctx, frames, params, scale_down_width, weight, weights, rc, out, dropped, applied, stats);
}

stk_status stk_ecc_match_quantile_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                           const stk_quantile_params* quantile, const stk_weight_params* weight, const float* weights,
                                           stk_image_f32* out, int32_t* counts, stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!quantile) return fail(ctx, STK_INVALID_PARAMS, "null quantile parameters");
    RobustCombine rc;
    rc.quantile = quantile; rc.counts = counts;
    return robust_ecc(ctx, frames, params, scale_down_width, weight, weights, rc, out, applied, stats);
}

stk_status stk_keypoint_match_quantile_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                                float scale_down_width, const stk_quantile_params* quantile,
                                                const stk_weight_params* weight, const float* weights, stk_image_f32* out,
                                                int32_t* dropped, int32_t* counts, stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!quantile) return fail(ctx, STK_INVALID_PARAMS, "null quantile parameters");
    RobustCombine rc;
    rc.quantile = quantile; rc.counts = counts;
    return robust_keypoint(ctx, frames, params, scale_down_width, weight, weights, rc, out, dropped, applied, stats);
}

}  // extern "C"
