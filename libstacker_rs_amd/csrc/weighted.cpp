// weighted.cpp — weighted, coverage-aware stacking with per-frame normalisation: stk_weighted_stack, stk_overlap_moments,
// stk_ecc_match_weighted, stk_keypoint_match_weighted (an extension beyond the reference; definition in
// include/stacker.h, kernels in kernels_weighted.hip).
// ctx->weighted (grow-only like the other workspaces) holds a w x h x cn f32 image (the plain call's mean in the
// whole-stack forms, then a host output's staging copy), the w x h den plane, the per-entry gain / offset / weight table,
// the moments and the per-wave partials they are reduced from. Like clip.cpp, the whole-stack forms run the plain call
// first and take the warps and the kept set from its stats (combine.h); the frames are still resident in HBM. With
// normalize != 0 the moments pass and the host estimator follow (weighted_match_records, which every whole-stack form with
// stk_weight_params shares), then one weighted fold.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

// (the checks, the moments pass and the estimator are shared with robust.cpp: context.h)
stk_status weighted_validate(stk_ctx* ctx, const stk_weight_params* p) {
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null weight parameters");
    if (p->normalize < 0 || p->normalize > 3) return fail(ctx, STK_INVALID_PARAMS, "weighted: normalize must be 0 .. 3");
    if (p->coverage < 0 || p->coverage > 1) return fail(ctx, STK_INVALID_PARAMS, "weighted: coverage must be 0 or 1");
    if (p->stat_step < 0 || p->stat_step > 64) return fail(ctx, STK_INVALID_PARAMS, "weighted: stat_step must be 0 .. 64");
    if (p->reserved != 0) return fail(ctx, STK_INVALID_PARAMS, "weight parameters: reserved must be 0");
    return STK_OK;
}

stk_status weighted_check_border(stk_ctx* ctx, int border_mode, const double* border_value, int coverage) {
    stk_status st = check_border_mode(ctx, border_mode);
    if (st) return st;
    if (coverage < 0 || coverage > 1) return fail(ctx, STK_INVALID_PARAMS, "weighted: coverage must be 0 or 1");
    if (coverage) {
        bool zero = border_mode == STK_BORDER_CONSTANT;
        for (int k = 0; k < 4 && border_value; k++) zero = zero && border_value[k] == 0.0;
        if (!zero) return fail(ctx, STK_INVALID_PARAMS, "weighted: coverage = 1 needs BORDER_CONSTANT with border value 0");
    }
    return STK_OK;
}

// the records of the table's entries: finite gains and offsets, finite weights >= 0, not all 0
stk_status weighted_check_coefs(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, int cn) {
    bool any = false;
    for (const stk_frame_weight& e : coef) {
        if (!std::isfinite(e.weight) || e.weight < 0.0f) return fail(ctx, STK_INVALID_PARAMS, "weighted: weights must be finite and >= 0");
        for (int c = 0; c < cn; c++)
            if (!std::isfinite(e.gain[c]) || !std::isfinite(e.offset[c]))
                return fail(ctx, STK_INVALID_PARAMS, "weighted: gains and offsets must be finite");
        any = any || e.weight > 0.0f;
    }
    if (!any) return fail(ctx, STK_INVALID_PARAMS, "weighted: every included weight is 0");
    return STK_OK;
}

// The moments pass over the n_entries entries of ctx->warpframes (uploaded for the w x h destination): (n_entries - 1) x
// cn x 6 doubles into `host`, entry 1 first. Synchronises; adds its device time to *ms.
stk_status weighted_moments(stk_ctx* ctx, int n_entries, const FoldSpec& spec, int step, double* host, double* ms) {
    if (n_entries < 2) return STK_OK;
    const WeightedLayout L = weighted_layout(n_entries, spec.w, spec.h, spec.cn, step);
    stk_status st = workspace_reserve(ctx, ctx->weighted, L.total, "weighted");
    if (st) return st;
    char* base = ctx->weighted.as<char>();
    const WarpArgs a = fold_warp_args(ctx, n_entries, spec);
    ClipArgs ca{};
    ca.partials = (double*)(base + L.partials);
    double* mom = (double*)(base + L.moments);
    const CombineOutputs o(host, mom, (size_t)(n_entries - 1) * spec.cn * 6, sizeof(double));
    if ((st = combine_begin(ctx))) return st;
    HIP_TRY(launch_overlap_moments(a, ca, spec.depth, step, mom, ctx->stream));
    return combine_end(ctx, ms, &o);
}

// The estimator (include/stacker.h): f64 on the host, each operation rounded on its own, results rounded to f32.
void weighted_estimate(const double* m /* cn x 6 */, int cn, int mode, stk_frame_weight* e) {
    e->flags = 0;
    for (int c = 0; c < 4; c++) { e->gain[c] = 1.0f; e->offset[c] = 0.0f; }
    if (mode == 0) return;
    for (int c = 0; c < cn; c++) {
        const double n = m[c * 6], sx = m[c * 6 + 1], sy = m[c * 6 + 2], sxx = m[c * 6 + 3], syy = m[c * 6 + 4];
        bool ok = n > 0.0;
        double g = 1.0, o = 0.0;
        if (ok) {
            const double mx = sx / n, my = sy / n;
            if (mode == 1) o = my - mx;
            else if (mode == 2) { ok = mx > 0.0; if (ok) g = my / mx; }
            else {
                const double vx = sxx / n - mx * mx, vy = syy / n - my * my;
                ok = vx > 0.0;
                if (ok) { g = std::sqrt(vy / vx); o = my - g * mx; }
            }
        }
        const float gf = (float)g, of = (float)o;
        if (!ok || !std::isfinite(gf) || !std::isfinite(of)) { e->flags |= 1 << c; continue; }
        e->gain[c] = gf; e->offset[c] = of;
    }
}

// (shared by every whole-stack form that takes stk_weight_params: robust.cpp, local.cpp, drizzle.cpp through context.h)
stk_status weighted_match_records(stk_ctx* ctx, int n, const EntryTable& table, const FoldSpec& spec, const stk_weight_params* p,
                                  const float* weights, std::vector<stk_frame_weight>& coef, stk_frame_weight* applied, double* ms) {
    const int ne = table.size(), cn = spec.cn;
    std::vector<double> mom((size_t)std::max(ne - 1, 0) * cn * 6);
    if (p->normalize != 0 && ne > 1) {
        stk_status st = weighted_moments(ctx, ne, spec, p->stat_step ? p->stat_step : 4, mom.data(), ms);
        if (st) return st;
    }
    coef.assign(ne, unit_record());
    for (int k = 0; k < ne; k++) {
        if (k > 0) weighted_estimate(mom.data() + (size_t)(k - 1) * cn * 6, cn, p->normalize, &coef[k]);
        coef[k].weight = weights ? weights[table.frame[k]] : 1.0f;
    }
    stk_status st = weighted_check_coefs(ctx, coef, cn);
    if (st) return st;
    if (applied) {
        for (int i = 0; i < n; i++) { applied[i] = unit_record(); applied[i].weight = 0.0f; }
        for (int k = 0; k < ne; k++) applied[table.frame[k]] = coef[k];
    }
    return STK_OK;
}

namespace {

// The weighted fold over the entries of ctx->warpframes with the per-entry records `coef`. Writes `out` and `coverage_out`
// (out's location); adds its device time to *ms.
stk_status weighted_fold(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, int coverage, stk_image_f32* out,
                         float* coverage_out, double* ms) {
    const int n_entries = (int)coef.size(), w = spec.w, h = spec.h, cn = spec.cn;
    const WeightedLayout L = weighted_layout(n_entries, w, h, cn, 0);
    stk_status st = workspace_reserve(ctx, ctx->weighted, L.total, "weighted");
    if (st) return st;
    char* base = ctx->weighted.as<char>();
    const CombineOutputs o(out, (float*)(base + L.image), (size_t)w * h * cn, {coverage_out, base + L.den, (size_t)w * h});
    const WarpArgs a = fold_warp_args(ctx, n_entries, spec);
    ClipArgs ca{};
    ca.coef = (const stk_frame_weight*)(base + L.coef);
    ca.coverage = coverage;
    ca.out = o.image();
    ca.out_stride = (size_t)w * cn;
    ca.den = o.side<float>(0);
    ca.den_stride = (size_t)w;
    if ((st = records_upload(ctx, base + L.coef, coef))) return st;
    if ((st = combine_begin(ctx))) return st;
    HIP_TRY(launch_weighted_fold(a, ca, spec.depth, ctx->stream));
    return combine_end(ctx, ms, &o);
}

// the checks the two whole-stack forms share, in the order the errors are reported; then their workspace (the plain call's
// mean lands in its image, unused)
stk_status weighted_match_check(stk_ctx* ctx, const stk_frames* frames, const stk_weight_params* weight, const stk_image_f32* out) {
    stk_status st = weighted_validate(ctx, weight);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    return combine_check_out(ctx, out, frames);
}
stk_status weighted_match_reserve(stk_ctx* ctx, const stk_frames* frames, const stk_weight_params* weight) {
    (void)hipSetDevice(ctx->device);
    const int step = weight->normalize ? (weight->stat_step ? weight->stat_step : 4) : 0;
    return workspace_reserve(ctx, ctx->weighted, weighted_layout(frames->n, frames->width, frames->height, frames->channels, step).total, "weighted");
}

// and their combine over the kept frames: the records, then one weighted fold
CombineFinish weighted_match_finish(stk_ctx* ctx, int n, const stk_weight_params* weight, const float* weights, stk_image_f32* out,
                                    float* coverage_out, stk_frame_weight* applied) {
    return [=](const EntryTable& table, const std::vector<const void*>&, const FoldSpec& spec, const stk_frame_stats*, double* ms) {
        std::vector<stk_frame_weight> coef;
        stk_status st = weighted_match_records(ctx, n, table, spec, weight, weights, coef, applied, ms);
        if (st) return st;
        return weighted_fold(ctx, coef, spec, weight->coverage, out, coverage_out, ms);
    };
}

}  // namespace

// (the fold alone, for a whole-stack form outside this file that makes its own records: noise.cpp)
stk_status weighted_fold_records(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, int coverage, stk_image_f32* out,
                                 float* coverage_out, double* ms) {
    return weighted_fold(ctx, coef, spec, coverage, out, coverage_out, ms);
}

extern "C" {

stk_status stk_weighted_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                              int32_t border_mode, const double* border_value, double alpha, const stk_frame_weight* per_frame,
                              int32_t coverage, stk_image_f32* out, float* coverage_out) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (!per_frame) return fail(ctx, STK_INVALID_PARAMS, "null per-frame records");
    if ((st = weighted_check_border(ctx, border_mode, border_value, coverage))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    EntryTable table;
    entries_from_include(frames->n, M, include, table);
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "weighted: no frame included");
    std::vector<stk_frame_weight> coef;
    gather_records(table, per_frame, coef);
    if ((st = weighted_check_coefs(ctx, coef, frames->channels))) return st;
    if ((st = entry_table_begin(ctx, frames, table, is_affine))) return st;
    double ms = 0.0;
    if ((st = weighted_fold(ctx, coef, fold_spec(frames, alpha, border_mode, border_value, is_affine), coverage, out, coverage_out, &ms)))
        return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

stk_status stk_overlap_moments(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                               int32_t border_mode, const double* border_value, double alpha, int32_t stat_step, double* moments) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (!moments) return fail(ctx, STK_INVALID_PARAMS, "null moments");
    if ((st = weighted_check_border(ctx, border_mode, border_value, 0))) return st;
    if (stat_step < 1 || stat_step > 64) return fail(ctx, STK_INVALID_PARAMS, "overlap moments: stat_step must be 1 .. 64");
    if (include && !include[0]) return fail(ctx, STK_INVALID_PARAMS, "overlap moments: frame 0 must be included");
    const int n = frames->n, cn = frames->channels;
    EntryTable table;
    entries_from_include(n, M, include, table);
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "weighted: no frame included");
    if ((st = entry_table_begin(ctx, frames, table, is_affine))) return st;
    const int ne = table.size();
    std::vector<double> mom((size_t)std::max(ne - 1, 0) * cn * 6);
    double ms = 0.0;
    if ((st = weighted_moments(ctx, ne, fold_spec(frames, alpha, border_mode, border_value, is_affine), stat_step, mom.data(), &ms))) return st;
    ctx->timing.finalize_ms = ms;
    std::memset(moments, 0, (size_t)n * cn * 6 * sizeof(double));
    for (int k = 1; k < ne; k++)
        std::memcpy(moments + (size_t)table.frame[k] * cn * 6, mom.data() + (size_t)(k - 1) * cn * 6, (size_t)cn * 6 * sizeof(double));
    return STK_OK;
}

stk_status stk_ecc_match_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                  const stk_weight_params* weight, const float* weights, stk_image_f32* out, float* coverage_out,
                                  stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = weighted_match_check(ctx, frames, weight, out);
    if (st) return st;
    if ((st = weighted_match_reserve(ctx, frames, weight))) return st;
    return ecc_match_then(ctx, frames, params, scale_down_width, ctx->weighted.as<float>(), stats,
                          weighted_match_finish(ctx, frames->n, weight, weights, out, coverage_out, applied));
}

stk_status stk_keypoint_match_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                                       const stk_weight_params* weight, const float* weights, stk_image_f32* out, int32_t* dropped,
                                       float* coverage_out, stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = weighted_match_check(ctx, frames, weight, out);
    if (st) return st;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null parameters");
    if (weight->coverage && (st = weighted_check_border(ctx, params->border_mode, params->border_value, 1))) return st;
    if ((st = weighted_match_reserve(ctx, frames, weight))) return st;
    return keypoint_match_then(ctx, frames, params, scale_down_width, ctx->weighted.as<float>(), dropped, stats,
                               weighted_match_finish(ctx, frames->n, weight, weights, out, coverage_out, applied));
}

}  // extern "C"
