// weighted.cpp — weighted, coverage-aware stacking with per-frame normalisation: stk_weighted_stack, stk_overlap_moments,
// stk_ecc_match_weighted, stk_keypoint_match_weighted (an extension beyond the reference; definition in
// include/stacker.h, kernels in kernels_weighted.hip).
// ctx->weighted (grow-only like the other workspaces) holds a w x h x cn f32 image (the plain call's mean in the
// whole-stack forms, then a host output's staging copy), the w x h den plane, the per-entry gain / offset / weight table,
// the moments and the per-wave partials they are reduced from. Like clip.cpp, the whole-stack forms run the plain call
// first and take the warps and the kept set from its stats; the frames are still resident in HBM. With normalize != 0 the
// moments pass and the host estimator follow, then one weighted fold.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

namespace {

struct WeightedLayout {
    size_t image, den, coef, moments, partials, total;     // byte offsets
};

WeightedLayout weighted_layout(int n_entries, int w, int h, int cn, int step) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    WeightedLayout L{};
    L.image = 0;
    L.den = up((size_t)w * h * cn * sizeof(float));
    L.coef = L.den + up((size_t)w * h * sizeof(float));
    L.moments = L.coef + up((size_t)std::max(n_entries, 1) * sizeof(stk_frame_weight));
    L.partials = L.moments + up((size_t)std::max(n_entries, 1) * cn * 6 * sizeof(double));
    size_t parts = 0;
    if (step > 0 && n_entries > 1) parts = moments_plan(w, h, step).parts() * (size_t)(n_entries - 1) * (1 + 5 * cn) * sizeof(double);
    L.total = L.partials + up(parts);
    return L;
}

}  // namespace

// (the checks, the moments pass and the estimator are shared with robust.cpp: context.h)
stk_status weighted_check_out(stk_ctx* ctx, const stk_image_f32* out, const stk_frames* f) {
    stk_status st = image_check(ctx, out, f->width, f->height, f->channels);
    if (st) return st;
    if (out->row_stride_bytes && out->row_stride_bytes != (size_t)f->width * f->channels * sizeof(float))
        return fail(ctx, STK_INVALID_PARAMS, "output must be tightly packed");
    return STK_OK;
}

stk_status weighted_validate(stk_ctx* ctx, const stk_weight_params* p) {
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null weight parameters");
    if (p->normalize < 0 || p->normalize > 3) return fail(ctx, STK_INVALID_PARAMS, "weighted: normalize must be 0 .. 3");
    if (p->coverage < 0 || p->coverage > 1) return fail(ctx, STK_INVALID_PARAMS, "weighted: coverage must be 0 or 1");
    if (p->stat_step < 0 || p->stat_step > 64) return fail(ctx, STK_INVALID_PARAMS, "weighted: stat_step must be 0 .. 64");
    if (p->reserved != 0) return fail(ctx, STK_INVALID_PARAMS, "weight parameters: reserved must be 0");
    return STK_OK;
}

stk_status weighted_check_border(stk_ctx* ctx, int border_mode, const double* border_value, int coverage) {
    if (border_mode < 0 || border_mode > 4)
        return fail(ctx, border_mode == STK_BORDER_TRANSPARENT ? STK_NOT_IMPLEMENTED : STK_INVALID_PARAMS,
                    "border mode not supported (BORDER_TRANSPARENT leaves the reference's output uninitialised)");
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

WarpArgs weighted_warp_args(stk_ctx* ctx, int n_entries, int depth, int w, int h, int cn, size_t src_row_bytes, double alpha,
                            int border_mode, const double* border_value, int is_affine) {
    WarpArgs a{};
    a.frames = ctx->warpframes.as<WarpFrame>();
    a.n_frames = n_entries;
    a.sw = w; a.sh = h; a.cn = cn;
    a.src_stride = src_row_bytes / (depth / 8);
    a.alpha = (float)alpha;
    a.border_mode = border_mode;
    for (int k = 0; k < 4; k++) a.bv[k] = border_value ? (float)border_value[k] : 0.f;
    a.acc = nullptr; a.dw = w; a.dh = h; a.acc_stride = 0;
    a.is_affine = is_affine; a.subpixel_bits = ctx->opt_subpixel_bits; a.tune = 0; a.interp = ctx->opt_interp;
    return a;
}

// The moments pass over the n_entries entries of ctx->warpframes (uploaded for the w x h destination): (n_entries - 1) x
// cn x 6 doubles into `host`, entry 1 first. Synchronises; adds its device time to *ms.
stk_status weighted_moments(stk_ctx* ctx, int n_entries, int depth, int w, int h, int cn, size_t src_row_bytes, double alpha,
                            int border_mode, const double* border_value, int is_affine, int step, double* host, double* ms) {
    if (n_entries < 2) return STK_OK;
    const WeightedLayout L = weighted_layout(n_entries, w, h, cn, step);
    HIP_TRY(ctx->weighted.reserve(L.total));
    char* base = ctx->weighted.as<char>();
    const WarpArgs a = weighted_warp_args(ctx, n_entries, depth, w, h, cn, src_row_bytes, alpha, border_mode, border_value, is_affine);
    ClipArgs ca{};
    ca.partials = (double*)(base + L.partials);
    double* mom = (double*)(base + L.moments);
    HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    HIP_TRY(launch_overlap_moments(a, ca, depth, step, mom, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    HIP_TRY(hipMemcpyAsync(host, mom, (size_t)(n_entries - 1) * cn * 6 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ms) *ms += ev_ms(ctx->ev[4], ctx->ev[5]);
    return STK_OK;
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

// common argument checks of the caller-held-warps forms (shared with local.cpp: context.h); fills the table's frame indices
stk_status weighted_table(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int is_affine,
                          std::vector<int>& entry_frame) {
    const int n = frames->n, w = frames->width, h = frames->height;
    for (int i = 0; i < n; i++) if (!include || include[i]) entry_frame.push_back(i);
    if (entry_frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "weighted: no frame included");
    (void)hipSetDevice(ctx->device);
    timing_begin(ctx);
    std::vector<const void*> dev;
    stk_status st = resolve_frames(ctx, frames, dev);
    if (st) return st;
    std::vector<WarpFrame> wf(entry_frame.size());
    for (size_t k = 0; k < entry_frame.size(); k++) make_warp_frame(wf[k], dev[entry_frame[k]], M + 9 * (size_t)entry_frame[k], is_affine);
    if ((st = warp_table_upload(ctx, wf, frame_row_bytes(frames), w, h, is_affine))) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));       // `wf` leaves scope
    return STK_OK;
}

namespace {

// The weighted fold over the n_entries entries of ctx->warpframes with the per-entry records `coef`. Writes `out` and
// `coverage_out` (out's location); adds its device time to *ms.
stk_status weighted_fold(stk_ctx* ctx, const std::vector<stk_frame_weight>& coef, int depth, int w, int h, int cn, size_t src_row_bytes,
                         double alpha, int border_mode, const double* border_value, int is_affine, int coverage,
                         stk_image_f32* out, float* coverage_out, double* ms) {
    const int n_entries = (int)coef.size();
    const WeightedLayout L = weighted_layout(n_entries, w, h, cn, 0);
    HIP_TRY(ctx->weighted.reserve(L.total));
    char* base = ctx->weighted.as<char>();
    const bool host = out->location != STK_DEVICE;
    const WarpArgs a = weighted_warp_args(ctx, n_entries, depth, w, h, cn, src_row_bytes, alpha, border_mode, border_value, is_affine);
    ClipArgs ca{};
    ca.coef = (const stk_frame_weight*)(base + L.coef);
    ca.coverage = coverage;
    ca.out = host ? (float*)(base + L.image) : out->data;
    ca.out_stride = (size_t)w * cn;
    ca.den = coverage_out ? (host ? (float*)(base + L.den) : coverage_out) : nullptr;
    ca.den_stride = (size_t)w;
    HIP_TRY(hipMemcpyAsync(base + L.coef, coef.data(), coef.size() * sizeof(stk_frame_weight), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    HIP_TRY(launch_weighted_fold(a, ca, depth, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    if (host) {
        HIP_TRY(hipMemcpyAsync(out->data, ca.out, (size_t)w * h * cn * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (coverage_out) HIP_TRY(hipMemcpyAsync(coverage_out, ca.den, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ms) *ms += ev_ms(ctx->ev[4], ctx->ev[5]);
    return STK_OK;
}

// the tail of the whole-stack forms: `entry_frame[k]` is the frame index of table entry k (entry 0 = frame 0)
stk_status weighted_finish(stk_ctx* ctx, const stk_frames* frames, const std::vector<int>& entry_frame, int depth, size_t rb,
                           int border_mode, const double* border_value, int is_affine, const stk_weight_params* p,
                           const float* weights, stk_image_f32* out, float* coverage_out, stk_frame_weight* applied) {
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const int ne = (int)entry_frame.size();
    const double alpha = 1.0 / 255.0;
    std::vector<stk_frame_weight> coef(ne);
    double ms = 0.0;
    std::vector<double> mom((size_t)std::max(ne - 1, 0) * cn * 6);
    if (p->normalize != 0 && ne > 1) {
        const int step = p->stat_step ? p->stat_step : 4;
        stk_status st = weighted_moments(ctx, ne, depth, w, h, cn, rb, alpha, border_mode, border_value, is_affine, step, mom.data(), &ms);
        if (st) return st;
    }
    for (int k = 0; k < ne; k++) {
        if (k == 0) weighted_estimate(nullptr, cn, 0, &coef[k]);
        else weighted_estimate(mom.data() + (size_t)(k - 1) * cn * 6, cn, p->normalize, &coef[k]);
        coef[k].weight = weights ? weights[entry_frame[k]] : 1.0f;
    }
    stk_status st = weighted_check_coefs(ctx, coef, cn);
    if (st) return st;
    if ((st = weighted_fold(ctx, coef, depth, w, h, cn, rb, alpha, border_mode, border_value, is_affine, p->coverage, out, coverage_out, &ms)))
        return st;
    ctx->timing.finalize_ms = ms;
    if (applied) {
        for (int i = 0; i < n; i++) { weighted_estimate(nullptr, cn, 0, &applied[i]); applied[i].weight = 0.0f; }
        for (int k = 0; k < ne; k++) applied[entry_frame[k]] = coef[k];
    }
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_weighted_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                              int32_t border_mode, const double* border_value, double alpha, const stk_frame_weight* per_frame,
                              int32_t coverage, stk_image_f32* out, float* coverage_out) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (!per_frame) return fail(ctx, STK_INVALID_PARAMS, "null per-frame records");
    if ((st = weighted_check_border(ctx, border_mode, border_value, coverage))) return st;
    if ((st = weighted_check_out(ctx, out, frames))) return st;
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    std::vector<stk_frame_weight> coef;
    for (int i = 0; i < n; i++) if (!include || include[i]) coef.push_back(per_frame[i]);
    if (coef.empty()) return fail(ctx, STK_INVALID_PARAMS, "weighted: no frame included");
    if ((st = weighted_check_coefs(ctx, coef, cn))) return st;
    std::vector<int> entry_frame;
    if ((st = weighted_table(ctx, frames, M, include, is_affine, entry_frame))) return st;
    double ms = 0.0;
    if ((st = weighted_fold(ctx, coef, frames->depth, w, h, cn, frame_row_bytes(frames), alpha, border_mode, border_value, is_affine,
                            coverage, out, coverage_out, &ms)))
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
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    std::vector<int> entry_frame;
    if ((st = weighted_table(ctx, frames, M, include, is_affine, entry_frame))) return st;
    const int ne = (int)entry_frame.size();
    std::vector<double> mom((size_t)std::max(ne - 1, 0) * cn * 6);
    double ms = 0.0;
    if ((st = weighted_moments(ctx, ne, frames->depth, w, h, cn, frame_row_bytes(frames), alpha, border_mode, border_value, is_affine,
                               stat_step, mom.data(), &ms)))
        return st;
    ctx->timing.finalize_ms = ms;
    std::memset(moments, 0, (size_t)n * cn * 6 * sizeof(double));
    for (int k = 1; k < ne; k++)
        std::memcpy(moments + (size_t)entry_frame[k] * cn * 6, mom.data() + (size_t)(k - 1) * cn * 6, (size_t)cn * 6 * sizeof(double));
    return STK_OK;
}

stk_status stk_ecc_match_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                  const stk_weight_params* weight, const float* weights, stk_image_f32* out, float* coverage_out,
                                  stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = weighted_validate(ctx, weight);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = weighted_check_out(ctx, out, frames))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const int step = weight->normalize ? (weight->stat_step ? weight->stat_step : 4) : 0;
    HIP_TRY(ctx->weighted.reserve(weighted_layout(n, w, h, cn, step).total));
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    // the plain call, on this context's own device, its mean into the workspace image (unused)
    stk_image_f32 mimg{ctx->weighted.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = ecc_match_single(ctx, frames, params, scale_down_width, &mimg, stats))) return st;
    const stk_timing keep = ctx->timing;
    // every frame is a sample: frame 0 through the identity, frame i through its warp (as in stk_ecc_match_clipped)
    const int is_affine = params->motion_type != STK_MOTION_HOMOGRAPHY;
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    std::vector<WarpFrame> wf(n);
    std::vector<int> entry_frame(n);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    make_warp_frame(wf[0], dev[0], I3, is_affine);
    for (int i = 1; i < n; i++) make_warp_frame(wf[i], dev[i], stats[i].warp, is_affine);
    for (int i = 0; i < n; i++) entry_frame[i] = i;
    const size_t rb = frame_row_bytes(frames);
    if ((st = warp_table_upload(ctx, wf, rb, w, h, is_affine))) return st;
    st = weighted_finish(ctx, frames, entry_frame, frames->depth, rb, STK_BORDER_CONSTANT, nullptr, is_affine, weight, weights, out,
                         coverage_out, applied);
    const double fin = ctx->timing.finalize_ms;
    ctx->timing = keep; ctx->timing.finalize_ms = st ? 0.0 : fin;
    return st;
}

stk_status stk_keypoint_match_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                                       const stk_weight_params* weight, const float* weights, stk_image_f32* out, int32_t* dropped,
                                       float* coverage_out, stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = weighted_validate(ctx, weight);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = weighted_check_out(ctx, out, frames))) return st;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null parameters");
    if (weight->coverage && (st = weighted_check_border(ctx, params->border_mode, params->border_value, 1))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const int step = weight->normalize ? (weight->stat_step ? weight->stat_step : 4) : 0;
    HIP_TRY(ctx->weighted.reserve(weighted_layout(n, w, h, cn, step).total));
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    stk_image_f32 mimg{ctx->weighted.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = keypoint_match_single(ctx, frames, params, scale_down_width, &mimg, dropped, stats))) return st;
    const stk_timing keep = ctx->timing;
    // the samples: frame 0 through the identity and the frames with a homography (status 0), in stack order, with the
    // params' border (as in stk_keypoint_match_clipped)
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    std::vector<WarpFrame> wf;
    std::vector<int> entry_frame;
    wf.reserve(n);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    wf.emplace_back();
    make_warp_frame(wf.back(), dev[0], I3, 0);
    entry_frame.push_back(0);
    for (int i = 1; i < n; i++) {
        if (stats[i].status != 0) continue;
        wf.emplace_back();
        make_warp_frame(wf.back(), dev[i], stats[i].warp, 0);
        entry_frame.push_back(i);
    }
    const size_t rb = frame_row_bytes(frames);
    if ((st = warp_table_upload(ctx, wf, rb, w, h, 0))) return st;
    st = weighted_finish(ctx, frames, entry_frame, 8, rb, params->border_mode, params->border_value, 0, weight, weights, out, coverage_out,
                         applied);
    const double fin = ctx->timing.finalize_ms;
    ctx->timing = keep; ctx->timing.finalize_ms = st ? 0.0 : fin;
    return st;
}

}  // extern "C"
