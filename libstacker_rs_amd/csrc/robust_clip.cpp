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
// the kept set from its stats.
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

stk_status robust_clip_bands(stk_ctx* ctx, int n_entries, const std::vector<stk_frame_weight>* coef, int depth, int w, int h, int cn,
                             size_t src_row_bytes, double alpha, int border_mode, const double* border_value, int is_affine,
                             int coverage, const stk_robust_clip_params* p, stk_image_f32* out, int32_t* counts, float* kept, double* ms) {
    stk_status st = quantile_check_count(ctx, n_entries);
    if (st) return st;
    const size_t row = (size_t)w * cn, nel = row * h;
    const size_t R = quantile_band_rows(ctx, n_entries, w, h, cn);
    HIP_TRY(ctx->clip.reserve(3 * nel * sizeof(float)));
    HIP_TRY(ctx->quantile.reserve(R * n_entries * row * sizeof(float)));
    float* c = ctx->clip.as<float>();
    float* band = ctx->quantile.as<float>();
    WarpArgs a = weighted_warp_args(ctx, n_entries, depth, w, h, cn, src_row_bytes, alpha, border_mode, border_value, is_affine);
    const bool host = out->location != STK_DEVICE;
    ClipArgs ca{};
    ca.c = c; ca.L = c + nel; ca.U = c + 2 * nel;
    ca.plane_stride = row;
    // a host output goes through the planes themselves, as in clip.cpp: the last pass reads c, L, U before it writes there
    ca.out = host ? c : out->data;
    ca.out_stride = row;
    ca.counts = counts ? (host ? (int*)ca.L : counts) : nullptr;
    ca.kept = coef && kept ? (host ? ca.U : kept) : nullptr;
    ca.kappa_low = p->kappa_low; ca.kappa_high = p->kappa_high;
    ca.band = band;
    if (coef) {
        HIP_TRY(ctx->coef.reserve(coef->size() * sizeof(stk_frame_weight)));
        HIP_TRY(hipMemcpyAsync(ctx->coef.p, coef->data(), coef->size() * sizeof(stk_frame_weight), hipMemcpyHostToDevice, ctx->stream));
        ca.coef = ctx->coef.as<stk_frame_weight>();
        ca.coverage = coverage;
    }
    const size_t n_bands = ((size_t)h + R - 1) / R;
    while (ctx->select_ev.size() < n_bands) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
        ctx->select_ev.emplace_back(e0, e1);
    }
    HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    size_t b = 0;
    for (size_t y0 = 0; y0 < (size_t)h; y0 += R, b++) {
        const size_t rows = std::min(R, (size_t)h - y0);
        ca.y0 = (int)y0; ca.band_rows = (int)rows;
        a.dh = (int)(y0 + rows);
        HIP_TRY(coef ? launch_quantile_store_weighted(a, ca, depth, ctx->stream) : launch_quantile_store(a, ca, depth, ctx->stream));
        HIP_TRY(hipEventRecord(ctx->select_ev[b].first, ctx->stream));
        HIP_TRY(launch_robust_select(band, rows * row, n_entries, coef ? 1 : 0, *p, ca.c + y0 * row, ca.L + y0 * row, ca.U + y0 * row,
                                     ctx->stream));
        HIP_TRY(hipEventRecord(ctx->select_ev[b].second, ctx->stream));
    }
    // the planes are complete: the last pass of the (weighted) clip over the whole frame
    a.dh = h;
    ca.first = 0; ca.last = 1; ca.centre = 0;
    HIP_TRY(coef ? launch_clip_pass_weighted(a, ca, depth, ctx->stream) : launch_clip_pass(a, ca, depth, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    if (host) {
        HIP_TRY(hipMemcpyAsync(out->data, c, nel * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (counts) HIP_TRY(hipMemcpyAsync(counts, ca.L, nel * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (ca.kept) HIP_TRY(hipMemcpyAsync(kept, ca.U, nel * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ms) *ms += ev_ms(ctx->ev[4], ctx->ev[5]);
    double sel = 0.0;
    for (size_t k = 0; k < n_bands; k++) sel += ev_ms(ctx->select_ev[k].first, ctx->select_ev[k].second);
    ctx->robust_select_us = (int64_t)std::llround(sel * 1000.0);
    return STK_OK;
}

extern "C" {

stk_status stk_robust_clip_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                 int32_t border_mode, const double* border_value, double alpha, const stk_robust_clip_params* clip,
                                 stk_image_f32* out, int32_t* counts) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (border_mode < 0 || border_mode > 4)
        return fail(ctx, border_mode == STK_BORDER_TRANSPARENT ? STK_NOT_IMPLEMENTED : STK_INVALID_PARAMS,
                    "border mode not supported (BORDER_TRANSPARENT leaves the reference's output uninitialised)");
    if ((st = robust_clip_validate(ctx, clip))) return st;
    if ((st = clip_check_out(ctx, out, frames))) return st;
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    int n_in = 0;
    for (int i = 0; i < n; i++) n_in += (!include || include[i]) ? 1 : 0;
    if (n_in == 0) return fail(ctx, STK_INVALID_PARAMS, "robust clipping: no frame included");
    if ((st = quantile_check_count(ctx, n_in))) return st;
    (void)hipSetDevice(ctx->device);
    timing_begin(ctx);
    std::vector<const void*> dev;
    if ((st = resolve_frames(ctx, frames, dev))) return st;
    std::vector<WarpFrame> wf;
    wf.reserve(n_in);
    for (int i = 0; i < n; i++) {
        if (include && !include[i]) continue;
        wf.emplace_back();
        make_warp_frame(wf.back(), dev[i], M + 9 * (size_t)i, is_affine);
    }
    const size_t rb = frame_row_bytes(frames);
    if ((st = warp_table_upload(ctx, wf, rb, w, h, is_affine))) return st;
    double ms = 0.0;
    st = robust_clip_bands(ctx, n_in, nullptr, frames->depth, w, h, cn, rb, alpha, border_mode, border_value, is_affine, 0, clip, out,
                           counts, nullptr, &ms);
    ctx->timing.finalize_ms = st ? 0.0 : ms;
    return st;
}

stk_status stk_ecc_match_robust_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                        const stk_robust_clip_params* clip, stk_image_f32* out, int32_t* counts,
                                        stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = robust_clip_validate(ctx, clip);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = clip_check_out(ctx, out, frames))) return st;
    if ((st = quantile_check_count(ctx, frames->n))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    HIP_TRY(ctx->clip.reserve(3 * (size_t)w * h * cn * sizeof(float)));
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    // the plain call, on this context's own device, its mean into the c plane (unused: the selection overwrites it)
    stk_image_f32 cimg{ctx->clip.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = ecc_match_single(ctx, frames, params, scale_down_width, &cimg, stats))) return st;
    const stk_timing keep = ctx->timing;
    // every frame is a sample: frame 0 through the identity, frame i through its warp (as in stk_ecc_match_clipped)
    const int is_affine = params->motion_type != STK_MOTION_HOMOGRAPHY;
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    std::vector<WarpFrame> wf(n);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    make_warp_frame(wf[0], dev[0], I3, is_affine);
    for (int i = 1; i < n; i++) make_warp_frame(wf[i], dev[i], stats[i].warp, is_affine);
    const size_t rb = frame_row_bytes(frames);
    if ((st = warp_table_upload(ctx, wf, rb, w, h, is_affine))) return st;
    double ms = 0.0;
    st = robust_clip_bands(ctx, n, nullptr, frames->depth, w, h, cn, rb, 1.0 / 255.0, STK_BORDER_CONSTANT, nullptr, is_affine, 0, clip, out,
                           counts, nullptr, &ms);
    ctx->timing = keep; ctx->timing.finalize_ms = st ? 0.0 : ms;
    return st;
}

stk_status stk_keypoint_match_robust_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                             float scale_down_width, const stk_robust_clip_params* clip, stk_image_f32* out,
                                             int32_t* dropped, int32_t* counts, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = robust_clip_validate(ctx, clip);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = clip_check_out(ctx, out, frames))) return st;
    if ((st = quantile_check_count(ctx, frames->n))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    HIP_TRY(ctx->clip.reserve(3 * (size_t)w * h * cn * sizeof(float)));
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    stk_image_f32 cimg{ctx->clip.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = keypoint_match_single(ctx, frames, params, scale_down_width, &cimg, dropped, stats))) return st;
    const stk_timing keep = ctx->timing;
    // the samples: frame 0 through the identity and the frames with a homography (status 0), in stack order, with the
    // params' border (as in stk_keypoint_match_clipped)
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    std::vector<WarpFrame> wf;
    wf.reserve(n);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    wf.emplace_back();
    make_warp_frame(wf.back(), dev[0], I3, 0);
    for (int i = 1; i < n; i++) {
        if (stats[i].status != 0) continue;
        wf.emplace_back();
        make_warp_frame(wf.back(), dev[i], stats[i].warp, 0);
    }
    const size_t rb = frame_row_bytes(frames);
    if ((st = warp_table_upload(ctx, wf, rb, w, h, 0))) return st;
    double ms = 0.0;
    st = robust_clip_bands(ctx, (int)wf.size(), nullptr, 8, w, h, cn, rb, 1.0 / 255.0, params->border_mode, params->border_value, 0, 0,
                           clip, out, counts, nullptr, &ms);
    ctx->timing = keep; ctx->timing.finalize_ms = st ? 0.0 : ms;
    return st;
}

}  // extern "C"
