// quantile.cpp — median and quantile stacking: stk_quantile_stack, stk_ecc_match_quantile, stk_keypoint_match_quantile (an
// extension beyond the reference; definition in include/stacker.h, kernels in kernels_quantile.hip).
// An order statistic needs all N samples of a pixel at once, so the combine goes band by band: rows [y0, y0 + R) of every
// frame are warped by the fold kernel in its store mode into a sample buffer (N x R x w x cn f32), then the selection
// kernel reduces them to R output rows. ctx->quantile holds a w x h x cn f32 image (the plain call's mean in the
// whole-stack forms, then a host output's staging copy) followed by the band. It is grow-only like the other workspaces;
// R is sized to a 4 GiB band (option quantile_band_rows caps it). Like clip.cpp, the whole-stack forms run the plain call
// first and take the warps and the kept set from its stats; the frames are still resident in HBM.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

namespace {

constexpr size_t QUANTILE_BAND_BYTES = (size_t)4 << 30;

}  // namespace

// (the checks and the band geometry are shared with robust.cpp: context.h)
stk_status quantile_validate(stk_ctx* ctx, const stk_quantile_params* p) {
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null quantile parameters");
    if (!(p->quantile >= 0.0f && p->quantile <= 1.0f))
        return fail(ctx, STK_INVALID_PARAMS, "quantile must be in [0, 1], got " + std::to_string(p->quantile));
    if (p->reserved != 0) return fail(ctx, STK_INVALID_PARAMS, "quantile parameters: reserved must be 0");
    return STK_OK;
}

stk_status quantile_check_out(stk_ctx* ctx, const stk_image_f32* out, const stk_frames* f) {
    stk_status st = image_check(ctx, out, f->width, f->height, f->channels);
    if (st) return st;
    if (out->row_stride_bytes && out->row_stride_bytes != (size_t)f->width * f->channels * sizeof(float))
        return fail(ctx, STK_INVALID_PARAMS, "output must be tightly packed");
    return STK_OK;
}

stk_status quantile_check_count(stk_ctx* ctx, int n) {
    if (n > QUANTILE_MAX_SAMPLES)
        return fail(ctx, STK_NOT_IMPLEMENTED, "quantile: at most " + std::to_string(QUANTILE_MAX_SAMPLES) + " samples per pixel, got " +
                                                  std::to_string(n));
    return STK_OK;
}

// floats of the image in front of the band (rounded up to 256 bytes: the band's rows start aligned)
size_t quantile_image_floats(int w, int h, int cn) { return ((size_t)w * h * cn + 63) & ~(size_t)63; }

size_t quantile_band_rows(const stk_ctx* ctx, int n, int w, int h, int cn) {
    const size_t row = (size_t)n * w * cn * sizeof(float);
    size_t R = std::max<size_t>(1, QUANTILE_BAND_BYTES / row);
    if (ctx->opt_quantile_band_rows > 0) R = std::min<size_t>(R, (size_t)ctx->opt_quantile_band_rows);
    return std::min<size_t>(R, (size_t)h);
}

// room for the image and, n > 0, the band of an n-frame w x h x cn stack
stk_status quantile_reserve(stk_ctx* ctx, int n, int w, int h, int cn) {
    const size_t R = n > 0 ? quantile_band_rows(ctx, n, w, h, cn) : 0;
    HIP_TRY(ctx->quantile.reserve((quantile_image_floats(w, h, cn) + R * n * w * cn) * sizeof(float)));
    return STK_OK;
}

namespace {

// The combine over the n_frames entries of ctx->warpframes (uploaded for the w x h destination): per band a store launch,
// then a selection launch into `out` (device) or the staging image (host, one copy back at the end). Sets
// stk_timing.finalize_ms to the device time of all bands.
stk_status quantile_bands(stk_ctx* ctx, int n_frames, int depth, int w, int h, int cn, size_t src_row_bytes, double alpha,
                          int border_mode, const double* border_value, int is_affine, const stk_quantile_params* p,
                          stk_image_f32* out) {
    stk_status st = quantile_check_count(ctx, n_frames);
    if (st) return st;
    if ((st = quantile_reserve(ctx, n_frames, w, h, cn))) return st;
    const size_t R = quantile_band_rows(ctx, n_frames, w, h, cn), row = (size_t)w * cn;
    float* img = ctx->quantile.as<float>();
    float* band = img + quantile_image_floats(w, h, cn);
    const bool host = out->location != STK_DEVICE;
    float* dst = host ? img : out->data;
    // j and g in f32, each operation rounded on its own, as the definition states them
    const float vi = (float)(n_frames - 1) * p->quantile;
    const float jf = std::floor(vi);
    const float g = vi - jf;
    const int j = (int)jf;
    WarpArgs a{};
    a.frames = ctx->warpframes.as<WarpFrame>();
    a.n_frames = n_frames;
    a.sw = w; a.sh = h; a.cn = cn;
    a.src_stride = src_row_bytes / (depth / 8);
    a.alpha = (float)alpha;
    a.border_mode = border_mode;
    for (int k = 0; k < 4; k++) a.bv[k] = border_value ? (float)border_value[k] : 0.f;
    a.acc = nullptr; a.dw = w; a.acc_stride = 0;
    a.is_affine = is_affine; a.subpixel_bits = ctx->opt_subpixel_bits; a.tune = 0; a.interp = ctx->opt_interp;
    ClipArgs ca{};
    ca.band = band;
    ca.plane_stride = row;
    HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    for (size_t y0 = 0; y0 < (size_t)h; y0 += R) {
        const size_t rows = std::min(R, (size_t)h - y0);
        ca.y0 = (int)y0; ca.band_rows = (int)rows;
        a.dh = (int)(y0 + rows);
        HIP_TRY(launch_quantile_store(a, ca, depth, ctx->stream));
        HIP_TRY(launch_quantile_select(band, rows * row, n_frames, j, g, dst + y0 * row, ctx->stream));
    }
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    if (host) HIP_TRY(hipMemcpyAsync(out->data, img, (size_t)h * row * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.finalize_ms = ev_ms(ctx->ev[4], ctx->ev[5]);
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_quantile_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                              int32_t border_mode, const double* border_value, double alpha, const stk_quantile_params* quantile,
                              stk_image_f32* out) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (border_mode < 0 || border_mode > 4)
        return fail(ctx, border_mode == STK_BORDER_TRANSPARENT ? STK_NOT_IMPLEMENTED : STK_INVALID_PARAMS,
                    "border mode not supported (BORDER_TRANSPARENT leaves the reference's output uninitialised)");
    if ((st = quantile_validate(ctx, quantile))) return st;
    if ((st = quantile_check_out(ctx, out, frames))) return st;
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    int n_in = 0;
    for (int i = 0; i < n; i++) n_in += (!include || include[i]) ? 1 : 0;
    if (n_in == 0) return fail(ctx, STK_INVALID_PARAMS, "quantile: no frame included");
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
    return quantile_bands(ctx, n_in, frames->depth, w, h, cn, rb, alpha, border_mode, border_value, is_affine, quantile, out);
}

stk_status stk_ecc_match_quantile(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                  const stk_quantile_params* quantile, stk_image_f32* out, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = quantile_validate(ctx, quantile);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = quantile_check_out(ctx, out, frames))) return st;
    if ((st = quantile_check_count(ctx, frames->n))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    if ((st = quantile_reserve(ctx, 0, w, h, cn))) return st;        // the image only: the band comes after the plain call
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    // the plain call, on this context's own device, its mean into the image in front of the band (unused)
    stk_image_f32 mimg{ctx->quantile.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = ecc_match_single(ctx, frames, params, scale_down_width, &mimg, stats))) return st;
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
    st = quantile_bands(ctx, n, frames->depth, w, h, cn, rb, 1.0 / 255.0, STK_BORDER_CONSTANT, nullptr, is_affine, quantile, out);
    const double fin = ctx->timing.finalize_ms;
    ctx->timing = keep; ctx->timing.finalize_ms = fin;
    return st;
}

stk_status stk_keypoint_match_quantile(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                                       const stk_quantile_params* quantile, stk_image_f32* out, int32_t* dropped,
                                       stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = quantile_validate(ctx, quantile);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = quantile_check_out(ctx, out, frames))) return st;
    if ((st = quantile_check_count(ctx, frames->n))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    if ((st = quantile_reserve(ctx, 0, w, h, cn))) return st;        // the image only: the band comes after the plain call
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    stk_image_f32 mimg{ctx->quantile.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = keypoint_match_single(ctx, frames, params, scale_down_width, &mimg, dropped, stats))) return st;
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
    st = quantile_bands(ctx, (int)wf.size(), 8, w, h, cn, rb, 1.0 / 255.0, params->border_mode, params->border_value, 0, quantile, out);
    const double fin = ctx->timing.finalize_ms;
    ctx->timing = keep; ctx->timing.finalize_ms = fin;
    return st;
}

}  // extern "C"
