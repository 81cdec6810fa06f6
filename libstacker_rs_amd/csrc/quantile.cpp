// quantile.cpp — median and quantile stacking: stk_quantile_stack, stk_ecc_match_quantile, stk_keypoint_match_quantile (an
// extension beyond the reference; definition in include/stacker.h, kernels in kernels_quantile.hip).
// An order statistic needs all N samples of a pixel at once, so the combine goes band by band: rows [y0, y0 + R) of every
// frame are warped by the fold kernel in its store mode into a sample buffer (N x R x w x cn f32), then the selection
// kernel reduces them to R output rows. ctx->quantile holds a w x h x cn f32 image (the plain call's mean in the
// whole-stack forms, then a host output's staging copy) followed by the band. It is grow-only like the other workspaces;
// R is sized to a 4 GiB band (option quantile_band_rows caps it). Like clip.cpp, the whole-stack forms run the plain call
// first and take the warps and the kept set from its stats (combine.h); the frames are still resident in HBM.
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

stk_status quantile_check_count(stk_ctx* ctx, int n) {
    if (n > QUANTILE_MAX_SAMPLES)
        return fail(ctx, STK_NOT_IMPLEMENTED, "quantile: at most " + std::to_string(QUANTILE_MAX_SAMPLES) + " samples per pixel, got " +
                                                  std::to_string(n));
    return STK_OK;
}

size_t quantile_band_rows(const stk_ctx* ctx, int n, int w, int h, int cn) {
    const size_t row = (size_t)n * w * cn * sizeof(float);
    size_t R = std::max<size_t>(1, QUANTILE_BAND_BYTES / row);
    if (ctx->opt_quantile_band_rows > 0) R = std::min<size_t>(R, (size_t)ctx->opt_quantile_band_rows);
    return std::min<size_t>(R, (size_t)h);
}

stk_status quantile_reserve(stk_ctx* ctx, int n, int w, int h, int cn, bool counts, QuantileLayout* L) {
    const QuantileLayout Q = quantile_layout(n, n > 0 ? quantile_band_rows(ctx, n, w, h, cn) : 0, w, h, cn, counts);
    if (L) *L = Q;
    return workspace_reserve(ctx, ctx->quantile, Q.total, "quantile");
}

namespace {

// The combine over the n_frames entries of ctx->warpframes (uploaded for the w x h destination): per band a store launch,
// then a selection launch into `out` (device) or the staging image (host, one copy back at the end). Adds the device time
// of all bands to *ms.
stk_status quantile_bands(stk_ctx* ctx, int n_frames, const FoldSpec& spec, const stk_quantile_params* p, stk_image_f32* out, double* ms) {
    const int w = spec.w, h = spec.h, cn = spec.cn, depth = spec.depth;
    stk_status st = quantile_check_count(ctx, n_frames);
    if (st) return st;
    QuantileLayout L;
    if ((st = quantile_reserve(ctx, n_frames, w, h, cn, false, &L))) return st;
    const size_t R = quantile_band_rows(ctx, n_frames, w, h, cn), row = (size_t)w * cn;
    float* band = (float*)(ctx->quantile.as<char>() + L.band);
    const CombineOutputs o(out, (float*)(ctx->quantile.as<char>() + L.image), (size_t)h * row);
    float* dst = o.image();
    // j and g in f32, each operation rounded on its own, as the definition states them
    const float vi = (float)(n_frames - 1) * p->quantile;
    const float jf = std::floor(vi);
    const float g = vi - jf;
    const int j = (int)jf;
    WarpArgs a = fold_warp_args(ctx, n_frames, spec);      // (dh: per band)
    ClipArgs ca{};
    ca.band = band;
    ca.plane_stride = row;
    if ((st = combine_begin(ctx))) return st;
    for (size_t y0 = 0; y0 < (size_t)h; y0 += R) {
        const size_t rows = std::min(R, (size_t)h - y0);
        ca.y0 = (int)y0; ca.band_rows = (int)rows;
        a.dh = (int)(y0 + rows);
        HIP_TRY(launch_quantile_store(a, ca, depth, ctx->stream));
        HIP_TRY(launch_quantile_select(band, rows * row, n_frames, j, g, dst + y0 * row, ctx->stream));
    }
    return combine_end(ctx, ms, &o);
}

// the checks and the workspace of the two whole-stack forms: the image only (the plain call's mean lands in front of the
// band, unused); the band comes after the plain call
stk_status quantile_match_begin(stk_ctx* ctx, const stk_frames* frames, const stk_quantile_params* quantile, const stk_image_f32* out) {
    stk_status st = quantile_validate(ctx, quantile);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    if ((st = quantile_check_count(ctx, frames->n))) return st;
    (void)hipSetDevice(ctx->device);
    return quantile_reserve(ctx, 0, frames->width, frames->height, frames->channels, false, nullptr);
}

// and their combine over the kept frames
CombineFinish quantile_match_finish(stk_ctx* ctx, const stk_quantile_params* quantile, stk_image_f32* out) {
    return [=](const EntryTable& table, const std::vector<const void*>&, const FoldSpec& spec, const stk_frame_stats*, double* ms) {
        return quantile_bands(ctx, table.size(), spec, quantile, out, ms);
    };
}

}  // namespace

extern "C" {

stk_status stk_quantile_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                              int32_t border_mode, const double* border_value, double alpha, const stk_quantile_params* quantile,
                              stk_image_f32* out) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if ((st = check_border_mode(ctx, border_mode))) return st;
    if ((st = quantile_validate(ctx, quantile))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    EntryTable table;
    entries_from_include(frames->n, M, include, table);
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "quantile: no frame included");
    if ((st = quantile_check_count(ctx, table.size()))) return st;
    if ((st = entry_table_begin(ctx, frames, table, is_affine))) return st;
    double ms = 0.0;
    if ((st = quantile_bands(ctx, table.size(), fold_spec(frames, alpha, border_mode, border_value, is_affine), quantile, out, &ms))) return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

stk_status stk_ecc_match_quantile(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                  const stk_quantile_params* quantile, stk_image_f32* out, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = quantile_match_begin(ctx, frames, quantile, out);
    if (st) return st;
    return ecc_match_then(ctx, frames, params, scale_down_width, ctx->quantile.as<float>(), stats, quantile_match_finish(ctx, quantile, out));
}

stk_status stk_keypoint_match_quantile(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                                       const stk_quantile_params* quantile, stk_image_f32* out, int32_t* dropped,
                                       stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = quantile_match_begin(ctx, frames, quantile, out);
    if (st) return st;
    return keypoint_match_then(ctx, frames, params, scale_down_width, ctx->quantile.as<float>(), dropped, stats,
                               quantile_match_finish(ctx, quantile, out));
}

}  // extern "C"
