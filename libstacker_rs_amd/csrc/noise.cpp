// noise.cpp — per-frame noise estimation and inverse-variance frame weights (an extension beyond the reference; definition
// in include/stacker.h, stk_noise_stat): stk_stack_noise, stk_noise_from_hist, stk_noise_weights,
// stk_ecc_match_noise_weighted, stk_keypoint_match_noise_weighted. The histograms of all frames come from one device pass
// (kernels_noise.hip) and travel to the host in one copy per batch; their reduction and the weights are host code
// (noise_host.h). ctx->quality (the workspace of the whole-stack passes, quality.cpp) holds the frame pointer table, the
// depth-16 window origins and the global histograms of one batch of frames. The whole-stack forms run the plain call
// first (combine.h) and then, over the frames still resident in HBM: the weighted form's records, the noise pass, the
// weights, one weighted fold.
#include <algorithm>
#include <cstring>

#include "context.h"
#include "noise_host.h"

using namespace stk;

namespace {

constexpr size_t NOISE_MAX_PIXELS = (size_t)1 << 27;              // quality.cpp's cap: sum b^2 HR[b] <= 65535^2 x 2^27 stays inside int64
constexpr size_t NOISE_HIST_BYTES = (size_t)256 << 20;            // global histograms of one batch (depth 16: 512 kB per frame and channel)

stk_status noise_check(stk_ctx* ctx, const stk_frames* f) {
    if (f->depth == 32)
        return fail(ctx, STK_NOT_IMPLEMENTED, "noise estimation takes 8- and 16-bit frames: the histograms are defined on integer values");
    if (f->width < 3 || f->height < 3) return fail(ctx, STK_INVALID_PARAMS, "noise estimation needs frames of at least 3 x 3 pixels");
    if ((size_t)f->width * f->height > NOISE_MAX_PIXELS)
        return fail(ctx, STK_NOT_IMPLEMENTED, "noise estimation: frames above 2^27 pixels could overflow the int64 sums");
    return STK_OK;
}

// The histograms of the n frames `src` (all in host or all in device memory, one row stride `rb`) into `hist` (host memory,
// n x cn x noise_hist_bins(depth)). Synchronises. *ms: the device time of the pass, for host frames with their copies.
stk_status noise_histograms(stk_ctx* ctx, const void* const* src, bool host, int n, int cn, int depth, int w, int h, size_t rb,
                            size_t copy_bytes, uint32_t* hist, double* ms) {
    (void)hipSetDevice(ctx->device);
    const size_t fb = rb * h, bins = noise_hist_bins(depth), per_frame = (size_t)cn * bins * sizeof(uint32_t);
    int batch = (int)std::min<size_t>({(size_t)n, (size_t)65535, std::max<size_t>(1, NOISE_HIST_BYTES / per_frame)});
    if (host) {                          // host frames go through the frame workspace in batches that fit it, as quality.cpp's do
        const size_t budget = std::max<size_t>(ctx->frames.cap, (size_t)ctx->opt_upload_batch * fb);
        batch = (int)std::min<size_t>((size_t)batch, std::max<size_t>(1, budget / fb));
        HIP_TRY(ctx->frames.reserve(fb * (size_t)batch));
    }
    const size_t n_ptrs = host ? (size_t)batch : (size_t)n;
    const size_t off_origin = (n_ptrs * sizeof(void*) + 15) & ~(size_t)15;
    const size_t off_hist = (off_origin + (size_t)batch * 4 * sizeof(int32_t) + 255) & ~(size_t)255;
    HIP_TRY(ctx->quality.reserve(off_hist + (size_t)batch * per_frame));
    const void** ptrs_dev = ctx->quality.as<const void*>();
    int32_t* origin = reinterpret_cast<int32_t*>(ctx->quality.as<uint8_t>() + off_origin);
    uint32_t* hist_dev = reinterpret_cast<uint32_t*>(ctx->quality.as<uint8_t>() + off_hist);
    std::vector<const void*> ptrs(n_ptrs);                         // (outlives the copy: the call synchronises below)
    for (size_t i = 0; i < n_ptrs; i++) ptrs[i] = host ? (const void*)(ctx->frames.as<uint8_t>() + fb * i) : src[i];
    double total = 0.0;
    HIP_TRY(hipMemcpyAsync(ptrs_dev, ptrs.data(), n_ptrs * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    for (int b0 = 0; b0 < n; b0 += batch) {
        const int nb = std::min(batch, n - b0);
        HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
        if (host)      // stream order keeps the previous batch's kernels ahead of the copies that overwrite its frames
            for (int i = 0; i < nb; i++)
                HIP_TRY(hipMemcpyAsync(ctx->frames.as<uint8_t>() + fb * (size_t)i, src[b0 + i], copy_bytes, hipMemcpyHostToDevice, ctx->stream));
        // no result may depend on what the workspace held: the histograms are zeroed here, on the call's stream
        HIP_TRY(hipMemsetAsync(hist_dev, 0, (size_t)nb * per_frame, ctx->stream));
        HIP_TRY(launch_noise_hist(ptrs_dev + (host ? 0 : b0), nb, cn, depth, w, h, rb, hist_dev, origin, ctx->stream));
        HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
        HIP_TRY(hipMemcpyAsync(hist + (size_t)b0 * cn * bins, hist_dev, (size_t)nb * per_frame, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        total += ev_ms(ctx->ev[0], ctx->ev[1]);
    }
    if (ms) *ms = total;
    return STK_OK;
}

// the reduction of every (frame, channel)'s histograms: stats is n x 4, the unused channel slots zeroed
void noise_reduce(const uint32_t* hist, int n, int cn, int depth, stk_noise_stat* stats) {
    const int bv = depth == 8 ? 256 : 65536, br = (int)noise_hist_bins(depth) - bv;
    std::memset(stats, 0, sizeof(stk_noise_stat) * (size_t)n * 4);
    for (int i = 0; i < n; i++)
        for (int c = 0; c < cn; c++) {
            const uint32_t* hv = hist + ((size_t)i * cn + c) * (size_t)(bv + br);
            noise::from_hist(hv, bv, hv + bv, br, depth == 16, &stats[(size_t)i * 4 + c]);
        }
}

stk_status noise_frames(stk_ctx* ctx, const void* const* src, bool host, int n, int cn, int depth, int w, int h, size_t rb,
                        size_t copy_bytes, stk_noise_stat* stats, uint32_t* hist_out, double* ms) {
    std::vector<uint32_t> own;
    if (!hist_out) { own.resize((size_t)n * cn * noise_hist_bins(depth)); hist_out = own.data(); }
    stk_status st = noise_histograms(ctx, src, host, n, cn, depth, w, h, rb, copy_bytes, hist_out, ms);
    if (st) return st;
    noise_reduce(hist_out, n, cn, depth, stats);
    return STK_OK;
}

// the checks the two whole-stack forms share, in the order the errors are reported
stk_status noise_match_check(stk_ctx* ctx, const stk_frames* frames, const stk_weight_params* weight, double sigma_floor,
                             const stk_image_f32* out) {
    stk_status st = weighted_validate(ctx, weight);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = noise_check(ctx, frames))) return st;
    if (!std::isfinite(sigma_floor) || !(sigma_floor > 0.0)) return fail(ctx, STK_INVALID_PARAMS, "noise weights: sigma_floor must be finite and > 0");
    return combine_check_out(ctx, out, frames);
}

stk_status noise_match_reserve(stk_ctx* ctx, const stk_frames* frames, const stk_weight_params* weight) {
    (void)hipSetDevice(ctx->device);
    const int step = weight->normalize ? (weight->stat_step ? weight->stat_step : 4) : 0;
    return workspace_reserve(ctx, ctx->weighted, weighted_layout(frames->n, frames->width, frames->height, frames->channels, step).total, "weighted");
}

// the combine over the kept frames: the weighted form's records, the noise pass over the resident frames, the weights, one
// weighted fold — each of them the very code of the call that stands alone
CombineFinish noise_match_finish(stk_ctx* ctx, const stk_frames* frames, const stk_weight_params* weight, const float* weights,
                                 double sigma_floor, stk_image_f32* out, float* coverage_out, stk_frame_weight* applied,
                                 stk_noise_stat* noise_out) {
    return [=](const EntryTable& table, const std::vector<const void*>& dev, const FoldSpec& spec, const stk_frame_stats*, double* ms) {
        const int n = frames->n, cn = spec.cn;
        std::vector<stk_frame_weight> coef, rec((size_t)n);
        stk_status st = weighted_match_records(ctx, n, table, spec, weight, nullptr, coef, rec.data(), ms);
        if (st) return st;
        std::vector<stk_noise_stat> own;
        stk_noise_stat* ns = noise_out;
        if (!ns) { own.resize((size_t)n * 4); ns = own.data(); }
        double pass_ms = 0.0;
        if ((st = noise_frames(ctx, dev.data(), false, n, cn, frames->depth, spec.w, spec.h, spec.src_row_bytes, 0, ns, nullptr, &pass_ms))) return st;
        *ms += pass_ms;
        std::vector<int32_t> include((size_t)n, 0);
        for (int i : table.frame) include[i] = 1;
        std::vector<float> wout((size_t)n);
        if ((st = noise::weights(ns, n, cn, rec.data(), include.data(), weights, sigma_floor, wout.data())))
            return fail(ctx, st, "noise weights: weights must be finite and >= 0, and a frame's gains may not all be 0");
        for (size_t k = 0; k < coef.size(); k++) coef[k].weight = wout[table.frame[k]];
        if ((st = weighted_check_coefs(ctx, coef, cn))) return st;
        if (applied) {
            std::memcpy(applied, rec.data(), sizeof(stk_frame_weight) * (size_t)n);
            for (size_t k = 0; k < coef.size(); k++) applied[table.frame[k]] = coef[k];
        }
        return weighted_fold_records(ctx, coef, spec, weight->coverage, out, coverage_out, ms);
    };
}

}  // namespace

extern "C" {

stk_status stk_noise_from_hist(const uint32_t* hv, int32_t bv, const uint32_t* hr, int32_t br, int32_t overflow_bin, stk_noise_stat* out) {
    return noise::from_hist(hv, bv, hr, br, overflow_bin, out);
}

stk_status stk_noise_weights(const stk_noise_stat* stats, int32_t n, int32_t channels, const stk_frame_weight* records_or_null,
                             const int32_t* include_or_null, const float* weights_or_null, double sigma_floor, float* weights_out) {
    return noise::weights(stats, n, channels, records_or_null, include_or_null, weights_or_null, sigma_floor, weights_out);
}

stk_status stk_stack_noise(stk_ctx* ctx, const stk_frames* frames, stk_noise_stat* stats, uint32_t* hist_or_null) {
    stk_status st = check_frames(ctx, frames, false, false);
    if (st) return st;
    if (!stats) return fail(ctx, STK_INVALID_PARAMS, "null noise statistics");
    if ((st = noise_check(ctx, frames))) return st;
    timing_begin(ctx);
    double ms = 0.0;
    if ((st = noise_frames(ctx, frames->data, frames->location == STK_HOST, frames->n, frames->channels, frames->depth, frames->width,
                           frames->height, frame_row_bytes(frames), frame_copy_bytes(frames), stats, hist_or_null, &ms)))
        return st;
    ctx->timing.prep_ms = ms;
    return STK_OK;
}

stk_status stk_ecc_match_noise_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                        const stk_weight_params* weight, const float* weights, double sigma_floor, stk_image_f32* out,
                                        float* coverage_out, stk_frame_weight* applied, stk_frame_stats* stats, stk_noise_stat* noise) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = noise_match_check(ctx, frames, weight, sigma_floor, out);
    if (st) return st;
    if ((st = noise_match_reserve(ctx, frames, weight))) return st;
    return ecc_match_then(ctx, frames, params, scale_down_width, ctx->weighted.as<float>(), stats,
                          noise_match_finish(ctx, frames, weight, weights, sigma_floor, out, coverage_out, applied, noise));
}

stk_status stk_keypoint_match_noise_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                             float scale_down_width, const stk_weight_params* weight, const float* weights,
                                             double sigma_floor, stk_image_f32* out, int32_t* dropped, float* coverage_out,
                                             stk_frame_weight* applied, stk_frame_stats* stats, stk_noise_stat* noise) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = noise_match_check(ctx, frames, weight, sigma_floor, out);
    if (st) return st;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null parameters");
    if (weight->coverage && (st = weighted_check_border(ctx, params->border_mode, params->border_value, 1))) return st;
    if ((st = noise_match_reserve(ctx, frames, weight))) return st;
    return keypoint_match_then(ctx, frames, params, scale_down_width, ctx->weighted.as<float>(), dropped, stats,
                               noise_match_finish(ctx, frames, weight, weights, sigma_floor, out, coverage_out, applied, noise));
}

}  // extern "C"
