// wavelet.cpp — the a trous wavelet layers of a finished stack: stk_wavelet_process, stk_wavelet_layers, stk_wavelet_sigma
// and stk_wavelet_noise_table (an extension beyond the reference; definition in include/stacker.h, "wavelet layers"; kernels
// in post/kernels_wavelet.hip, the host half in wavelet_host.h).
// ctx->local (WaveletLayout, workspace.h) holds the selection's words, the planar work images (two c planes, acc), the copy
// of a host image, the copy of a host mask and the staged outputs of a host image. A host image is uploaded once and each
// result goes back with one strided copy that writes the pixel bytes of each row and nothing else. The levels read and write
// the work images; only the last one reads the image again (D, where the blend needs it) and writes the output, each thread
// its own pixel, so `out` may be the input itself.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "context.h"
#include "spans.h"
#include "wavelet_host.h"

using namespace stk;

namespace {

enum WvForm { WV_PROCESS, WV_LAYERS, WV_SIGMA };

// The form of the level launches at spacings up to WV_STAGED_MAX_S: the one that measured faster. The
// environment variable STK_WAVELET_FORM ("direct" or "staged"), read at every call, overrides it: the hook by which the tests
// run both forms against the restatement and tools/wavelet_time.py times them side by side in one process.
constexpr int WV_FORM_DEFAULT = WV_FORM_DIRECT;
int wv_level_form() {
    const char* e = std::getenv("STK_WAVELET_FORM");
    if (e && !std::strcmp(e, "staged")) return WV_FORM_STAGED;
    if (e && !std::strcmp(e, "direct")) return WV_FORM_DIRECT;
    return WV_FORM_DEFAULT;
}

stk_status wv_image_check(stk_ctx* ctx, const stk_image_f32* im, const char* what) {
    if (!im || !im->data) return fail(ctx, STK_INVALID_PARAMS, std::string("wavelet: null ") + what);
    if (im->width <= 0 || im->height <= 0 || (im->channels != 1 && im->channels != 3 && im->channels != 4))
        return fail(ctx, STK_INVALID_PARAMS, std::string("wavelet: bad geometry of the ") + what + " (1, 3 or 4 channels)");
    if ((size_t)im->width * im->height > (size_t)1 << 30) return fail(ctx, STK_INVALID_PARAMS, std::string("wavelet: the ") + what + " is too large");
    if (im->location != STK_HOST && im->location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, std::string("wavelet: bad location of the ") + what);
    if (im->row_stride_bytes && (im->row_stride_bytes % 4 || im->row_stride_bytes < (size_t)im->width * im->channels * 4))
        return fail(ctx, STK_INVALID_PARAMS, std::string("wavelet: bad row stride of the ") + what);
    return STK_OK;
}

// the three forms: p is null for the layers and the sigma form; outs: n_out images (process 1, layers levels + 1, sigma 0)
stk_status wv_run(stk_ctx* ctx, WvForm form, const stk_image_f32* in, const stk_wavelet_params* p, int levels, const float* mask,
                  size_t mask_stride_bytes, int32_t mask_location, stk_image_f32* outs, int n_out, float* sigma_out, float* median_out) {
    stk_status st = wv_image_check(ctx, in, "image");
    if (st) return st;
    const int w = in->width, h = in->height, cn = in->channels, cc = std::min(cn, 3);
    if (form == WV_PROCESS) {
        if (const char* e = wavelet::validate(p, w, h)) return fail(ctx, STK_INVALID_PARAMS, e);
    } else {
        if (levels < 1 || levels > wavelet::MAX_LEVELS) return fail(ctx, STK_INVALID_PARAMS, "wavelet: levels must be 1 .. 8");
        if (w < (1 << levels) + 1 || h < (1 << levels) + 1) return fail(ctx, STK_INVALID_PARAMS, "wavelet: width and height must be at least 2^levels + 1");
    }
    if (n_out && !outs) return fail(ctx, STK_INVALID_PARAMS, "wavelet: null output");
    for (int k = 0; k < n_out; k++) {
        if ((st = wv_image_check(ctx, &outs[k], "output"))) return st;
        if (outs[k].width != w || outs[k].height != h || outs[k].channels != cn || outs[k].location != in->location)
            return fail(ctx, STK_INVALID_PARAMS, "wavelet: the output must have the image's geometry and location");
    }
    const size_t mrow = (size_t)w * 4, mstride = mask_stride_bytes ? mask_stride_bytes : mrow;
    if (mask) {
        if (mask_location != STK_HOST && mask_location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, "wavelet: bad location of the mask");
        if (mstride < mrow || mstride % 4) return fail(ctx, STK_INVALID_PARAMS, "wavelet: bad row stride of the mask");
    }

    // the output of the process form may be the input itself; any other overlap with what the call reads, or with another
    // output, in the same memory space is refused
    const size_t row = (size_t)w * cn * 4, istride = image_stride_floats(in) * 4;
    const size_t ispan = istride * (size_t)(h - 1) + row;
    const bool in_place = form == WV_PROCESS && outs[0].data == in->data && image_stride_floats(&outs[0]) * 4 == istride;
    {
        SpanSet reads;
        if (!in_place) reads.add(in->data, ispan);
        if (mask && mask_location == in->location) reads.add(mask, mstride * (size_t)(h - 1) + mrow);
        reads.seal();
        for (int k = 0; k < n_out; k++) {
            const size_t ospan = image_stride_floats(&outs[k]) * 4 * (size_t)(h - 1) + row;
            if (reads.overlaps(outs[k].data, ospan))
                return fail(ctx, STK_INVALID_PARAMS, "wavelet: an output overlaps the image or the mask (it may only be the image itself: same pointer, same row stride)");
            SpanSet mine;
            mine.add(outs[k].data, ospan);
            mine.seal();
            for (int m = k + 1; m < n_out; m++)
                if (mine.overlaps(outs[m].data, image_stride_floats(&outs[m]) * 4 * (size_t)(h - 1) + row))
                    return fail(ctx, STK_INVALID_PARAMS, "wavelet: two outputs overlap");
        }
    }

    double e[wavelet::MAX_LEVELS];
    (void)wavelet::noise_table(wavelet::MAX_LEVELS, e);
    const bool estimate = form == WV_SIGMA || (form == WV_PROCESS && !p->sigma_given && (sigma_out || wavelet::needs_estimate(p)));

    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    const bool host = in->location == STK_HOST, mask_host = mask && mask_location == STK_HOST;
    const size_t image_bytes = row * (size_t)h;
    const WaveletLayout L = wavelet_layout(w, h, cc, host ? image_bytes : 0, mask_host ? mrow * (size_t)h : 0, host ? image_bytes * (size_t)n_out : 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "wavelet"))) return st;
    char* base = ctx->local.as<char>();

    const float* src = in->data;
    size_t src_stride = istride / 4;
    if (host) {
        HIP_TRY(hipMemcpy2DAsync(base + L.image, row, in->data, istride, row, h, hipMemcpyHostToDevice, ctx->stream));
        src = (const float*)(base + L.image); src_stride = row / 4;
    }
    const float* dmask = mask;
    size_t dmask_stride = mstride / 4;
    if (mask_host) {
        HIP_TRY(hipMemcpy2DAsync(base + L.mask, mrow, mask, mstride, mrow, h, hipMemcpyHostToDevice, ctx->stream));
        dmask = (const float*)(base + L.mask); dmask_stride = (size_t)w;
    }
    float* dout[wavelet::MAX_LEVELS + 1] = {};
    size_t dout_stride[wavelet::MAX_LEVELS + 1] = {};
    for (int k = 0; k < n_out; k++) {
        dout[k] = host ? (float*)(base + L.out + image_bytes * (size_t)k) : outs[k].data;
        dout_stride[k] = host ? row / 4 : image_stride_floats(&outs[k]);
    }

    // the first bracket: the initialisation and, where needed, the selection
    HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    WvInitArgs ia{};
    ia.in = src; ia.c0 = (float*)(base + L.c[0]);
    ia.in_stride = src_stride; ia.plane = L.plane / 4; ia.w = w; ia.h = h;
    ia.n_alpha = cn == 4 ? n_out : 0;
    for (int k = 0; k < ia.n_alpha; k++) { ia.alpha[k] = dout[k]; ia.alpha_stride[k] = dout_stride[k]; }
    HIP_TRY(launch_wavelet_init(ia, cn, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
    float sigma[4] = {0.0f, 0.0f, 0.0f, 0.0f}, median[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    double est_ms = 0.0;
    if (estimate) {
        WvSelectArgs sa{};
        sa.c0 = ia.c0; sa.state = (uint32_t*)(base + L.state);
        sa.plane = L.plane / 4; sa.w = w; sa.h = h; sa.channels = cc;
        sa.rank = (uint32_t)(((size_t)w * h + 1) / 2);
        HIP_TRY(launch_wavelet_select_reset(sa, ctx->stream));
        for (int r = 0; r < WV_ROUNDS; r++) {
            sa.round = r;
            HIP_TRY(launch_wavelet_select_hist(sa, ctx->stream));
            HIP_TRY(launch_wavelet_select_pick(sa, ctx->stream));
        }
        HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
        uint32_t words[6] = {};
        HIP_TRY(hipMemcpyAsync(words, sa.state, (size_t)cc * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        est_ms = ev_ms(ctx->ev[1], ctx->ev[2]);
        for (int c = 0; c < cc; c++) {
            std::memcpy(&median[c], &words[2 * c], sizeof(float));
            sigma[c] = wavelet::sigma_from_median(median[c], e[0]);
        }
    } else if (form == WV_PROCESS && p->sigma_given) {
        for (int c = 0; c < cc; c++) sigma[c] = p->sigma[c];
    }
    if (sigma_out) std::memcpy(sigma_out, sigma, sizeof(sigma));
    if (median_out) std::memcpy(median_out, median, sizeof(median));

    // the second bracket: the levels
    HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    if (form != WV_SIGMA) {
        float t[3][wavelet::MAX_LEVELS] = {};
        if (form == WV_PROCESS)
            for (int c = 0; c < cc; c++) wavelet::thresholds(p, sigma[c], e, t[c]);
        WvLevelArgs a{};
        a.acc = (float*)(base + L.acc);
        a.in = src; a.in_stride = src_stride; a.mask = dmask; a.mask_stride = dmask_stride;
        a.plane = L.plane / 4; a.w = w; a.h = h; a.cn = cn; a.channels = cc;
        a.layers = form == WV_LAYERS;
        a.form = wv_level_form();
        if (form == WV_PROCESS) {
            a.out = dout[0]; a.out_stride = dout_stride[0];
            a.mode = p->mode; a.residual_gain = p->residual_gain; a.amount = p->amount;
        }
        for (int j = 0; j < levels; j++) {
            a.src = (const float*)(base + L.c[j & 1]);
            a.dst = (float*)(base + L.c[(j + 1) & 1]);
            a.s = 1 << j; a.first = j == 0; a.last = j == levels - 1;
            if (form == WV_PROCESS) {
                for (int c = 0; c < cc; c++) a.t[c] = t[c][j];
                a.layer_amount = p->layer_amount[j]; a.keep = 1.0f - p->layer_amount[j]; a.gain = p->gain[j];
            } else {
                a.wout = dout[j]; a.wout_stride = dout_stride[j];
                a.cout = dout[levels]; a.cout_stride = dout_stride[levels];
            }
            // the last level and the last inner level (it writes c_{j+1} and acc) are timed on their own too
            if (j == levels - 2) HIP_TRY(hipEventRecord(ctx->ev[6], ctx->stream));
            if (a.last) HIP_TRY(hipEventRecord(levels > 1 ? ctx->ev[7] : ctx->ev[3], ctx->stream));
            if (a.last && levels > 1) HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));
            HIP_TRY(launch_wavelet_level(a, ctx->stream));
        }
    }
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    if (host)
        for (int k = 0; k < n_out; k++)
            HIP_TRY(hipMemcpy2DAsync(outs[k].data, image_stride_floats(&outs[k]) * 4, dout[k], row, row, h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.finalize_ms = ev_ms(ctx->ev[0], ctx->ev[1]) + est_ms + ev_ms(ctx->ev[4], ctx->ev[5]);
    ctx->timing.prep_ms = est_ms;
    ctx->timing.warp_ms = form != WV_SIGMA ? ev_ms(ctx->ev[3], ctx->ev[5]) : 0.0;
    ctx->timing.align_ms = form != WV_SIGMA && levels > 1 ? ev_ms(ctx->ev[6], ctx->ev[7]) : 0.0;
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_wavelet_noise_table(int32_t levels, double* e) { return wavelet::noise_table(levels, e); }

stk_status stk_wavelet_process(stk_ctx* ctx, const stk_image_f32* in, const stk_wavelet_params* p, const float* mask, size_t mask_stride_bytes,
                               int32_t mask_location, stk_image_f32* out, float* sigma_out) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null wavelet parameters");
    if (!out) return fail(ctx, STK_INVALID_PARAMS, "wavelet: null output");
    return wv_run(ctx, WV_PROCESS, in, p, p->levels, mask, mask_stride_bytes, mask_location, out, 1, sigma_out, nullptr);
}

stk_status stk_wavelet_layers(stk_ctx* ctx, const stk_image_f32* in, int32_t levels, stk_image_f32* out) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (levels < 1 || levels > wavelet::MAX_LEVELS) return fail(ctx, STK_INVALID_PARAMS, "wavelet: levels must be 1 .. 8");
    return wv_run(ctx, WV_LAYERS, in, nullptr, levels, nullptr, 0, 0, out, levels + 1, nullptr, nullptr);
}

stk_status stk_wavelet_sigma(stk_ctx* ctx, const stk_image_f32* in, float* sigma, float* median) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!sigma) return fail(ctx, STK_INVALID_PARAMS, "wavelet: null sigma");
    return wv_run(ctx, WV_SIGMA, in, nullptr, 1, nullptr, 0, 0, nullptr, 0, sigma, median);
}

}  // extern "C"
