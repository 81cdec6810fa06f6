// deconvolve.cpp — Richardson-Lucy deconvolution of a finished stack: stk_deconvolve, stk_psf_model and
// stk_psf_from_shapes (an extension beyond the reference; definition in include/stacker.h, "deconvolution"; kernels in
// kernels_deconvolve.hip, the PSF functions in psf_host.h).
// ctx->local (DeconvLayout, workspace.h) holds the padded tap table, the planar work images (D, two u planes, r), the copy
// of a host image, the copy of a host mask and the staged output of a host image. A host image is uploaded once and the
// result goes back with one strided copy that writes the pixel bytes of each row and nothing else. The iterations read and
// write the work images only, so `out` may be the input itself.
#include <cmath>
#include <cstring>

#include "context.h"
#include "psf_host.h"
#include "spans.h"

using namespace stk;

namespace {

stk_status dcv_image_check(stk_ctx* ctx, const stk_image_f32* im, const char* what) {
    if (!im || !im->data) return fail(ctx, STK_INVALID_PARAMS, std::string("deconvolve: null ") + what);
    if (im->width <= 0 || im->height <= 0 || (im->channels != 1 && im->channels != 3 && im->channels != 4))
        return fail(ctx, STK_INVALID_PARAMS, std::string("deconvolve: bad geometry of the ") + what + " (1, 3 or 4 channels)");
    if ((size_t)im->width * im->height > (size_t)1 << 30) return fail(ctx, STK_INVALID_PARAMS, std::string("deconvolve: the ") + what + " is too large");
    if (im->location != STK_HOST && im->location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, std::string("deconvolve: bad location of the ") + what);
    if (im->row_stride_bytes && (im->row_stride_bytes % 4 || im->row_stride_bytes < (size_t)im->width * im->channels * 4))
        return fail(ctx, STK_INVALID_PARAMS, std::string("deconvolve: bad row stride of the ") + what);
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_psf_model(int32_t kind, double beta, int32_t radius, double cxx, double cyy, double cxy, float* psf) {
    return psf::model(kind, beta, radius, cxx, cyy, cxy, psf);
}

stk_status stk_psf_from_shapes(const stk_star_shape* shapes, int32_t count, double min_snr, double scale, double* cxx, double* cyy,
                               double* cxy, int32_t* used) {
    return psf::from_shapes(shapes, count, min_snr, scale, cxx, cyy, cxy, used);
}

stk_status stk_deconvolve(stk_ctx* ctx, const stk_image_f32* in, const float* taps, const stk_deconv_params* p, const float* mask,
                          size_t mask_stride_bytes, int32_t mask_location, stk_image_f32* out) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = dcv_image_check(ctx, in, "image");
    if (st) return st;
    if ((st = dcv_image_check(ctx, out, "output"))) return st;
    const int w = in->width, h = in->height, cn = in->channels, cc = std::min(cn, 3);
    if (out->width != w || out->height != h || out->channels != cn || out->location != in->location)
        return fail(ctx, STK_INVALID_PARAMS, "deconvolve: the output must have the image's geometry and location");
    if (const char* e = psf::validate(p, w, h)) return fail(ctx, STK_INVALID_PARAMS, e);
    if (const char* e = psf::validate_taps(taps, p->radius)) return fail(ctx, STK_INVALID_PARAMS, e);
    const size_t mrow = (size_t)w * 4, mstride = mask_stride_bytes ? mask_stride_bytes : mrow;
    if (mask) {
        if (mask_location != STK_HOST && mask_location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, "deconvolve: bad location of the mask");
        if (mstride < mrow || mstride % 4) return fail(ctx, STK_INVALID_PARAMS, "deconvolve: bad row stride of the mask");
    }
    if ((h + DCV_TH - 1) / DCV_TH > 65535) return fail(ctx, STK_NOT_IMPLEMENTED, "deconvolve: images above 65535 tile rows");

    // the output may be the input itself; any other overlap with what the call reads in the same memory space is refused
    const size_t row = (size_t)w * cn * 4, istride = image_stride_floats(in) * 4, ostride = image_stride_floats(out) * 4;
    const size_t ispan = istride * (size_t)(h - 1) + row, ospan = ostride * (size_t)(h - 1) + row;
    const bool in_place = out->data == in->data && ostride == istride;
    {
        SpanSet reads;
        if (!in_place) reads.add(in->data, ispan);
        if (mask && mask_location == in->location) reads.add(mask, mstride * (size_t)(h - 1) + mrow);
        reads.seal();
        if (reads.overlaps(out->data, ospan))
            return fail(ctx, STK_INVALID_PARAMS, "deconvolve: the output overlaps the image or the mask (it may only be the image itself: same pointer, same row stride)");
    }

    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    const bool host = in->location == STK_HOST, mask_host = mask && mask_location == STK_HOST;
    const DeconvLayout L = deconv_layout(p->radius, w, h, cc, host ? row * (size_t)h : 0, mask_host ? mrow * (size_t)h : 0, host ? row * (size_t)h : 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "deconvolve"))) return st;
    char* base = ctx->local.as<char>();

    std::vector<float> table(dcv_tap_floats(p->radius));                  // (outlives its copy: the call synchronises)
    dcv_pad_taps(taps, p->radius, table.data());
    HIP_TRY(hipMemcpyAsync(base + L.taps, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
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
    float* dout = host ? (float*)(base + L.out) : out->data;
    const size_t dout_stride = host ? row / 4 : ostride / 4;

    if ((st = combine_begin(ctx))) return st;                             // the timed bracket: the launches alone
    DeconvInitArgs ia{};
    ia.in = src; ia.out = dout; ia.D = (float*)(base + L.D);
    ia.in_stride = src_stride; ia.out_stride = dout_stride; ia.plane = L.plane / 4;
    ia.w = w; ia.h = h; ia.pedestal = p->pedestal;
    HIP_TRY(launch_deconv_init(ia, cn, ctx->stream));
    DeconvPassArgs a{};
    a.taps = (const float*)(base + L.taps);
    a.D = (const float*)(base + L.D);
    a.out = dout; a.mask = dmask;
    a.out_stride = dout_stride; a.mask_stride = dmask_stride; a.plane = L.plane / 4;
    a.w = w; a.h = h; a.cn = cn; a.channels = cc; a.radius = p->radius;
    a.floor = p->floor; a.lambda = p->lambda; a.e2 = p->tv_eps * p->tv_eps; a.amount = p->amount; a.pedestal = p->pedestal;
    const float* u = a.D;                                                 // u_0 = D
    for (int k = 0; k < p->iterations; k++) {
        float* r = (float*)(base + L.r);
        float* next = (float*)(base + L.u[k & 1]);
        const bool last = k == p->iterations - 1;                         // its two launches are timed each on its own
        a.src = u; a.u = u; a.dst = r; a.last = 0;
        if (last) HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
        HIP_TRY(launch_deconv_ratio(a, ctx->stream));
        if (last) HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
        a.src = r; a.dst = next; a.last = last;
        HIP_TRY(launch_deconv_update(a, ctx->stream));
        u = next;
    }
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    if (host) HIP_TRY(hipMemcpy2DAsync(out->data, ostride, dout, row, row, h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.finalize_ms = ev_ms(ctx->ev[4], ctx->ev[5]);
    ctx->timing.prep_ms = ev_ms(ctx->ev[0], ctx->ev[1]);
    ctx->timing.warp_ms = ev_ms(ctx->ev[1], ctx->ev[5]);
    return STK_OK;
}

}  // extern "C"
