// demosaic.cpp — colour-filter mosaics: stk_demosaic, stk_cfa_mask (an extension beyond the reference; definition in
// include/stacker.h, stk_mosaic; kernels in kernels_demosaic.hip). A device-resident stack of mosaics stays where it is: one
// launch over tiles x frames reads the planes and writes the caller's outputs. Host mosaics go through ctx->frames, their
// outputs through a staging block of ctx->local (DemosaicLayout, workspace.h) and back with one strided copy per frame,
// which writes the pixel bytes of each row and nothing else.
#include "context.h"
#include "demosaic_check.h"

using namespace stk;

extern "C" {

stk_status stk_demosaic(stk_ctx* ctx, const stk_mosaic* mosaic, int32_t method, int32_t out_depth, void* const* out,
                        size_t out_row_stride_bytes) {
    if (!ctx) return STK_INVALID_PARAMS;
    DemosaicPlan P{};
    std::string why;
    if (stk_status st = demosaic_check(mosaic, method, out_depth, out, out_row_stride_bytes, &P, &why)) return fail(ctx, st, why);
    const int n = mosaic->n, w = mosaic->width, h = mosaic->height;
    const bool host = mosaic->location == STK_HOST;

    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    stk_status st;
    const size_t fb = P.in_stride * (size_t)h, ofb = P.out_row * (size_t)P.oh;               // staged outputs are tightly packed
    const DemosaicLayout L = demosaic_layout((size_t)n, host ? ofb * (size_t)n : 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "demosaic"))) return st;
    if (host && (st = workspace_reserve(ctx, ctx->frames, fb * (size_t)n, "demosaic frames"))) return st;
    char* base = ctx->local.as<char>();

    DemArgs a{};
    a.frames = (const DemFrame*)(base + L.records);
    a.n = n; a.w = w; a.h = h;
    a.pattern = mosaic->pattern;
    a.in_stride = P.in_stride;
    a.out_stride = host ? P.out_row : P.out_stride;
    std::vector<DemFrame> rec((size_t)n);
    if ((st = combine_begin(ctx))) return st;
    for (int i = 0; i < n; i++) {
        if (host) HIP_TRY(hipMemcpyAsync(ctx->frames.as<uint8_t>() + fb * (size_t)i, mosaic->data[i], P.in_span, hipMemcpyHostToDevice, ctx->stream));
        rec[i].src = host ? (const void*)(ctx->frames.as<uint8_t>() + fb * (size_t)i) : mosaic->data[i];
        rec[i].dst = host ? (void*)(base + L.out + ofb * (size_t)i) : out[i];
    }
    HIP_TRY(hipMemcpyAsync(base + L.records, rec.data(), (size_t)n * sizeof(DemFrame), hipMemcpyHostToDevice, ctx->stream));   // (rec outlives it: combine_end synchronises)
    HIP_TRY(launch_demosaic(a, mosaic->depth, out_depth, method, ctx->stream));
    if (host)
        for (int i = 0; i < n; i++)
            HIP_TRY(hipMemcpy2DAsync(out[i], P.out_stride, base + L.out + ofb * (size_t)i, P.out_row, P.out_row, P.oh, hipMemcpyDeviceToHost, ctx->stream));
    double ms = 0.0;
    if ((st = combine_end(ctx, &ms))) return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

stk_status stk_cfa_mask(stk_ctx* ctx, int32_t width, int32_t height, int32_t pattern, int32_t channel, float* plane, int32_t location) {
    if (!ctx) return STK_INVALID_PARAMS;
    std::string why;
    if (stk_status st = cfa_mask_check(width, height, pattern, channel, plane, location, &why)) return fail(ctx, st, why);
    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    stk_status st;
    const bool host = location == STK_HOST;
    const size_t bytes = (size_t)width * height * sizeof(float);
    const DemosaicLayout L = demosaic_layout(0, host ? bytes : 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "cfa mask"))) return st;
    float* dst = host ? (float*)(ctx->local.as<char>() + L.out) : plane;
    if ((st = combine_begin(ctx))) return st;
    HIP_TRY(launch_cfa_mask(dst, width, height, pattern, channel, ctx->stream));
    if (host) HIP_TRY(hipMemcpyAsync(plane, dst, bytes, hipMemcpyDeviceToHost, ctx->stream));
    double ms = 0.0;
    if ((st = combine_end(ctx, &ms))) return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

}  // extern "C"
