// calibrate.cpp — frame calibration: stk_calibrate, stk_defect_map, stk_image_mean, stk_master_stack (an extension beyond
// the reference; definition in include/stacker.h, stk_calibration; kernels in kernels_calibrate.hip).
// stk_calibrate keeps a device-resident stack where it is: one launch over tiles x frame chunks reads the frames and writes
// the caller's outputs. Host frames go through ctx->frames, their outputs through a staging block of ctx->local
// and back with one strided copy per frame, which writes the pixel bytes of each row and nothing else. Host masters and a
// host map are copied once per call into ctx->local (CalLayout, workspace.h). stk_master_stack is host composition of two
// existing entry points and owns no kernel.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"
#include "spans.h"

using namespace stk;

namespace {

stk_status master_check(stk_ctx* ctx, const stk_image_f32* m, const stk_frames* f, const char* what) {
    if (!m) return STK_OK;
    if (!m->data) return fail(ctx, STK_INVALID_PARAMS, std::string("calibrate: null ") + what + " master");
    if (m->width != f->width || m->height != f->height || m->channels != f->channels)
        return fail(ctx, STK_INVALID_PARAMS, std::string("calibrate: the ") + what + " master's geometry differs from the frames'");
    if (m->location != STK_HOST && m->location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, std::string("calibrate: bad location of the ") + what + " master");
    if (m->row_stride_bytes && (m->row_stride_bytes % 4 || m->row_stride_bytes < (size_t)m->width * m->channels * 4))
        return fail(ctx, STK_INVALID_PARAMS, std::string("calibrate: bad row stride of the ") + what + " master");
    return STK_OK;
}

size_t image_span_bytes(const stk_image_f32* m) {
    return image_stride_floats(m) * 4 * (size_t)(m->height - 1) + (size_t)m->width * m->channels * 4;
}

// an f32 image the kernels can read: a device image where it lies, a host image copied tightly packed to `stage`
stk_status image_on_device(stk_ctx* ctx, const stk_image_f32* m, void* stage, const float** data, size_t* stride_floats) {
    const size_t row = (size_t)m->width * m->channels;
    if (m->location == STK_DEVICE) { *data = m->data; *stride_floats = image_stride_floats(m); return STK_OK; }
    HIP_TRY(hipMemcpy2DAsync(stage, row * 4, m->data, image_stride_floats(m) * 4, row * 4, m->height, hipMemcpyHostToDevice, ctx->stream));
    *data = (const float*)stage; *stride_floats = row;
    return STK_OK;
}

stk_status plain_image_check(stk_ctx* ctx, const stk_image_f32* im, const char* what) {
    if (!im || !im->data) return fail(ctx, STK_INVALID_PARAMS, std::string(what) + ": null image");
    if (im->width <= 0 || im->height <= 0 || (im->channels != 1 && im->channels != 3 && im->channels != 4))
        return fail(ctx, STK_INVALID_PARAMS, std::string(what) + ": bad image geometry");
    if ((size_t)im->width * im->height > (size_t)1 << 30) return fail(ctx, STK_INVALID_PARAMS, std::string(what) + ": image too large");
    if (im->location != STK_HOST && im->location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, std::string(what) + ": bad image location");
    if (im->row_stride_bytes && (im->row_stride_bytes % 4 || im->row_stride_bytes < (size_t)im->width * im->channels * 4))
        return fail(ctx, STK_INVALID_PARAMS, std::string(what) + ": bad row stride");
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_calibrate(stk_ctx* ctx, const stk_frames* frames, const stk_calibration* cal, void* const* out, size_t out_row_stride_bytes) {
    stk_status st = check_frames(ctx, frames, false, false);
    if (st) return st;
    if (!cal) return fail(ctx, STK_INVALID_PARAMS, "calibrate: null calibration");
    if (!out) return fail(ctx, STK_INVALID_PARAMS, "calibrate: null outputs");
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels, depth = frames->depth;
    for (int i = 0; i < n; i++)
        if (!out[i] || !frames->data[i]) return fail(ctx, STK_INVALID_PARAMS, "calibrate: null frame or output pointer");
    if (frames->location != STK_HOST && frames->location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, "calibrate: bad frame location");
    if (cal->out_depth != depth && cal->out_depth != STK_DEPTH_F32)
        return fail(ctx, STK_INVALID_PARAMS, depth == 32 ? "calibrate: f32 frames calibrate to STK_DEPTH_F32 only"
                                                         : "calibrate: out_depth must be the frames' depth or STK_DEPTH_F32");
    if (cal->defect_step != 1 && cal->defect_step != 2) return fail(ctx, STK_INVALID_PARAMS, "calibrate: defect_step must be 1 or 2");
    if (cal->reserved != 0 || cal->reserved2 != 0) return fail(ctx, STK_INVALID_PARAMS, "calibration: reserved must be 0");
    const stk_image_f32* masters[3] = {cal->bias_or_null, cal->dark_or_null, cal->flat_or_null};
    const char* names[3] = {"bias", "dark", "flat"};
    for (int k = 0; k < 3; k++)
        if ((st = master_check(ctx, masters[k], frames, names[k]))) return st;
    const int cc = std::min(cn, 3);
    if (cal->flat_or_null) {
        for (int c = 0; c < cc; c++)
            if (!std::isfinite(cal->flat_mean[c]) || !(cal->flat_mean[c] > 0.0f))
                return fail(ctx, STK_INVALID_PARAMS, "calibrate: flat_mean must be finite and > 0 in every colour channel");
        if (!std::isfinite(cal->flat_min) || !(cal->flat_min > 0.0f)) return fail(ctx, STK_INVALID_PARAMS, "calibrate: flat_min must be finite and > 0");
    }
    if (!std::isfinite(cal->pedestal)) return fail(ctx, STK_INVALID_PARAMS, "calibrate: pedestal must be finite");
    if (cal->dark_scale_or_null)
        for (int i = 0; i < n; i++)
            if (!std::isfinite(cal->dark_scale_or_null[i])) return fail(ctx, STK_INVALID_PARAMS, "calibrate: dark_scale must be finite");
    if (cal->defects_or_null && cal->defects_location != STK_HOST && cal->defects_location != STK_DEVICE)
        return fail(ctx, STK_INVALID_PARAMS, "calibrate: bad location of the defect map");
    const size_t oel = (size_t)cal->out_depth / 8, orow = (size_t)w * cn * oel;
    const size_t ostride = out_row_stride_bytes ? out_row_stride_bytes : orow;
    if (ostride < orow || ostride % oel) return fail(ctx, STK_INVALID_PARAMS, "calibrate: bad output row stride");
    if ((h + CAL_TH - 1) / CAL_TH > 65535) return fail(ctx, STK_NOT_IMPLEMENTED, "calibrate: frames above 262140 rows");

    // no output may overlap anything the call reads in the same memory space
    const bool host = frames->location == STK_HOST;
    {
        SpanSet in;
        for (int i = 0; i < n; i++) in.add(frames->data[i], frame_copy_bytes(frames));
        for (const stk_image_f32* m : masters)
            if (m && m->location == frames->location) in.add(m->data, image_span_bytes(m));
        if (cal->defects_or_null && cal->defects_location == frames->location) in.add(cal->defects_or_null, (size_t)w * h);
        in.seal();
        const size_t ospan = ostride * (size_t)(h - 1) + orow;
        for (int i = 0; i < n; i++)
            if (in.overlaps(out[i], ospan)) return fail(ctx, STK_INVALID_PARAMS, "calibrate: an output overlaps a frame, a master or the map (in-place calibration is not supported)");
    }

    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    const size_t rb = frame_row_bytes(frames), fb = rb * (size_t)h, ofb = orow * (size_t)h;      // staged outputs are tightly packed
    size_t mbytes[3];
    for (int k = 0; k < 3; k++) mbytes[k] = masters[k] && masters[k]->location == STK_HOST ? (size_t)w * h * cn * 4 : 0;
    const bool map_host = cal->defects_or_null && cal->defects_location == STK_HOST;
    const CalLayout L = cal_layout((size_t)n, mbytes, map_host ? (size_t)w * h : 0, host ? ofb * (size_t)n : 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "calibrate"))) return st;
    if (host && (st = workspace_reserve(ctx, ctx->frames, fb * (size_t)n, "calibrate frames"))) return st;
    char* base = ctx->local.as<char>();

    CalArgs a{};
    a.frames = (const CalFrame*)(base + L.records);
    a.chunk = ctx->opt_calibrate_chunk > 0 ? ctx->opt_calibrate_chunk : CAL_CHUNK;
    a.w = w; a.h = h;
    a.in_stride = rb;
    a.out_stride = host ? orow : ostride;
    const float** mptr[3] = {&a.bias, &a.dark, &a.flat};
    size_t* mstride[3] = {&a.bias_stride, &a.dark_stride, &a.flat_stride};
    for (int k = 0; k < 3; k++)
        if (masters[k] && (st = image_on_device(ctx, masters[k], base + L.master[k], mptr[k], mstride[k]))) return st;
    if (cal->defects_or_null) {
        if (map_host) HIP_TRY(hipMemcpyAsync(base + L.map, cal->defects_or_null, (size_t)w * h, hipMemcpyHostToDevice, ctx->stream));
        a.defects = map_host ? (const uint8_t*)(base + L.map) : cal->defects_or_null;
    }
    a.step = cal->defect_step;
    for (int c = 0; c < 4; c++) a.flat_mean[c] = cal->flat_mean[c];
    a.flat_min = cal->flat_min; a.pedestal = cal->pedestal;

    std::vector<CalFrame> rec((size_t)n);
    if ((st = combine_begin(ctx))) return st;
    for (int i = 0; i < n; i++) {
        if (host) HIP_TRY(hipMemcpyAsync(ctx->frames.as<uint8_t>() + fb * (size_t)i, frames->data[i], frame_copy_bytes(frames), hipMemcpyHostToDevice, ctx->stream));
        rec[i].src = host ? (const void*)(ctx->frames.as<uint8_t>() + fb * (size_t)i) : frames->data[i];
        rec[i].dst = host ? (void*)(base + L.out + ofb * (size_t)i) : out[i];
        rec[i].dark_scale = cal->dark_scale_or_null ? cal->dark_scale_or_null[i] : 1.0f;
        rec[i].pad = 0;
    }
    HIP_TRY(hipMemcpyAsync(base + L.records, rec.data(), (size_t)n * sizeof(CalFrame), hipMemcpyHostToDevice, ctx->stream));   // (rec outlives it: combine_end synchronises)
    for (int l0 = 0; l0 < n; l0 += a.chunk * 65535) {
        CalArgs al = a;
        al.frames = a.frames + l0;
        al.n = std::min(n - l0, a.chunk * 65535);
        HIP_TRY(launch_calibrate(al, depth, cal->out_depth, cn, ctx->stream));
    }
    if (host)
        for (int i = 0; i < n; i++)
            HIP_TRY(hipMemcpy2DAsync(out[i], ostride, base + L.out + ofb * (size_t)i, orow, orow, h, hipMemcpyDeviceToHost, ctx->stream));
    double ms = 0.0;
    if ((st = combine_end(ctx, &ms))) return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

stk_status stk_defect_map(stk_ctx* ctx, const stk_image_f32* master, const stk_defect_params* p, uint8_t* map, int32_t map_location,
                          int64_t* counts) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = plain_image_check(ctx, master, "defect map");
    if (st) return st;
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "defect map: null parameters");
    if (!map) return fail(ctx, STK_INVALID_PARAMS, "defect map: null map");
    if (map_location != STK_HOST && map_location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, "defect map: bad map location");
    if (p->tests < 1 || p->tests > 3) return fail(ctx, STK_INVALID_PARAMS, "defect map: tests must be 1 .. 3");
    if (!std::isfinite(p->high_abs) || p->high_abs < 0.0f) return fail(ctx, STK_INVALID_PARAMS, "defect map: high_abs must be finite and >= 0");
    if (!(p->low_ratio >= 0.0f && p->low_ratio <= 1.0f)) return fail(ctx, STK_INVALID_PARAMS, "defect map: low_ratio must be 0 .. 1");
    if (p->step != 1 && p->step != 2) return fail(ctx, STK_INVALID_PARAMS, "defect map: step must be 1 or 2");
    if (p->accumulate != 0 && p->accumulate != 1) return fail(ctx, STK_INVALID_PARAMS, "defect map: accumulate must be 0 or 1");
    if (p->reserved != 0) return fail(ctx, STK_INVALID_PARAMS, "defect parameters: reserved must be 0");
    const int w = master->width, h = master->height, cn = master->channels;
    if ((h + DEF_TH - 1) / DEF_TH > 65535) return fail(ctx, STK_NOT_IMPLEMENTED, "defect map: masters above 1048560 rows");
    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    const size_t nb = (size_t)w * h;
    const bool map_host = map_location == STK_HOST;
    const ImageLayout L = image_layout(0, master->location == STK_HOST ? nb * cn * 4 : 0, map_host ? nb : 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "defect map"))) return st;
    char* base = ctx->local.as<char>();
    const float* data = nullptr;
    size_t stride = 0;
    if ((st = image_on_device(ctx, master, base + L.image, &data, &stride))) return st;
    uint8_t* dmap = map_host ? (uint8_t*)(base + L.map) : map;
    if (map_host && p->accumulate) HIP_TRY(hipMemcpyAsync(dmap, map, nb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(base + L.counters, 0, 4 * sizeof(unsigned long long), ctx->stream));
    if ((st = combine_begin(ctx))) return st;
    HIP_TRY(launch_defect_map(data, stride, w, h, cn, p->tests, p->high_abs, p->low_ratio, p->step, p->accumulate, dmap,
                              (unsigned long long*)(base + L.counters), ctx->stream));
    unsigned long long got[4] = {0, 0, 0, 0};
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    if (map_host) HIP_TRY(hipMemcpyAsync(map, dmap, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(got, base + L.counters, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.finalize_ms = ev_ms(ctx->ev[4], ctx->ev[5]);
    if (counts) for (int c = 0; c < 4; c++) counts[c] = (int64_t)got[c];
    return STK_OK;
}

stk_status stk_image_mean(stk_ctx* ctx, const stk_image_f32* image, double* mean) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = plain_image_check(ctx, image, "image mean");
    if (st) return st;
    if (!mean) return fail(ctx, STK_INVALID_PARAMS, "image mean: null output");
    const int w = image->width, h = image->height, cn = image->channels;
    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    const ImageLayout L = image_layout((size_t)h, image->location == STK_HOST ? (size_t)w * h * cn * 4 : 0, 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "image mean"))) return st;
    char* base = ctx->local.as<char>();
    const float* data = nullptr;
    size_t stride = 0;
    if ((st = image_on_device(ctx, image, base + L.image, &data, &stride))) return st;
    if ((st = combine_begin(ctx))) return st;
    HIP_TRY(launch_image_sums(data, stride, w, h, cn, (double*)(base + L.partials), (double*)(base + L.counters), ctx->stream));
    double sums[4] = {0, 0, 0, 0};
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    HIP_TRY(hipMemcpyAsync(sums, base + L.counters, sizeof(sums), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.finalize_ms = ev_ms(ctx->ev[4], ctx->ev[5]);
    const double count = (double)w * (double)h;
    for (int c = 0; c < 4; c++) mean[c] = c < cn ? sums[c] / count : 0.0;
    return STK_OK;
}

stk_status stk_master_stack(stk_ctx* ctx, const stk_frames* frames, int32_t normalize, int32_t stat_step, const stk_robust_clip_params* clip,
                            stk_image_f32* out, int32_t* counts) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (normalize != 0 && normalize != 2) return fail(ctx, STK_INVALID_PARAMS, "master stack: normalize must be 0 (bias, darks) or 2 (flats)");
    if (stat_step < 0 || stat_step > 64) return fail(ctx, STK_INVALID_PARAMS, "master stack: stat_step must be 0 .. 64");
    const int n = frames->n, cn = frames->channels;
    std::vector<double> M((size_t)n * 9, 0.0);
    for (int i = 0; i < n; i++) M[(size_t)i * 9] = M[(size_t)i * 9 + 4] = M[(size_t)i * 9 + 8] = 1.0;
    const double bv[4] = {0, 0, 0, 0};
    std::vector<stk_frame_weight> rec((size_t)n);
    for (stk_frame_weight& r : rec) { weighted_estimate(nullptr, cn, 0, &r); r.weight = 1.0f; }
    if (normalize == 2 && n > 1) {
        std::vector<double> mom((size_t)n * cn * 6, 0.0);
        if ((st = stk_overlap_moments(ctx, frames, M.data(), nullptr, 0, STK_BORDER_CONSTANT, bv, 1.0, stat_step ? stat_step : 4, mom.data()))) return st;
        for (int i = 1; i < n; i++) { weighted_estimate(mom.data() + (size_t)i * cn * 6, cn, 2, &rec[i]); rec[i].weight = 1.0f; }
    }
    return stk_robust_clip_stack_weighted(ctx, frames, M.data(), nullptr, 0, STK_BORDER_CONSTANT, bv, 1.0, clip, rec.data(), 0, out, counts, nullptr);
}

}  // extern "C"
