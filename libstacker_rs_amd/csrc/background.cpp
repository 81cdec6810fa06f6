// background.cpp — the background model: stk_background_cells, stk_background_estimate, stk_background_apply and
// stk_background_flatten (an extension beyond the reference; definition in include/stacker.h, stk_background_params; kernels
// in kernels_background.hip, the estimator in background_host.h).
// A device-resident stack stays where it is; host frames go through ctx->frames once per call (the whole-stack form runs
// both launches on that one copy). ctx->local (BgLayout, workspace.h) holds the frame pointer table of the cells launch, the
// per-frame records of the apply launch, the copy of a host mask, the window records, the level planes and the tightly
// packed outputs of host frames, which go back with one strided copy per frame that writes the pixel bytes of each row and
// nothing else.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "background_host.h"
#include "context.h"
#include "spans.h"

using namespace stk;

namespace {

struct BgGeometry {
    int n, w, h, cn, C, depth;
    NodeGrid g;
    size_t nodes, plane_floats;      // per frame
};
BgGeometry bg_geometry(const stk_frames* f, int step) {
    BgGeometry q{};
    q.n = f->n; q.w = f->width; q.h = f->height; q.cn = f->channels; q.C = std::min(f->channels, 3); q.depth = f->depth;
    q.g = node_grid(q.w, q.h, step);
    q.nodes = q.g.nodes(); q.plane_floats = q.nodes * q.C;
    return q;
}

stk_status bg_check_frames(stk_ctx* ctx, const stk_frames* frames) {
    stk_status st = check_frames(ctx, frames, false, false);
    if (st) return st;
    if (frames->location != STK_HOST && frames->location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, "background: bad frame location");
    for (int i = 0; i < frames->n; i++)
        if (!frames->data[i]) return fail(ctx, STK_INVALID_PARAMS, "background: null frame pointer");
    return STK_OK;
}

stk_status bg_check_params(stk_ctx* ctx, const stk_frames* frames, const stk_background_params* p, const uint8_t* mask, int mask_location) {
    if (const char* e = bg::validate(p, frames->depth == 32)) return fail(ctx, STK_INVALID_PARAMS, e);
    if (mask && mask_location != STK_HOST && mask_location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, "background: bad location of the mask");
    return STK_OK;
}

// out_depth, the outputs, their row stride and the overlap refusal, as stk_calibrate checks them
stk_status bg_check_out(stk_ctx* ctx, const stk_frames* frames, int out_depth, void* const* out, size_t out_row_stride_bytes,
                        const uint8_t* mask, int mask_location, size_t* ostride) {
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels, depth = frames->depth;
    if (!out) return fail(ctx, STK_INVALID_PARAMS, "background: null outputs");
    for (int i = 0; i < n; i++)
        if (!out[i]) return fail(ctx, STK_INVALID_PARAMS, "background: null output pointer");
    if (out_depth != depth && out_depth != STK_DEPTH_F32)
        return fail(ctx, STK_INVALID_PARAMS, depth == 32 ? "background: f32 frames flatten to STK_DEPTH_F32 only"
                                                         : "background: out_depth must be the frames' depth or STK_DEPTH_F32");
    const size_t oel = (size_t)out_depth / 8, orow = (size_t)w * cn * oel;
    *ostride = out_row_stride_bytes ? out_row_stride_bytes : orow;
    if (*ostride < orow || *ostride % oel) return fail(ctx, STK_INVALID_PARAMS, "background: bad output row stride");
    if ((h + BG_TH - 1) / BG_TH > 65535) return fail(ctx, STK_NOT_IMPLEMENTED, "background: frames above 1048560 rows");
    SpanSet in;
    for (int i = 0; i < n; i++) in.add(frames->data[i], frame_copy_bytes(frames));
    if (mask && mask_location == frames->location) in.add(mask, (size_t)w * h);
    in.seal();
    const size_t ospan = *ostride * (size_t)(h - 1) + orow;
    for (int i = 0; i < n; i++)
        if (in.overlaps(out[i], ospan)) return fail(ctx, STK_INVALID_PARAMS, "background: an output overlaps a frame or the mask (in-place flattening is not supported)");
    return STK_OK;
}

// the cells launches over the frames `dev` (device pointers), behind combine_begin; the records stay at base + L.cells
stk_status bg_cells_run(stk_ctx* ctx, const BgLayout& L, const BgGeometry& q, const stk_frames* frames, const std::vector<const void*>& dev,
                        const stk_background_params* p, const uint8_t* mask, int mask_location) {
    char* base = ctx->local.as<char>();
    HIP_TRY(hipMemcpyAsync(base + L.fptrs, dev.data(), (size_t)q.n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    BgCellsArgs a{};
    if (mask) {
        if (mask_location == STK_HOST) HIP_TRY(hipMemcpyAsync(base + L.mask, mask, (size_t)q.w * q.h, hipMemcpyHostToDevice, ctx->stream));
        a.mask = mask_location == STK_HOST ? (const uint8_t*)(base + L.mask) : mask;
    }
    a.w = q.w; a.h = q.h;
    a.stride = frame_row_bytes(frames);
    a.step = p->step; a.gw = q.g.gw; a.gh = q.g.gh;
    a.clip_iters = p->clip_iters;
    a.ks = (float)((double)p->kappa * 1.4826);
    a.f32_scale = q.depth == 32 ? p->f32_scale : 1.0f;
    if (stk_status st = combine_begin(ctx)) return st;                     // the timed bracket: the launches alone
    for (int f0 = 0; f0 < q.n; f0 += 65535) {
        a.frames = (const void* const*)(base + L.fptrs) + f0;
        a.cells = (stk_bg_cell*)(base + L.cells) + (size_t)f0 * q.nodes * q.C;
        HIP_TRY(launch_background_cells(a, std::min(65535, q.n - f0), q.depth, q.cn, ctx->stream));
    }
    return STK_OK;
}

// the apply launches over the frames `dev`; planes[i]: a HOST plane or null. The planes go up in one copy through `stage`.
// The launches follow combine_begin. Host frames: the outputs land at base + L.out. (rec and stage outlive their copies: the
// caller synchronises.)
stk_status bg_apply_run(stk_ctx* ctx, const BgLayout& L, const BgGeometry& q, const stk_frames* frames, const std::vector<const void*>& dev,
                        const float* const* planes, const float* target, int out_depth, void* const* out, size_t ostride,
                        std::vector<BgFrame>& rec, std::vector<float>& stage) {
    char* base = ctx->local.as<char>();
    const bool host = frames->location == STK_HOST;
    const size_t orow = (size_t)q.w * q.cn * ((size_t)out_depth / 8), ofb = orow * (size_t)q.h;
    rec.assign((size_t)q.n, BgFrame{});
    stage.assign((size_t)q.n * q.plane_floats, 0.0f);
    bool any = false;
    for (int i = 0; i < q.n; i++) {
        rec[i].src = dev[i];
        rec[i].dst = host ? (void*)(base + L.out + ofb * (size_t)i) : out[i];
        if (planes && planes[i]) {
            std::memcpy(stage.data() + (size_t)i * q.plane_floats, planes[i], q.plane_floats * sizeof(float));
            rec[i].plane = (const float*)(base + L.planes + (size_t)i * L.plane);
            any = true;
        }
    }
    if (any) HIP_TRY(hipMemcpyAsync(base + L.planes, stage.data(), stage.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(base + L.records, rec.data(), (size_t)q.n * sizeof(BgFrame), hipMemcpyHostToDevice, ctx->stream));
    BgApplyArgs a{};
    a.w = q.w; a.h = q.h;
    a.in_stride = frame_row_bytes(frames);
    a.out_stride = host ? orow : ostride;
    a.shift = q.g.shift; a.gw = q.g.gw; a.gh = q.g.gh;
    a.inv = 1.0f / (float)q.g.step;
    for (int c = 0; c < 4; c++) a.target[c] = target[c];
    if (stk_status st = combine_begin(ctx)) return st;                     // the timed bracket: the launches alone
    for (int f0 = 0; f0 < q.n; f0 += 65535) {
        a.frames = (const BgFrame*)(base + L.records) + f0;
        a.n = std::min(65535, q.n - f0);
        HIP_TRY(launch_background_apply(a, q.depth, out_depth, q.cn, ctx->stream));
    }
    if (host)
        for (int i = 0; i < q.n; i++)
            HIP_TRY(hipMemcpy2DAsync(out[i], ostride, base + L.out + ofb * (size_t)i, orow, orow, q.h, hipMemcpyDeviceToHost, ctx->stream));
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_background_estimate(int32_t width, int32_t height, int32_t channels, int32_t depth, const stk_background_params* params,
                                   const stk_bg_cell* cells, float* level, float* rms, int32_t* valid, int32_t* flags) {
    return bg::estimate(width, height, channels, depth, params, cells, level, rms, valid, flags);
}

stk_status stk_background_cells(stk_ctx* ctx, const stk_frames* frames, const stk_background_params* params, const uint8_t* mask,
                                int32_t mask_location, stk_bg_cell* cells) {
    stk_status st = bg_check_frames(ctx, frames);
    if (st) return st;
    if ((st = bg_check_params(ctx, frames, params, mask, mask_location))) return st;
    if (!cells) return fail(ctx, STK_INVALID_PARAMS, "background: null cells");
    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    const BgGeometry q = bg_geometry(frames, params->step);
    const size_t records = (size_t)q.n * q.nodes * q.C;
    const BgLayout L = bg_layout((size_t)q.n, mask && mask_location == STK_HOST ? (size_t)q.w * q.h : 0, records * sizeof(stk_bg_cell), 0, 0, 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "background"))) return st;
    std::vector<const void*> dev;
    if ((st = resolve_frames(ctx, frames, dev))) return st;
    if ((st = bg_cells_run(ctx, L, q, frames, dev, params, mask, mask_location))) return st;
    const CombineOutputs o(cells, ctx->local.as<char>() + L.cells, records, sizeof(stk_bg_cell));
    double ms = 0.0;
    if ((st = combine_end(ctx, &ms, &o))) return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

stk_status stk_background_apply(stk_ctx* ctx, const stk_frames* frames, const float* const* planes, int32_t step, const float* target,
                                int32_t out_depth, void* const* out, size_t out_row_stride_bytes) {
    stk_status st = bg_check_frames(ctx, frames);
    if (st) return st;
    if (!bg::step_ok(step)) return fail(ctx, STK_INVALID_PARAMS, "background: step must be 16, 32, 64 or 128");
    if (!target) return fail(ctx, STK_INVALID_PARAMS, "background: null target");
    for (int c = 0; c < 4; c++)
        if (!std::isfinite(target[c])) return fail(ctx, STK_INVALID_PARAMS, "background: target must be finite");
    size_t ostride = 0;
    if ((st = bg_check_out(ctx, frames, out_depth, out, out_row_stride_bytes, nullptr, 0, &ostride))) return st;
    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    const BgGeometry q = bg_geometry(frames, step);
    const bool host = frames->location == STK_HOST;
    const size_t ofb = (size_t)q.w * q.cn * ((size_t)out_depth / 8) * (size_t)q.h;
    const BgLayout L = bg_layout((size_t)q.n, 0, 0, (size_t)q.n, q.plane_floats, host ? ofb * (size_t)q.n : 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "background"))) return st;
    std::vector<const void*> dev;
    if ((st = resolve_frames(ctx, frames, dev))) return st;
    std::vector<BgFrame> rec;
    std::vector<float> stage;
    if ((st = bg_apply_run(ctx, L, q, frames, dev, planes, target, out_depth, out, ostride, rec, stage))) return st;
    double ms = 0.0;
    if ((st = combine_end(ctx, &ms))) return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

stk_status stk_background_flatten(stk_ctx* ctx, const stk_frames* frames, const stk_background_params* params, const uint8_t* mask,
                                  int32_t mask_location, void* const* out, size_t out_row_stride_bytes, float* const* planes_out,
                                  float* const* rms_out, stk_bg_cell* cells_out) {
    stk_status st = bg_check_frames(ctx, frames);
    if (st) return st;
    if ((st = bg_check_params(ctx, frames, params, mask, mask_location))) return st;
    size_t ostride = 0;
    if ((st = bg_check_out(ctx, frames, params->out_depth, out, out_row_stride_bytes, mask, mask_location, &ostride))) return st;
    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    const BgGeometry q = bg_geometry(frames, params->step);
    const bool host = frames->location == STK_HOST;
    const size_t records = (size_t)q.n * q.nodes * q.C;
    const size_t ofb = (size_t)q.w * q.cn * ((size_t)params->out_depth / 8) * (size_t)q.h;
    const BgLayout L = bg_layout((size_t)q.n, mask && mask_location == STK_HOST ? (size_t)q.w * q.h : 0, records * sizeof(stk_bg_cell), (size_t)q.n,
                                 q.plane_floats, host ? ofb * (size_t)q.n : 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "background"))) return st;
    std::vector<const void*> dev;
    if ((st = resolve_frames(ctx, frames, dev))) return st;                // host frames: the one upload of the call
    // 1. the window records
    std::vector<stk_bg_cell> cells(records);
    if ((st = bg_cells_run(ctx, L, q, frames, dev, params, mask, mask_location))) return st;
    const CombineOutputs o(cells.data(), ctx->local.as<char>() + L.cells, records, sizeof(stk_bg_cell));
    double ms = 0.0;
    if ((st = combine_end(ctx, &ms, &o))) return st;
    if (cells_out) std::memcpy(cells_out, cells.data(), records * sizeof(stk_bg_cell));
    // 2. the estimator, per frame
    std::vector<float> level((size_t)q.n * q.plane_floats), rms(rms_out ? level.size() : 0);
    std::vector<const float*> planes((size_t)q.n);
    for (int i = 0; i < q.n; i++) {
        float* P = level.data() + (size_t)i * q.plane_floats;
        float* R = rms_out ? rms.data() + (size_t)i * q.plane_floats : nullptr;
        if (bg::estimate(q.w, q.h, q.cn, q.depth, params, cells.data() + (size_t)i * q.nodes * q.C, P, R, nullptr, nullptr))
            return fail(ctx, STK_INVALID_PARAMS, "background: the estimator refused its arguments");
        planes[i] = P;
        if (planes_out && planes_out[i]) std::memcpy(planes_out[i], P, q.plane_floats * sizeof(float));
        if (rms_out && rms_out[i]) std::memcpy(rms_out[i], R, q.plane_floats * sizeof(float));
    }
    // 3. the subtraction, on the frames still resident
    std::vector<BgFrame> rec;
    std::vector<float> stage;
    if ((st = bg_apply_run(ctx, L, q, frames, dev, planes.data(), params->target, params->out_depth, out, ostride, rec, stage))) return st;
    if ((st = combine_end(ctx, &ms))) return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

}  // extern "C"
