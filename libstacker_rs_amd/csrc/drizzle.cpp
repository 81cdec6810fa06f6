// drizzle.cpp — drizzle integration onto a finer or larger output grid: stk_drizzle_stack, stk_ecc_match_drizzle,
// stk_keypoint_match_drizzle, their forms through local-alignment fields: stk_mesh_drizzle_stack,
// stk_ecc_match_local_aligned_drizzle, stk_keypoint_match_local_aligned_drizzle, and their forms with rejection maps
// (reject.cpp): stk_ecc_match_drizzle_rejected, stk_keypoint_match_drizzle_rejected (an extension beyond the reference;
// definition in include/stacker.h, stk_drizzle_params and the block after it; kernel in kernels_drizzle.hip). The fields
// and their pointer table live in ctx->mesh and are mesh.cpp's to place (through context.h). The frame table is the fold's (ctx->warpframes), its matrices composed here with the
// output grid's map. ctx->local (grow-only, shared with local.cpp; one call at a time) holds, in this order: in the
// whole-stack forms the plain call's mean (unused), then the footprint table, the per-entry records, the map pointer
// table, a host output's staging image and den plane, and host maps' planes. Like weighted.cpp, the whole-stack forms run
// the plain call first and take the warps and the kept set from its stats; the frames are still resident in HBM.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"
#include "drizzle.h"

using namespace stk;

namespace {

// every check that needs neither the matrices nor the records, in the order the errors are reported
stk_status drizzle_validate(stk_ctx* ctx, const stk_frames* frames, bool need_bgr, const stk_drizzle_params* p, const stk_image_f32* out) {
    stk_status st = check_frames(ctx, frames, need_bgr, false);     // warp_interpolation is ignored: the option pair is not asked
    if (st) return st;
    if (ctx->opt_subpixel_bits != 0)
        return fail(ctx, STK_INVALID_PARAMS, "drizzle needs warp_subpixel_bits = 0: it is defined on exact coordinates only");
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null drizzle parameters");
    if (!std::isfinite(p->scale) || p->scale < 1.0f || p->scale > 4.0f) return fail(ctx, STK_INVALID_PARAMS, "drizzle: scale must be 1 .. 4");
    if (!std::isfinite(p->pixfrac) || !(p->pixfrac > 0.0f) || p->pixfrac > 1.0f)
        return fail(ctx, STK_INVALID_PARAMS, "drizzle: pixfrac must be in (0, 1]");
    if (!std::isfinite(p->origin_x) || !std::isfinite(p->origin_y)) return fail(ctx, STK_INVALID_PARAMS, "drizzle: the origin must be finite");
    if (!std::isfinite(p->fill)) return fail(ctx, STK_INVALID_PARAMS, "drizzle: fill must be finite");
    if (p->reserved != 0) return fail(ctx, STK_INVALID_PARAMS, "drizzle parameters: reserved must be 0");
    if (!out || !out->data) return fail(ctx, STK_INVALID_PARAMS, "null output image");
    if (out->width < 1 || out->height < 1 || out->width > 32768 || out->height > 32768)
        return fail(ctx, STK_INVALID_PARAMS, "drizzle: the output must be 1 .. 32768 pixels wide and high");
    if (out->channels != frames->channels) return fail(ctx, STK_INVALID_PARAMS, "drizzle: the output must have the frames' channels");
    if (out->row_stride_bytes && out->row_stride_bytes != (size_t)out->width * out->channels * sizeof(float))
        return fail(ctx, STK_INVALID_PARAMS, "output must be tightly packed");
    return STK_OK;
}

// Table entry under forward matrix M (include/stacker.h, "Coordinates"): A = inv(M) . G in double, each operation rounded on
// its own, cast to f32; for an affine entry the footprint half-extents from the f32 values of A.
void drizzle_entry(WarpFrame& wf, float* foot, const void* src, const double* M, int is_affine, const stk_drizzle_params* p) {
    double inv[9], A[9];
    if (is_affine) warp_invert_affine(M, inv); else warp_invert3x3(M, inv);
    const double g = 1.0 / (double)p->scale;
    const double tx = (0.5 * g - 0.5) + (double)p->origin_x, ty = (0.5 * g - 0.5) + (double)p->origin_y;
    for (int r = 0; r < 3; r++) {
        A[3 * r] = inv[3 * r] * g;
        A[3 * r + 1] = inv[3 * r + 1] * g;
        A[3 * r + 2] = (inv[3 * r] * tx + inv[3 * r + 1] * ty) + inv[3 * r + 2];
    }
    wf.src = src;
    wf.flags = 0;
    for (int k = 0; k < 9; k++) { wf.Md[k] = A[k]; wf.M[k] = (float)A[k]; }
    const float hmax = 1.5f - 0.5f * p->pixfrac;
    foot[0] = std::fmin((float)(0.5 * (std::fabs((double)wf.M[0]) + std::fabs((double)wf.M[1]))), hmax);
    foot[1] = std::fmin((float)(0.5 * (std::fabs((double)wf.M[3]) + std::fabs((double)wf.M[4]))), hmax);
}

// The drizzle launch over the table's entries, `dev[table.frame[k]]` under table.M[k], with the records `coef` (per entry) and the
// maps (by frame index, in frames->location or with maps_device in device memory whatever the frames' location, or null).
// ctx->local is reserved for L. Writes `out` and `den_out` (out's location), synchronises, adds the launch's device time
// to *ms.
stk_status drizzle_run(stk_ctx* ctx, const DrizzleLayout& L, const stk_frames* frames, const std::vector<const void*>& dev,
                       const EntryTable& table, int is_affine, double alpha,
                       const stk_drizzle_params* p, const std::vector<stk_frame_weight>& coef, const float* const* maps,
                       stk_image_f32* out, float* den_out, double* ms, const MeshFoldArgs* mesh = nullptr, bool maps_device = false) {
    const int ne = table.size(), sw = frames->width, sh = frames->height, cn = frames->channels;
    const int ow = out->width, oh = out->height;
    const size_t rb = frame_row_bytes(frames);
    char* base = ctx->local.as<char>();
    const bool host_maps = frames->location != STK_DEVICE && !maps_device;
    const CombineOutputs o(out, (float*)(base + L.image), (size_t)ow * oh * cn, {den_out, base + L.den, (size_t)ow * oh});
    std::vector<WarpFrame> wf(ne);
    std::vector<float> foot((size_t)ne * 2);
    std::vector<const float*> mptr(ne, nullptr);
    for (int k = 0; k < ne; k++) drizzle_entry(wf[k], &foot[2 * (size_t)k], dev[table.frame[k]], table.M[k], is_affine, p);
    stk_status st = warp_table_upload(ctx, wf, rb, ow, oh, is_affine);
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(base + L.foot, foot.data(), foot.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if ((st = records_upload(ctx, base + L.coef, coef))) return st;
    if (maps) {
        size_t slot = 0;
        for (int k = 0; k < ne; k++) {
            const float* m = maps[table.frame[k]];
            if (m && host_maps) {
                float* d = (float*)(base + L.planes + slot++ * L.plane);
                HIP_TRY(hipMemcpyAsync(d, m, (size_t)sw * sh * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
                m = d;
            }
            mptr[k] = m;
        }
        HIP_TRY(hipMemcpyAsync(base + L.mptrs, mptr.data(), (size_t)ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    }
    DrizzleArgs a{};
    a.frames = ctx->warpframes.as<WarpFrame>();
    a.n_frames = ne;
    a.sw = sw; a.sh = sh; a.cn = cn;
    a.src_stride = rb / (frames->depth / 8);
    a.alpha = (float)alpha;
    a.is_affine = is_affine;
    a.foot = (const float*)(base + L.foot);
    a.coef = (const stk_frame_weight*)(base + L.coef);
    a.maps = maps ? (const float* const*)(base + L.mptrs) : nullptr;
    a.hp = 0.5f * p->pixfrac; a.hmax = 1.5f - 0.5f * p->pixfrac; a.fill = p->fill;
    a.out = o.image();
    a.den = o.side<float>(0);
    a.ow = ow; a.oh = oh;
    if (mesh) {
        // the grid's map onto frame 0, as drizzle_entry composes it
        const double g = 1.0 / (double)p->scale;
        a.fields = mesh->fields;
        a.mesh_shift = 0;
        while ((1 << a.mesh_shift) < mesh->step) a.mesh_shift++;
        a.mesh_gw = mesh->gw; a.mesh_gh = mesh->gh;
        a.mesh_inv = 1.0f / (float)mesh->step;
        a.mesh_g = (float)g;
        a.mesh_tx = (float)((0.5 * g - 0.5) + (double)p->origin_x);
        a.mesh_ty = (float)((0.5 * g - 0.5) + (double)p->origin_y);
        a.mesh_s = p->scale;
    }
    if ((st = combine_begin(ctx))) return st;
    HIP_TRY(launch_drizzle(a, frames->depth, ctx->stream));
    return combine_end(ctx, ms, &o);                     // (synchronises: the host tables leave scope)
}

// the tail of the whole-stack forms: the frames the plain call kept (combine.h: entries_from_stats), all weights 1, no
// maps, alpha = 1 / 255; the timing stays the plain call's but for finalize_ms. With mesh parameters: the field pass over
// the same entries under the fold's matrices first (ctx->mesh is reserved), the drizzle through its fields, and
// finalize_ms the sum of the two. (Not combine.h's scaffold: the drizzle's own table has the output's geometry, and
// without mesh parameters the fold's table is never uploaded.)
stk_status drizzle_finish(stk_ctx* ctx, const DrizzleLayout& L, const stk_frames* frames, const stk_frame_stats* stats, bool keypoint,
                          int is_affine, const stk_drizzle_params* p, stk_image_f32* out, float* den_out, const stk_mesh_params* mp = nullptr) {
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    EntryTable table;
    entries_from_stats(frames->n, stats, keypoint, table);
    const std::vector<stk_frame_weight> coef(table.frame.size(), unit_record());
    const stk_timing keep = ctx->timing;
    double ms = 0.0, fms = 0.0;
    stk_status st = STK_OK;
    MeshFoldArgs mf{};
    if (mp && !(st = entry_table_upload(ctx, frames, dev, table, is_affine)))
        st = mesh_match_fields(ctx, frames, table.size(), is_affine, mp, &mf, &fms);
    if (!st) st = drizzle_run(ctx, L, frames, dev, table, is_affine, 1.0 / 255.0, p, coef, nullptr, out, den_out, &ms, mp ? &mf : nullptr);
    ctx->timing = keep; ctx->timing.finalize_ms = st ? 0.0 : fms + ms;
    return st;
}

// stk_drizzle_stack, and with `fields` (n planes by frame index, in frames->location) stk_mesh_drizzle_stack
stk_status drizzle_stack_impl(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                              double alpha, const stk_drizzle_params* p, const stk_frame_weight* per_frame, const float* const* maps,
                              bool mesh, const float* const* fields, int32_t step, stk_image_f32* out, float* den_out) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = drizzle_validate(ctx, frames, false, p, out);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (mesh) {
        if (!fields) return fail(ctx, STK_INVALID_PARAMS, "null fields");
        if (!grid_step_ok(step)) return fail(ctx, STK_INVALID_PARAMS, "mesh: step must be 8, 16, 32, 64, 128 or 256");
    }
    const int n = frames->n, cn = frames->channels;
    EntryTable table;
    entries_from_include(n, M, include, table);
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "drizzle: no frame included");
    std::vector<stk_frame_weight> coef;
    gather_records(table, per_frame, coef);
    size_t n_planes = 0;
    for (int i : table.frame)
        if (maps && maps[i] && frames->location != STK_DEVICE) n_planes++;
    if ((st = weighted_check_coefs(ctx, coef, cn))) return st;
    (void)hipSetDevice(ctx->device);
    timing_begin(ctx);
    const DrizzleLayout L = drizzle_layout(0, (int)coef.size(), frames->width, frames->height, out->width, out->height, cn,
                                           out->location != STK_DEVICE, n_planes);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "drizzle"))) return st;
    std::vector<const void*> dev;
    if ((st = resolve_frames(ctx, frames, dev))) return st;
    MeshFoldArgs mf{};
    if (mesh && (st = mesh_fold_table(ctx, frames, table, fields, step, &mf))) return st;
    double ms = 0.0;
    if ((st = drizzle_run(ctx, L, frames, dev, table, is_affine != 0, alpha, p, coef, maps, out, den_out, &ms, mesh ? &mf : nullptr)))
        return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

// stk_ecc_match_drizzle, and with mesh parameters stk_ecc_match_local_aligned_drizzle
stk_status ecc_match_drizzle_impl(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                  const stk_mesh_params* mesh, const stk_drizzle_params* p, stk_image_f32* out, float* den_out,
                                  stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = drizzle_validate(ctx, frames, true, p, out);
    if (st) return st;
    if (mesh && (st = mesh_match_fields_check(ctx, frames, mesh))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const size_t pre = (size_t)w * h * cn * sizeof(float);
    const DrizzleLayout L = drizzle_layout(pre, n, w, h, out->width, out->height, cn, out->location != STK_DEVICE, 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "drizzle"))) return st;
    if (mesh && (st = mesh_match_fields_reserve(ctx, frames, mesh))) return st;
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    // the plain call, on this context's own device, its mean into the head of the workspace (unused)
    stk_image_f32 mimg{ctx->local.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = ecc_match_single(ctx, frames, params, scale_down_width, &mimg, stats))) return st;
    return drizzle_finish(ctx, L, frames, stats, false, params->motion_type != STK_MOTION_HOMOGRAPHY, p, out, den_out, mesh);
}

// stk_keypoint_match_drizzle, and with mesh parameters stk_keypoint_match_local_aligned_drizzle
stk_status keypoint_match_drizzle_impl(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                                       const stk_mesh_params* mesh, const stk_drizzle_params* p, stk_image_f32* out, int32_t* dropped,
                                       float* den_out, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = drizzle_validate(ctx, frames, true, p, out);
    if (st) return st;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null parameters");
    if (mesh && (st = mesh_match_fields_check(ctx, frames, mesh))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const size_t pre = (size_t)w * h * cn * sizeof(float);
    const DrizzleLayout L = drizzle_layout(pre, n, w, h, out->width, out->height, cn, out->location != STK_DEVICE, 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "drizzle"))) return st;
    if (mesh && (st = mesh_match_fields_reserve(ctx, frames, mesh))) return st;
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    stk_image_f32 mimg{ctx->local.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = keypoint_match_single(ctx, frames, params, scale_down_width, &mimg, dropped, stats))) return st;
    return drizzle_finish(ctx, L, frames, stats, true, 0, p, out, den_out, mesh);
}

// the checks of the rejected forms beyond drizzle's own, in the order the errors are reported
stk_status drizzle_rejected_validate(stk_ctx* ctx, const stk_frames* frames, const stk_weight_params* weight, const stk_reject_params* reject) {
    stk_status st = weighted_validate(ctx, weight);
    if (st) return st;
    if (weight->coverage != 1) return fail(ctx, STK_INVALID_PARAMS, "rejected drizzle: weight coverage must be 1 (the clean image is the coverage-aware median)");
    if ((st = reject_validate(ctx, reject))) return st;
    return quantile_check_count(ctx, frames->n);
}

struct RejectedLayouts { DrizzleLayout D; RejectLayout R; };

// device memory of the rejected forms, before the plain call runs: the maps, the clean image and its counts (ctx->reject),
// the median's image and band (ctx->quantile), the drizzle's tables and staging behind the plain call's mean (ctx->local)
stk_status drizzle_rejected_reserve(stk_ctx* ctx, const stk_frames* frames, const stk_image_f32* out, RejectedLayouts* Ls) {
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    Ls->D = drizzle_layout((size_t)w * h * cn * sizeof(float), n, w, h, out->width, out->height, cn, out->location != STK_DEVICE, 0);
    Ls->R = reject_layout(n, w, h, cn, true, true, (size_t)n);
    stk_status st = workspace_reserve(ctx, ctx->reject, Ls->R.total, "reject maps");
    if (st) return st;
    if ((st = workspace_reserve(ctx, ctx->local, Ls->D.total, "drizzle"))) return st;
    return quantile_reserve(ctx, n, w, h, cn, false, nullptr);
}

// the tail of the rejected forms, after the plain call: records, median, reject maps, drizzle (include/stacker.h, the steps
// of stk_ecc_match_drizzle_rejected); finalize_ms = the sum of their device times, the rest of the timing the plain call's
stk_status drizzle_rejected_finish(stk_ctx* ctx, const RejectedLayouts& Ls, const stk_frames* frames, const stk_frame_stats* stats,
                                   bool keypoint, const FoldSpec& spec, const stk_drizzle_params* p, const stk_weight_params* weight,
                                   const float* weights, const stk_reject_params* reject, stk_image_f32* out, float* den_out,
                                   float* const* maps, int64_t* rejected, stk_frame_weight* applied) {
    const int n = frames->n, w = frames->width, h = frames->height, is_affine = spec.is_affine;
    const stk_timing keep = ctx->timing;
    EntryTable table;
    const std::vector<int>& entry_frame = table.frame;
    std::vector<stk_frame_weight> coef;
    double ms = 0.0, dms = 0.0;
    char* base = ctx->reject.as<char>();
    float* clean = (float*)(base + Ls.R.clean);
    int32_t* counts = (int32_t*)(base + Ls.R.counts);
    stk_status st = robust_match_records(ctx, frames, stats, keypoint, spec, weight, weights, table, coef, applied, &ms);
    if (!st) st = robust_match_median(ctx, frames, coef, is_affine, clean, counts, &ms);
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    const size_t ne = entry_frame.size();
    std::vector<const float*> in(ne, nullptr), by_frame(n, nullptr);
    std::vector<float*> planes(ne);
    std::vector<int64_t> rej(ne);
    for (size_t k = 0; k < ne; k++) {
        planes[k] = (float*)(base + Ls.R.planes + k * Ls.R.plane);
        by_frame[entry_frame[k]] = planes[k];
    }
    if (!st) st = reject_run(ctx, Ls.R, frames, dev, table, is_affine, 1.0 / 255.0, coef, clean, counts, reject, in, planes, rej.data(), nullptr,
                             &ms);
    if (!st) st = drizzle_run(ctx, Ls.D, frames, dev, table, is_affine, 1.0 / 255.0, p, coef, by_frame.data(), out, den_out, &dms, nullptr,
                              true);
    if (!st && maps) {
        const hipMemcpyKind kind = frames->location != STK_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        for (size_t k = 0; k < ne && !st; k++) {
            float* dst = maps[entry_frame[k]];
            if (dst && hipMemcpyAsync(dst, planes[k], (size_t)w * h * sizeof(float), kind, ctx->stream) != hipSuccess)
                st = fail(ctx, STK_HIP_ERROR, "rejected drizzle: copying a map out failed");
        }
        if (!st && hipStreamSynchronize(ctx->stream) != hipSuccess) st = fail(ctx, STK_HIP_ERROR, "rejected drizzle: copying the maps out failed");
    }
    if (!st && rejected) {
        for (int i = 0; i < n; i++) rejected[i] = 0;
        for (size_t k = 0; k < ne; k++) rejected[entry_frame[k]] = rej[k];
    }
    ctx->timing = keep; ctx->timing.finalize_ms = st ? 0.0 : ms + dms;
    return st;
}

}  // namespace

extern "C" {

stk_status stk_ecc_match_drizzle_rejected(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                          const stk_drizzle_params* p, const stk_weight_params* weight, const float* weights,
                                          const stk_reject_params* reject, stk_image_f32* out, float* den_out, float* const* maps,
                                          int64_t* rejected, stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = drizzle_validate(ctx, frames, true, p, out);
    if (st) return st;
    if ((st = drizzle_rejected_validate(ctx, frames, weight, reject))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    RejectedLayouts Ls;
    if ((st = drizzle_rejected_reserve(ctx, frames, out, &Ls))) return st;
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    // the plain call, on this context's own device, its mean into the head of the workspace (unused)
    stk_image_f32 mimg{ctx->local.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = ecc_match_single(ctx, frames, params, scale_down_width, &mimg, stats))) return st;
    return drizzle_rejected_finish(ctx, Ls, frames, stats, false, fold_spec_ecc(frames, params), p, weight, weights, reject, out, den_out,
                                   maps, rejected, applied);
}

stk_status stk_keypoint_match_drizzle_rejected(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                               float scale_down_width, const stk_drizzle_params* p, const stk_weight_params* weight,
                                               const float* weights, const stk_reject_params* reject, stk_image_f32* out,
                                               int32_t* dropped, float* den_out, float* const* maps, int64_t* rejected,
                                               stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = drizzle_validate(ctx, frames, true, p, out);
    if (st) return st;
    if ((st = drizzle_rejected_validate(ctx, frames, weight, reject))) return st;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null parameters");
    if ((st = weighted_check_border(ctx, params->border_mode, params->border_value, 1))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    RejectedLayouts Ls;
    if ((st = drizzle_rejected_reserve(ctx, frames, out, &Ls))) return st;
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    stk_image_f32 mimg{ctx->local.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = keypoint_match_single(ctx, frames, params, scale_down_width, &mimg, dropped, stats))) return st;
    return drizzle_rejected_finish(ctx, Ls, frames, stats, true, fold_spec_keypoint(frames, params), p, weight, weights, reject, out,
                                   den_out, maps, rejected, applied);
}

stk_status stk_drizzle_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                             double alpha, const stk_drizzle_params* p, const stk_frame_weight* per_frame, const float* const* maps,
                             stk_image_f32* out, float* den_out) {
    return drizzle_stack_impl(ctx, frames, M, include, is_affine, alpha, p, per_frame, maps, false, nullptr, 0, out, den_out);
}

stk_status stk_mesh_drizzle_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                  double alpha, const stk_drizzle_params* p, const stk_frame_weight* per_frame, const float* const* maps,
                                  const float* const* fields, int32_t step, stk_image_f32* out, float* den_out) {
    return drizzle_stack_impl(ctx, frames, M, include, is_affine, alpha, p, per_frame, maps, true, fields, step, out, den_out);
}

stk_status stk_ecc_match_drizzle(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                 const stk_drizzle_params* p, stk_image_f32* out, float* den_out, stk_frame_stats* stats) {
    return ecc_match_drizzle_impl(ctx, frames, params, scale_down_width, nullptr, p, out, den_out, stats);
}

stk_status stk_keypoint_match_drizzle(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                                      const stk_drizzle_params* p, stk_image_f32* out, int32_t* dropped, float* den_out,
                                      stk_frame_stats* stats) {
    return keypoint_match_drizzle_impl(ctx, frames, params, scale_down_width, nullptr, p, out, dropped, den_out, stats);
}

stk_status stk_ecc_match_local_aligned_drizzle(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                               float scale_down_width, const stk_mesh_params* mesh, const stk_drizzle_params* p,
                                               stk_image_f32* out, float* den_out, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!mesh) return fail(ctx, STK_INVALID_PARAMS, "null mesh parameters");
    return ecc_match_drizzle_impl(ctx, frames, params, scale_down_width, mesh, p, out, den_out, stats);
}

stk_status stk_keypoint_match_local_aligned_drizzle(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                                    float scale_down_width, const stk_mesh_params* mesh, const stk_drizzle_params* p,
                                                    stk_image_f32* out, int32_t* dropped, float* den_out, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!mesh) return fail(ctx, STK_INVALID_PARAMS, "null mesh parameters");
    return keypoint_match_drizzle_impl(ctx, frames, params, scale_down_width, mesh, p, out, dropped, den_out, stats);
}

}  // extern "C"
