// local.cpp — per-pixel weight maps and local-sharpness (lucky-region) stacking: stk_local_sharpness,
// stk_local_weighted_stack, stk_ecc_match_local_weighted, stk_keypoint_match_local_weighted (an extension beyond the
// reference; definition in include/stacker.h, stk_local_params; kernels in kernels_local.hip and warp_body.h).
// ctx->local (grow-only like the other workspaces) holds the pointer tables of the map pass and of the fold, the per-entry
// gain / offset / weight table, a w x h x cn f32 image (the plain call's mean in the whole-stack forms, then a host
// output's staging copy), the w x h den plane and the map planes of the fold's entries. The checks, the frame table, the
// moments pass and the estimator are the weighted combine's (weighted.cpp, through context.h). Like weighted.cpp, the
// whole-stack forms run the plain call first and take the warps and the kept set from its stats; the frames are still
// resident in HBM, full size, and the maps of the entries are computed from them.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

// (the layout, the checks, the map pass and the fold are shared with mesh.cpp: context.h)
// cn == 0: the map pass alone (no per-entry table, image or den plane)
LocalLayout local_layout(size_t n_ptrs, int n_entries, int w, int h, int cn, size_t n_planes) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    LocalLayout L{};
    L.fptrs = 0;
    L.mptrs = up(std::max<size_t>(n_ptrs, 1) * sizeof(void*));
    L.coef = L.mptrs + up(std::max<size_t>(n_ptrs, 1) * sizeof(void*));
    L.image = L.coef + (cn ? up((size_t)std::max(n_entries, 1) * sizeof(stk_frame_weight)) : 0);
    L.den = L.image + up((size_t)w * h * cn * sizeof(float));
    L.planes = L.den + (cn ? up((size_t)w * h * sizeof(float)) : 0);
    L.plane = up((size_t)w * h * sizeof(float));
    L.total = L.planes + n_planes * L.plane;
    return L;
}

stk_status local_reserve(stk_ctx* ctx, const LocalLayout& L, size_t n_planes) {
    if (ctx->local.reserve(L.total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, STK_HIP_ERROR, "local: device allocation of " + std::to_string(L.total) + " bytes failed (" +
                                            std::to_string(n_planes) + " map planes of " + std::to_string(L.plane) + " bytes)");
    }
    return STK_OK;
}

stk_status local_validate(stk_ctx* ctx, const stk_local_params* p) {
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null local parameters");
    if (p->radius < 1 || p->radius > 15) return fail(ctx, STK_INVALID_PARAMS, "local: radius must be 1 .. 15");
    if (p->threshold < 0 || p->threshold > 1020) return fail(ctx, STK_INVALID_PARAMS, "local: threshold must be 0 .. 1020");
    if (p->power < 1 || p->power > 4) return fail(ctx, STK_INVALID_PARAMS, "local: power must be 1 .. 4");
    if (!std::isfinite(p->floor) || p->floor < 0.0f) return fail(ctx, STK_INVALID_PARAMS, "local: floor must be finite and >= 0");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(ctx, STK_INVALID_PARAMS, "local parameters: reserved must be 0");
    return STK_OK;
}

namespace {

stk_status local_check_depth(stk_ctx* ctx, const stk_frames* f) {
    if (f->depth != 8)
        return fail(ctx, STK_NOT_IMPLEMENTED,
                    "local sharpness takes 8-bit frames: the quality map is defined on the 8-bit integer grey, its sums are exact "
                    "integers below 2^24");
    return STK_OK;
}

}  // namespace

// a weight taken outside a frame means nothing: the fold runs under BORDER_CONSTANT with border value 0
stk_status local_check_border(stk_ctx* ctx, int border_mode, const double* border_value) {
    if (border_mode < 0 || border_mode > 4)
        return fail(ctx, border_mode == STK_BORDER_TRANSPARENT ? STK_NOT_IMPLEMENTED : STK_INVALID_PARAMS,
                    "border mode not supported (BORDER_TRANSPARENT leaves the reference's output uninitialised)");
    bool zero = border_mode == STK_BORDER_CONSTANT;
    for (int k = 0; k < 4 && border_value; k++) zero = zero && border_value[k] == 0.0;
    if (!zero) return fail(ctx, STK_INVALID_PARAMS, "local: the fold needs border_mode BORDER_CONSTANT with border_value 0");
    return STK_OK;
}

// The map pass over frames[k] -> planes[k] (device pointers) through the pointer tables at L.fptrs / L.mptrs of ctx->local:
// the tables' upload (asynchronous: the two vectors must outlive the stream's copies), then launches over table entries
// [first, first + n).
stk_status local_maps_enqueue(stk_ctx* ctx, const LocalLayout& L, const std::vector<const void*>& frames, const std::vector<float*>& planes) {
    char* base = ctx->local.as<char>();
    const size_t n = frames.size();
    HIP_TRY(hipMemcpyAsync(base + L.fptrs, frames.data(), n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(base + L.mptrs, planes.data(), n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    return STK_OK;
}
stk_status local_maps_launch(stk_ctx* ctx, const LocalLayout& L, size_t first, size_t n, int cn, int w, int h, size_t rb,
                             const stk_local_params* p) {
    char* base = ctx->local.as<char>();
    for (size_t l0 = 0; l0 < n; l0 += 65535) {
        const int nl = (int)std::min<size_t>(65535, n - l0);
        HIP_TRY(launch_local_maps((const void* const*)(base + L.fptrs) + first + l0, (float* const*)(base + L.mptrs) + first + l0, nl, cn,
                                  w, h, rb, p->radius, p->threshold, ctx->stream));
    }
    return STK_OK;
}

// The local-weighted fold over the n_entries entries of ctx->warpframes with the per-entry records `coef` and the plane
// table at L.mptrs (uploaded by the caller). Writes `out` and `den_out` (out's location); adds its device time to *ms.
// mesh: the generic kernel's mesh variant with that field table (mesh.cpp).
stk_status local_fold(stk_ctx* ctx, const LocalLayout& L, const std::vector<stk_frame_weight>& coef, int depth, int w, int h, int cn,
                      size_t src_row_bytes, double alpha, int is_affine, float floor, int power, stk_image_f32* out, float* den_out,
                      double* ms, const MeshFoldArgs* mesh) {
    char* base = ctx->local.as<char>();
    const bool host = out->location != STK_DEVICE;
    const WarpArgs a = weighted_warp_args(ctx, (int)coef.size(), depth, w, h, cn, src_row_bytes, alpha, STK_BORDER_CONSTANT, nullptr, is_affine);
    ClipArgs ca{};
    ca.coef = (const stk_frame_weight*)(base + L.coef);
    ca.coverage = 1;
    ca.out = host ? (float*)(base + L.image) : out->data;
    ca.out_stride = (size_t)w * cn;
    ca.den = den_out ? (host ? (float*)(base + L.den) : den_out) : nullptr;
    ca.den_stride = (size_t)w;
    ca.maps = (const float* const*)(base + L.mptrs);
    ca.map_stride = (size_t)w;
    ca.floor = floor;
    ca.power = power;
    HIP_TRY(hipMemcpyAsync(base + L.coef, coef.data(), coef.size() * sizeof(stk_frame_weight), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    if (mesh) {
        mesh_fold_clip_args(*mesh, ca);
        HIP_TRY(launch_mesh_fold(a, ca, depth, true, ctx->stream));
    } else HIP_TRY(launch_local_fold(a, ca, depth, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    if (host) {
        HIP_TRY(hipMemcpyAsync(out->data, ca.out, (size_t)w * h * cn * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (den_out) HIP_TRY(hipMemcpyAsync(den_out, ca.den, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ms) *ms += ev_ms(ctx->ev[4], ctx->ev[5]);
    return STK_OK;
}

namespace {

// the checks the two whole-stack forms share, in the order the errors are reported
stk_status local_match_check(stk_ctx* ctx, const stk_frames* frames, const stk_weight_params* weight, const stk_local_params* local,
                             const stk_image_f32* out) {
    stk_status st = weighted_validate(ctx, weight);
    if (st) return st;
    if (weight->coverage != 1) return fail(ctx, STK_INVALID_PARAMS, "local: stk_weight_params.coverage must be 1");
    if ((st = local_validate(ctx, local))) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = local_check_depth(ctx, frames))) return st;
    return weighted_check_out(ctx, out, frames);
}

// the tail of the whole-stack forms: `entry_frame[k]` is the frame index of table entry k (entry 0 = frame 0), `dev` the
// resident full-size frames by frame index; the frame table is uploaded. Map pass, moments pass, estimator, fold.
stk_status local_finish(stk_ctx* ctx, const LocalLayout& L, const stk_frames* frames, const std::vector<int>& entry_frame,
                        const std::vector<const void*>& dev, size_t rb, int is_affine, const stk_weight_params* p, const float* weights,
                        const stk_local_params* lp, stk_image_f32* out, float* den_out, stk_frame_weight* applied) {
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const int ne = (int)entry_frame.size();
    const double alpha = 1.0 / 255.0;
    char* base = ctx->local.as<char>();
    double ms = 0.0;
    std::vector<const void*> fptr(ne);
    std::vector<float*> mptr(ne);
    for (int k = 0; k < ne; k++) { fptr[k] = dev[entry_frame[k]]; mptr[k] = (float*)(base + L.planes + (size_t)k * L.plane); }
    stk_status st = local_maps_enqueue(ctx, L, fptr, mptr);
    if (st) return st;
    HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    if ((st = local_maps_launch(ctx, L, 0, (size_t)ne, cn, w, h, rb, lp))) return st;
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ms += ev_ms(ctx->ev[4], ctx->ev[5]);
    std::vector<stk_frame_weight> coef(ne);
    std::vector<double> mom((size_t)std::max(ne - 1, 0) * cn * 6);
    if (p->normalize != 0 && ne > 1) {
        const int step = p->stat_step ? p->stat_step : 4;
        if ((st = weighted_moments(ctx, ne, 8, w, h, cn, rb, alpha, STK_BORDER_CONSTANT, nullptr, is_affine, step, mom.data(), &ms))) return st;
    }
    for (int k = 0; k < ne; k++) {
        if (k == 0) weighted_estimate(nullptr, cn, 0, &coef[k]);
        else weighted_estimate(mom.data() + (size_t)(k - 1) * cn * 6, cn, p->normalize, &coef[k]);
        coef[k].weight = weights ? weights[entry_frame[k]] : 1.0f;
    }
    if ((st = weighted_check_coefs(ctx, coef, cn))) return st;
    if ((st = local_fold(ctx, L, coef, 8, w, h, cn, rb, alpha, is_affine, lp->floor, lp->power, out, den_out, &ms))) return st;
    ctx->timing.finalize_ms = ms;
    if (applied) {
        for (int i = 0; i < n; i++) { weighted_estimate(nullptr, cn, 0, &applied[i]); applied[i].weight = 0.0f; }
        for (int k = 0; k < ne; k++) applied[entry_frame[k]] = coef[k];
    }
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_local_sharpness(stk_ctx* ctx, const stk_frames* frames, const stk_local_params* p, float* const* maps) {
    stk_status st = check_frames(ctx, frames, false, false);
    if (st) return st;
    if ((st = local_validate(ctx, p))) return st;
    if (!maps) return fail(ctx, STK_INVALID_PARAMS, "null maps");
    if ((st = local_check_depth(ctx, frames))) return st;
    (void)hipSetDevice(ctx->device);
    timing_begin(ctx);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const size_t rb = frame_row_bytes(frames), fb = rb * h;
    const bool host = frames->location == STK_HOST;
    for (int i = 0; i < n; i++) if (!maps[i]) return fail(ctx, STK_INVALID_PARAMS, "null map plane");
    // host frames go through the frame workspace in batches that fit it (at least "upload_batch" frames), as in
    // stk_stack_sharpness; their planes through ctx->local
    int batch = n;
    if (host) {
        const size_t budget = std::max<size_t>(ctx->frames.cap, (size_t)ctx->opt_upload_batch * fb);
        batch = (int)std::min<size_t>((size_t)n, std::max<size_t>(1, budget / fb));
        HIP_TRY(ctx->frames.reserve(fb * (size_t)batch));
    }
    const size_t n_ptrs = host ? (size_t)batch : (size_t)n;
    const LocalLayout Lp = local_layout(n_ptrs, 0, w, h, 0, host ? (size_t)batch : 0);
    if ((st = local_reserve(ctx, Lp, host ? (size_t)batch : 0))) return st;
    char* base = ctx->local.as<char>();
    std::vector<const void*> fptr(n_ptrs);                         // (outlive the copies: the call synchronises below)
    std::vector<float*> mptr(n_ptrs);
    for (size_t i = 0; i < n_ptrs; i++) {
        fptr[i] = host ? (const void*)(ctx->frames.as<uint8_t>() + fb * i) : frames->data[i];
        mptr[i] = host ? (float*)(base + Lp.planes + i * Lp.plane) : maps[i];
    }
    HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    if ((st = local_maps_enqueue(ctx, Lp, fptr, mptr))) return st;
    for (int b0 = 0; b0 < n; b0 += batch) {
        const int nb = std::min(batch, n - b0);
        if (host)      // stream order keeps the previous batch's kernels and copies ahead of the copies that overwrite its frames
            for (int i = 0; i < nb; i++)
                HIP_TRY(hipMemcpyAsync(ctx->frames.as<uint8_t>() + fb * (size_t)i, frames->data[b0 + i], frame_copy_bytes(frames), hipMemcpyHostToDevice, ctx->stream));
        if ((st = local_maps_launch(ctx, Lp, host ? 0 : (size_t)b0, (size_t)nb, cn, w, h, rb, p))) return st;
        if (host)
            for (int i = 0; i < nb; i++)
                HIP_TRY(hipMemcpyAsync(maps[b0 + i], mptr[i], (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.prep_ms = ev_ms(ctx->ev[0], ctx->ev[1]);
    return STK_OK;
}

stk_status stk_local_weighted_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                    int32_t border_mode, const double* border_value, double alpha, const stk_frame_weight* per_frame,
                                    const float* const* maps, float floor, int32_t power, stk_image_f32* out, float* den_out) {
    return local_weighted_stack_impl(ctx, frames, M, include, is_affine, border_mode, border_value, alpha, per_frame, maps, floor, power,
                                     nullptr, 0, out, den_out);
}

}  // extern "C"

stk_status local_weighted_stack_impl(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                     int32_t border_mode, const double* border_value, double alpha, const stk_frame_weight* per_frame,
                                     const float* const* maps, float floor, int32_t power, const float* const* fields, int32_t step,
                                     stk_image_f32* out, float* den_out) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (!maps) return fail(ctx, STK_INVALID_PARAMS, "null maps");
    if (fields && (st = mesh_check_fold(ctx, step))) return st;
    if ((st = local_check_border(ctx, border_mode, border_value))) return st;
    if (power < 1 || power > 4) return fail(ctx, STK_INVALID_PARAMS, "local: power must be 1 .. 4");
    if (!std::isfinite(floor) || floor < 0.0f) return fail(ctx, STK_INVALID_PARAMS, "local: floor must be finite and >= 0");
    if ((st = weighted_check_out(ctx, out, frames))) return st;
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    std::vector<stk_frame_weight> coef;
    for (int i = 0; i < n; i++) {
        if (include && !include[i]) continue;
        if (!maps[i]) return fail(ctx, STK_INVALID_PARAMS, "null map plane of an included frame");
        if (fields && i > 0 && !fields[i]) return fail(ctx, STK_INVALID_PARAMS, "null field plane of an included frame");
        stk_frame_weight e;
        if (per_frame) e = per_frame[i];
        else { weighted_estimate(nullptr, cn, 0, &e); e.weight = 1.0f; }
        coef.push_back(e);
    }
    if (coef.empty()) return fail(ctx, STK_INVALID_PARAMS, "weighted: no frame included");
    if ((st = weighted_check_coefs(ctx, coef, cn))) return st;
    std::vector<int> entry_frame;
    if ((st = weighted_table(ctx, frames, M, include, is_affine, entry_frame))) return st;
    const int ne = (int)entry_frame.size();
    const bool host = frames->location != STK_DEVICE;       // the planes are where the frames are
    const LocalLayout L = local_layout((size_t)ne, ne, w, h, cn, host ? (size_t)ne : 0);
    if ((st = local_reserve(ctx, L, host ? (size_t)ne : 0))) return st;
    char* base = ctx->local.as<char>();
    std::vector<const float*> mptr(ne);
    for (int k = 0; k < ne; k++) {
        if (host) {
            float* d = (float*)(base + L.planes + (size_t)k * L.plane);
            HIP_TRY(hipMemcpyAsync(d, maps[entry_frame[k]], (size_t)w * h * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            mptr[k] = d;
        } else mptr[k] = maps[entry_frame[k]];
    }
    HIP_TRY(hipMemcpyAsync(base + L.mptrs, mptr.data(), (size_t)ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    double ms = 0.0;
    MeshFoldArgs mf{};
    if (fields && (st = mesh_fold_table(ctx, frames, entry_frame, fields, step, &mf))) return st;
    // (local_fold synchronises: `mptr` outlives the copy)
    if ((st = local_fold(ctx, L, coef, frames->depth, w, h, cn, frame_row_bytes(frames), alpha, is_affine, floor, power, out, den_out, &ms,
                         fields ? &mf : nullptr)))
        return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

extern "C" {

stk_status stk_ecc_match_local_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                        const stk_weight_params* weight, const float* weights, const stk_local_params* local,
                                        stk_image_f32* out, float* den_out, stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = local_match_check(ctx, frames, weight, local, out);
    if (st) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const LocalLayout L = local_layout((size_t)n, n, w, h, cn, (size_t)n);
    if ((st = local_reserve(ctx, L, (size_t)n))) return st;
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    // the plain call, on this context's own device, its mean into the workspace image (unused)
    stk_image_f32 mimg{(float*)(ctx->local.as<char>() + L.image), w, h, cn, STK_DEVICE, 0};
    if ((st = ecc_match_single(ctx, frames, params, scale_down_width, &mimg, stats))) return st;
    const stk_timing keep = ctx->timing;
    // every frame is a sample: frame 0 through the identity, frame i through its warp (as in stk_ecc_match_weighted)
    const int is_affine = params->motion_type != STK_MOTION_HOMOGRAPHY;
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    std::vector<WarpFrame> wf(n);
    std::vector<int> entry_frame(n);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    make_warp_frame(wf[0], dev[0], I3, is_affine);
    for (int i = 1; i < n; i++) make_warp_frame(wf[i], dev[i], stats[i].warp, is_affine);
    for (int i = 0; i < n; i++) entry_frame[i] = i;
    const size_t rb = frame_row_bytes(frames);
    if ((st = warp_table_upload(ctx, wf, rb, w, h, is_affine))) return st;
    st = local_finish(ctx, L, frames, entry_frame, dev, rb, is_affine, weight, weights, local, out, den_out, applied);
    const double fin = ctx->timing.finalize_ms;
    ctx->timing = keep; ctx->timing.finalize_ms = st ? 0.0 : fin;
    return st;
}

stk_status stk_keypoint_match_local_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                             float scale_down_width, const stk_weight_params* weight, const float* weights,
                                             const stk_local_params* local, stk_image_f32* out, int32_t* dropped, float* den_out,
                                             stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = local_match_check(ctx, frames, weight, local, out);
    if (st) return st;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null parameters");
    if ((st = local_check_border(ctx, params->border_mode, params->border_value))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const LocalLayout L = local_layout((size_t)n, n, w, h, cn, (size_t)n);
    if ((st = local_reserve(ctx, L, (size_t)n))) return st;
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    stk_image_f32 mimg{(float*)(ctx->local.as<char>() + L.image), w, h, cn, STK_DEVICE, 0};
    if ((st = keypoint_match_single(ctx, frames, params, scale_down_width, &mimg, dropped, stats))) return st;
    const stk_timing keep = ctx->timing;
    // the samples: frame 0 through the identity and the frames with a homography (status 0), in stack order (as in
    // stk_keypoint_match_weighted)
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    std::vector<WarpFrame> wf;
    std::vector<int> entry_frame;
    wf.reserve(n);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    wf.emplace_back();
    make_warp_frame(wf.back(), dev[0], I3, 0);
    entry_frame.push_back(0);
    for (int i = 1; i < n; i++) {
        if (stats[i].status != 0) continue;
        wf.emplace_back();
        make_warp_frame(wf.back(), dev[i], stats[i].warp, 0);
        entry_frame.push_back(i);
    }
    const size_t rb = frame_row_bytes(frames);
    if ((st = warp_table_upload(ctx, wf, rb, w, h, 0))) return st;
    st = local_finish(ctx, L, frames, entry_frame, dev, rb, 0, weight, weights, local, out, den_out, applied);
    const double fin = ctx->timing.finalize_ms;
    ctx->timing = keep; ctx->timing.finalize_ms = st ? 0.0 : fin;
    return st;
}

}  // extern "C"
