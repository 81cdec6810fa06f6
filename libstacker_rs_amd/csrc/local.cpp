// local.cpp — per-pixel weight maps and local-sharpness (lucky-region) stacking: stk_local_sharpness,
// stk_local_weighted_stack, stk_ecc_match_local_weighted, stk_keypoint_match_local_weighted (an extension beyond the
// reference; definition in include/stacker.h, stk_local_params; kernels in kernels_local.hip and warp_body.h).
// ctx->local (grow-only like the other workspaces) holds the pointer tables of the map pass and of the fold, the per-entry
// gain / offset / weight table, a w x h x cn f32 image (the plain call's mean in the whole-stack forms, then a host
// output's staging copy), the w x h den plane and the map planes of the fold's entries. The frame table is combine.h's; the
// checks, the moments pass and the estimator are the weighted combine's (weighted.cpp, through context.h). Like weighted.cpp, the
// whole-stack forms run the plain call first and take the warps and the kept set from its stats; the frames are still
// resident in HBM, full size, and the maps of the entries are computed from them.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

// (the checks, the map pass and the fold are shared with mesh.cpp: context.h; the layout: workspace.h)
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

// what local_check_border has checked, written the one way the kernels have always been given it
FoldSpec local_border(FoldSpec spec) {
    spec.border_mode = STK_BORDER_CONSTANT; spec.border_value = nullptr;
    return spec;
}

}  // namespace

// a weight taken outside a frame means nothing: the fold runs under BORDER_CONSTANT with border value 0
stk_status local_check_border(stk_ctx* ctx, int border_mode, const double* border_value) {
    stk_status st = check_border_mode(ctx, border_mode);
    if (st) return st;
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
stk_status local_fold(stk_ctx* ctx, const LocalLayout& L, const std::vector<stk_frame_weight>& coef, const FoldSpec& spec, float floor,
                      int power, stk_image_f32* out, float* den_out, double* ms, const MeshFoldArgs* mesh) {
    const int w = spec.w, h = spec.h, cn = spec.cn, depth = spec.depth;
    char* base = ctx->local.as<char>();
    const CombineOutputs o(out, (float*)(base + L.image), (size_t)w * h * cn, {den_out, base + L.den, (size_t)w * h});
    const WarpArgs a = fold_warp_args(ctx, (int)coef.size(), local_border(spec));
    ClipArgs ca{};
    ca.coef = (const stk_frame_weight*)(base + L.coef);
    ca.coverage = 1;
    ca.out = o.image();
    ca.out_stride = (size_t)w * cn;
    ca.den = o.side<float>(0);
    ca.den_stride = (size_t)w;
    ca.maps = (const float* const*)(base + L.mptrs);
    ca.map_stride = (size_t)w;
    ca.floor = floor;
    ca.power = power;
    stk_status st = records_upload(ctx, base + L.coef, coef);
    if (st || (st = combine_begin(ctx))) return st;
    if (mesh) {
        mesh_fold_clip_args(*mesh, ca);
        HIP_TRY(launch_mesh_fold(a, ca, depth, true, ctx->stream));
    } else HIP_TRY(launch_local_fold(a, ca, depth, ctx->stream));
    return combine_end(ctx, ms, &o);
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
    return combine_check_out(ctx, out, frames);
}

// their workspace (the plain call's mean lands in its image, unused)
stk_status local_match_reserve(stk_ctx* ctx, const stk_frames* frames, LocalLayout* L) {
    (void)hipSetDevice(ctx->device);
    const int n = frames->n;
    *L = local_layout((size_t)n, n, frames->width, frames->height, frames->channels, (size_t)n);
    return workspace_reserve(ctx, ctx->local, L->total, "local");
}

// and their combine over the kept frames (`dev`: the resident full-size frames by frame index): map pass, records, fold
CombineFinish local_match_finish(stk_ctx* ctx, const LocalLayout& L, int n, const stk_weight_params* p, const float* weights,
                                 const stk_local_params* lp, stk_image_f32* out, float* den_out, stk_frame_weight* applied) {
    return [=](const EntryTable& table, const std::vector<const void*>& dev, const FoldSpec& plain, const stk_frame_stats*, double* ms) {
        const FoldSpec spec = local_border(plain);
        const int ne = table.size();
        char* base = ctx->local.as<char>();
        std::vector<const void*> fptr(ne);
        std::vector<float*> mptr(ne);
        for (int k = 0; k < ne; k++) { fptr[k] = dev[table.frame[k]]; mptr[k] = (float*)(base + L.planes + (size_t)k * L.plane); }
        stk_status st = local_maps_enqueue(ctx, L, fptr, mptr);
        if (st) return st;
        if ((st = combine_begin(ctx))) return st;
        if ((st = local_maps_launch(ctx, L, 0, (size_t)ne, spec.cn, spec.w, spec.h, spec.src_row_bytes, lp))) return st;
        if ((st = combine_end(ctx, ms))) return st;
        std::vector<stk_frame_weight> coef;
        if ((st = weighted_match_records(ctx, n, table, spec, p, weights, coef, applied, ms))) return st;
        return local_fold(ctx, L, coef, spec, lp->floor, lp->power, out, den_out, ms);
    };
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
        if ((st = workspace_reserve(ctx, ctx->frames, fb * (size_t)batch, "local sharpness frames"))) return st;
    }
    const size_t n_ptrs = host ? (size_t)batch : (size_t)n;
    const LocalLayout Lp = local_layout(n_ptrs, 0, w, h, 0, host ? (size_t)batch : 0);
    if ((st = workspace_reserve(ctx, ctx->local, Lp.total, "local"))) return st;
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
    if ((st = combine_check_out(ctx, out, frames))) return st;
    const int w = frames->width, h = frames->height, cn = frames->channels;
    EntryTable table;
    entries_from_include(frames->n, M, include, table);
    for (int i : table.frame) {
        if (!maps[i]) return fail(ctx, STK_INVALID_PARAMS, "null map plane of an included frame");
        if (fields && i > 0 && !fields[i]) return fail(ctx, STK_INVALID_PARAMS, "null field plane of an included frame");
    }
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "weighted: no frame included");
    std::vector<stk_frame_weight> coef;
    gather_records(table, per_frame, coef);
    if ((st = weighted_check_coefs(ctx, coef, cn))) return st;
    if ((st = entry_table_begin(ctx, frames, table, is_affine))) return st;
    const int ne = table.size();
    const bool host = frames->location != STK_DEVICE;       // the planes are where the frames are
    const LocalLayout L = local_layout((size_t)ne, ne, w, h, cn, host ? (size_t)ne : 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "local"))) return st;
    char* base = ctx->local.as<char>();
    std::vector<const float*> mptr(ne);
    for (int k = 0; k < ne; k++) {
        if (host) {
            float* d = (float*)(base + L.planes + (size_t)k * L.plane);
            HIP_TRY(hipMemcpyAsync(d, maps[table.frame[k]], (size_t)w * h * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            mptr[k] = d;
        } else mptr[k] = maps[table.frame[k]];
    }
    HIP_TRY(hipMemcpyAsync(base + L.mptrs, mptr.data(), (size_t)ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    double ms = 0.0;
    MeshFoldArgs mf{};
    if (fields && (st = mesh_fold_table(ctx, frames, table, fields, step, &mf))) return st;
    // (local_fold synchronises: `mptr` outlives the copy)
    if ((st = local_fold(ctx, L, coef, fold_spec(frames, alpha, border_mode, border_value, is_affine), floor, power, out, den_out, &ms,
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
    LocalLayout L;
    if ((st = local_match_reserve(ctx, frames, &L))) return st;
    return ecc_match_then(ctx, frames, params, scale_down_width, (float*)(ctx->local.as<char>() + L.image), stats,
                          local_match_finish(ctx, L, frames->n, weight, weights, local, out, den_out, applied));
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
    LocalLayout L;
    if ((st = local_match_reserve(ctx, frames, &L))) return st;
    return keypoint_match_then(ctx, frames, params, scale_down_width, (float*)(ctx->local.as<char>() + L.image), dropped, stats,
                               local_match_finish(ctx, L, frames->n, weight, weights, local, out, den_out, applied));
}

}  // extern "C"
