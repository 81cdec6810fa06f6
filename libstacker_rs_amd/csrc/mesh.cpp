// mesh.cpp — local alignment: stk_mesh_grid, stk_local_align, stk_mesh_stack, stk_mesh_local_weighted_stack,
// stk_ecc_match_local_aligned, stk_keypoint_match_local_aligned, and the coarse-to-fine forms stk_grey_pyramid,
// stk_local_align_pyramid, stk_*_match_local_aligned_pyramid (an extension beyond the reference; definition in
// include/stacker.h, stk_mesh_params; kernels in kernels_mesh.hip and warp_body.h).
// ctx->mesh (grow-only like the other workspaces) holds three pointer tables indexed like the frame table (the fold's
// fields, the field pass's fields and status planes), the field and status planes the caller does not hold on the device,
// the fill pass's scratch and a w x h x cn f32 image (the plain call's mean in the whole-stack forms, then a host output's
// staging copy); behind that, for the coarse-to-fine forms, what PyrLayout lists. The frame table is combine.h's; the local-weighted fold and its map pass are the local combine's
// (local.cpp, through context.h). Like the other combines, the whole-stack forms run the plain
// call first and take the warps and the kept set from its stats; the frames are still resident in HBM, full size.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

namespace {

stk_status local_align_impl(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                            const stk_mesh_params* p, int levels, float* const* fields, int32_t* const* status);

void mesh_grid_of(int w, int h, int step, int* gw, int* gh) {
    const NodeGrid g = node_grid(w, h, step);
    *gw = g.gw; *gh = g.gh;
}

stk_status mesh_validate(stk_ctx* ctx, const stk_mesh_params* p) {
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null mesh parameters");
    if (!grid_step_ok(p->step)) return fail(ctx, STK_INVALID_PARAMS, "mesh: step must be 8, 16, 32, 64, 128 or 256");
    if (p->radius < 2 || p->radius > 32) return fail(ctx, STK_INVALID_PARAMS, "mesh: radius must be 2 .. 32");
    if (p->max_iters < 1 || p->max_iters > 32) return fail(ctx, STK_INVALID_PARAMS, "mesh: max_iters must be 1 .. 32");
    if (!std::isfinite(p->epsilon) || p->epsilon < 0.0f) return fail(ctx, STK_INVALID_PARAMS, "mesh: epsilon must be finite and >= 0");
    if (!std::isfinite(p->max_shift) || !(p->max_shift > 0.0f) || p->max_shift > 64.0f)
        return fail(ctx, STK_INVALID_PARAMS, "mesh: max_shift must be finite, > 0 and <= 64");
    if (!std::isfinite(p->min_eig) || p->min_eig < 0.0f) return fail(ctx, STK_INVALID_PARAMS, "mesh: min_eig must be finite and >= 0");
    if (p->fill < 0 || p->fill > 16) return fail(ctx, STK_INVALID_PARAMS, "mesh: fill must be 0 .. 16");
    if (p->reserved != 0) return fail(ctx, STK_INVALID_PARAMS, "mesh parameters: reserved must be 0");
    return STK_OK;
}

stk_status mesh_check_depth(stk_ctx* ctx, const stk_frames* f) {
    if (f->depth != 8)
        return fail(ctx, STK_NOT_IMPLEMENTED,
                    "local alignment takes 8-bit frames: the displacement is estimated on the 8-bit integer grey, its gradients are exact integers");
    return STK_OK;
}

// The field pass over entries 1 .. ne - 1 of ctx->warpframes (entry 0 = frame 0; the table is uploaded): fdev[k] / sdev[k]
// are the device planes of entry k (sdev[k] never null; index 0 unused). Tables at L.fptrs / L.sptrs, fill scratch at
// L.scratch (ne - 1 planes). Synchronises; adds the device time of the two kernels to *ms.
stk_status mesh_align_entries(stk_ctx* ctx, const MeshLayout& L, int ne, int w, int h, int cn, size_t rb, int is_affine,
                              const stk_mesh_params* p, int gw, int gh, const std::vector<float*>& fdev, const std::vector<int32_t*>& sdev,
                              double* ms) {
    if (ne < 2) return STK_OK;
    char* base = ctx->mesh.as<char>();
    HIP_TRY(hipMemcpyAsync(base + L.fptrs, fdev.data(), (size_t)ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(base + L.sptrs, sdev.data(), (size_t)ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    MeshLkArgs a{};
    a.frames = ctx->warpframes.as<WarpFrame>();
    a.fields = (float* const*)(base + L.fptrs);
    a.status = (int* const*)(base + L.sptrs);
    a.n_entries = ne;
    a.w = w; a.h = h; a.stride = rb; a.is_affine = is_affine;
    a.step = p->step; a.gw = gw; a.gh = gh; a.radius = p->radius; a.max_iters = p->max_iters;
    a.eps2 = (double)p->epsilon * (double)p->epsilon;
    a.max_shift2 = (double)p->max_shift * (double)p->max_shift;
    a.min_eig4 = 4.0 * (double)p->min_eig;
    if (stk_status st = combine_begin(ctx)) return st;
    HIP_TRY(launch_mesh_lk(a, cn, ctx->stream));
    if (p->fill > 0)
        HIP_TRY(launch_mesh_fill(a.fields, (const int* const*)a.status, ne, gw, gh, p->fill, base + L.scratch, ctx->stream));
    return combine_end(ctx, ms);                         // (synchronises: the pointer vectors leave scope)
}

// The mesh mean fold over the ne entries of ctx->warpframes with the field table `mf`: sums in fold order, then x
// (float)(1.0 / ne). `image`: a w x h x cn f32 device buffer for a host output. Synchronises; adds its device time to *ms.
stk_status mesh_mean_fold(stk_ctx* ctx, int ne, const FoldSpec& spec, const MeshFoldArgs& mf, float* image, stk_image_f32* out, double* ms) {
    const size_t nel = (size_t)spec.w * spec.h * spec.cn;
    const CombineOutputs o(out, image, nel);
    WarpArgs a = fold_warp_args(ctx, ne, spec);
    a.acc = o.image();
    a.acc_stride = (size_t)spec.w * spec.cn;
    a.accumulate = 0;
    ClipArgs ca{};
    mesh_fold_clip_args(mf, ca);
    if (stk_status st = combine_begin(ctx)) return st;
    HIP_TRY(launch_mesh_fold(a, ca, spec.depth, false, ctx->stream));
    HIP_TRY(launch_scale(a.acc, a.acc, nel, (float)(1.0 / (double)ne), ctx->stream));
    return combine_end(ctx, ms, &o);
}

// ---- the coarse-to-fine form (include/stacker.h, "coarse-to-fine local alignment") -------------------------------------
// What it keeps in ctx->mesh behind a MeshLayout: PyrLayout (workspace.h).
stk_status pyr_validate(stk_ctx* ctx, const stk_frames* f, const stk_mesh_params* p, int levels) {
    if (levels < 1 || levels > 4) return fail(ctx, STK_INVALID_PARAMS, "mesh: levels must be 1 .. 4");
    if ((p->step >> (levels - 1)) < 4) return fail(ctx, STK_INVALID_PARAMS, "mesh: step >> (levels - 1) must be at least 4");
    if ((std::min(f->width, f->height) >> (levels - 1)) < 16)
        return fail(ctx, STK_INVALID_PARAMS, "mesh: min(width, height) >> (levels - 1) must be at least 16");
    return STK_OK;
}

// C_l^-1 inv C_l in double, in the header's order of operations
void pyr_level_matrix(const double* inv, int level, double* o) {
    const double s = (double)(1 << level), c = 0.5 * (s - 1.0), is = 1.0 / s, cs = c * is;
    double A[9];
    for (int r = 0; r < 3; r++) {
        A[3 * r] = inv[3 * r] * s;
        A[3 * r + 1] = inv[3 * r + 1] * s;
        A[3 * r + 2] = (inv[3 * r] * c + inv[3 * r + 1] * c) + inv[3 * r + 2];
    }
    for (int j = 0; j < 3; j++) {
        o[j] = A[j] * is - cs * A[6 + j];
        o[3 + j] = A[3 + j] * is - cs * A[6 + j];
        o[6 + j] = A[6 + j];
    }
}

// mesh_align_entries, coarse to fine: the pyramid of entries (build_ref ? 0 : 1) .. ne - 1, then per level from the top the
// seeded estimation and the fill on the carried validity, all in stream order. fwd[k]: the forward matrix of entry k (k >= 1),
// the one its uploaded table entry was made from. Synchronises; adds the device time of the levels to *ms and of the
// pyramid pass to *pyr_ms.
stk_status mesh_align_entries_pyr(stk_ctx* ctx, const MeshLayout& L, const PyrLayout& P, int ne, int w, int h, int cn, size_t rb,
                                  int is_affine, const stk_mesh_params* p, int levels, int gw, int gh, const std::vector<float*>& fdev,
                                  const std::vector<int32_t*>& sdev, const std::vector<const double*>& fwd, bool build_ref, double* ms,
                                  double* pyr_ms) {
    if (ne < 2) return STK_OK;
    char* base = ctx->mesh.as<char>();
    std::vector<uint8_t*> vdev(ne, nullptr);
    for (int k = 1; k < ne; k++) vdev[k] = (uint8_t*)(base + P.valid + (size_t)k * P.vplane);
    HIP_TRY(hipMemcpyAsync(base + L.fptrs, fdev.data(), (size_t)ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(base + L.sptrs, sdev.data(), (size_t)ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(base + P.vptrs, vdev.data(), (size_t)ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    std::vector<WarpFrame> lt((size_t)(levels - 1) * ne);
    for (int l = 1; l < levels; l++) {
        for (int k = 0; k < ne; k++) {
            WarpFrame& f = lt[(size_t)(l - 1) * ne + k];
            WarpFrame full;
            warp_frame_make(full, nullptr, k ? fwd[k] : IDENTITY3, is_affine);
            pyr_level_matrix(full.Md, l, f.Md);
            for (int q = 0; q < 9; q++) f.M[q] = (float)f.Md[q];
            f.src = base + P.planes + (size_t)k * P.pstride + mesh_pyr_offset(w, h, l);
            f.flags = 0;
        }
        HIP_TRY(hipMemcpyAsync(base + P.tables + (size_t)(l - 1) * P.tbytes, &lt[(size_t)(l - 1) * ne], (size_t)ne * sizeof(WarpFrame),
                               hipMemcpyHostToDevice, ctx->stream));
    }
    if (stk_status st = combine_begin(ctx)) return st;
    MeshPyrArgs pa{};
    pa.frames = ctx->warpframes.as<WarpFrame>();
    pa.planes = (uint8_t*)(base + P.planes);
    pa.entry_stride = P.pstride; pa.stride = rb;
    pa.first = build_ref ? 0 : 1; pa.n = ne - pa.first;
    pa.w = w; pa.h = h; pa.levels = levels;
    HIP_TRY(launch_mesh_pyr(pa, cn, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[6], ctx->stream));
    for (int l = levels - 1; l >= 0; l--) {
        MeshLkArgs a{};
        a.frames = l ? (const WarpFrame*)(base + P.tables + (size_t)(l - 1) * P.tbytes) : ctx->warpframes.as<WarpFrame>();
        a.fields = (float* const*)(base + L.fptrs);
        a.status = l ? nullptr : (int* const*)(base + L.sptrs);
        a.valid = (uint8_t* const*)(base + P.vptrs);
        a.n_entries = ne;
        a.w = w >> l; a.h = h >> l; a.stride = l ? (size_t)(w >> l) : rb; a.is_affine = is_affine;
        a.step = p->step; a.gw = gw; a.gh = gh; a.radius = p->radius; a.max_iters = p->max_iters;
        a.level = l; a.top = l == levels - 1;
        const float max_shift = p->max_shift * (1.0f / (float)(1 << l));
        a.eps2 = (double)p->epsilon * (double)p->epsilon;
        a.max_shift2 = (double)max_shift * (double)max_shift;
        a.min_eig4 = 4.0 * (double)p->min_eig;
        HIP_TRY(launch_mesh_lk_seeded(a, l ? 1 : cn, ctx->stream));
        HIP_TRY(launch_mesh_fill_valid(a.fields, a.valid, ne, gw, gh, p->fill, base + L.scratch, ctx->stream));
    }
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));          // the host tables leave scope
    if (ms) *ms += ev_ms(ctx->ev[6], ctx->ev[5]);
    if (pyr_ms) *pyr_ms += ev_ms(ctx->ev[4], ctx->ev[6]);
    return STK_OK;
}

// the checks the two whole-stack forms share, in the order the errors are reported
stk_status mesh_match_check(stk_ctx* ctx, const stk_frames* frames, const stk_mesh_params* mesh, const stk_local_params* local,
                            const stk_image_f32* out) {
    stk_status st = mesh_validate(ctx, mesh);
    if (st) return st;
    if (local && (st = local_validate(ctx, local))) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = mesh_check_fold(ctx, mesh->step))) return st;
    if ((st = mesh_check_depth(ctx, frames))) return st;
    return combine_check_out(ctx, out, frames);
}

// The field pass of a whole-stack form over the ne entries of ctx->warpframes (entry 0 = frame 0; the table is uploaded):
// the planes of entries 1 .. ne - 1 into L.fields, then the fold's pointer table (entry 0: null) at L.tptrs. Synchronises;
// adds the pass's device time to *ms.
// levels > 0: the coarse-to-fine pass (P: its layout behind L; fwd: the entries' forward matrices).
stk_status mesh_entry_fields(stk_ctx* ctx, const MeshLayout& L, int ne, int w, int h, int cn, size_t rb, int is_affine,
                             const stk_mesh_params* mp, MeshFoldArgs* out, double* ms, int levels = 0, const PyrLayout* P = nullptr,
                             const std::vector<const double*>* fwd = nullptr) {
    int gw, gh;
    mesh_grid_of(w, h, mp->step, &gw, &gh);
    char* base = ctx->mesh.as<char>();
    std::vector<float*> fdev(ne, nullptr);
    std::vector<int32_t*> sdev(ne, nullptr);
    for (int k = 1; k < ne; k++) {
        fdev[k] = (float*)(base + L.fields + (size_t)(k - 1) * L.fplane);
        sdev[k] = (int32_t*)(base + L.status + (size_t)(k - 1) * L.splane);
    }
    stk_status st = levels > 0 ? mesh_align_entries_pyr(ctx, L, *P, ne, w, h, cn, rb, is_affine, mp, levels, gw, gh, fdev, sdev, *fwd, true, ms, ms)
                               : mesh_align_entries(ctx, L, ne, w, h, cn, rb, is_affine, mp, gw, gh, fdev, sdev, ms);
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(base + L.tptrs, fdev.data(), (size_t)ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));          // `fdev` leaves scope
    *out = MeshFoldArgs{(const float* const*)(base + L.tptrs), mp->step, gw, gh};
    return STK_OK;
}

// the workspaces of a whole-stack form over n frames, reserved before the plain call writes its mean into ctx->mesh
stk_status mesh_match_reserve(stk_ctx* ctx, const stk_frames* frames, const stk_mesh_params* mp, const stk_local_params* lp, MeshLayout* L,
                              int levels = 0, PyrLayout* P = nullptr) {
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    int gw, gh;
    mesh_grid_of(w, h, mp->step, &gw, &gh);
    *L = mesh_layout((size_t)n, (size_t)n, (size_t)n, (size_t)n, gw, gh, (size_t)w * h * cn);
    if (levels > 0) *P = pyr_layout(L->total, (size_t)n, gw, gh, w, h, levels);
    stk_status st = workspace_reserve(ctx, ctx->mesh, levels > 0 ? P->total : L->total, "mesh");
    if (st) return st;
    if (lp) {
        const LocalLayout LL = local_layout((size_t)n, n, w, h, cn, (size_t)n);
        if ((st = workspace_reserve(ctx, ctx->local, LL.total, "local"))) return st;
    }
    return STK_OK;
}

// the combine of the whole-stack forms over the kept frames (`dev`: the resident full-size frames by frame index): field
// pass, then the mesh mean fold, or the map pass and the mesh local-weighted fold with unit records
CombineFinish mesh_match_finish(stk_ctx* ctx, const MeshLayout& L, const stk_mesh_params* mp, const stk_local_params* lp, stk_image_f32* out,
                                int levels = 0, const PyrLayout& P = PyrLayout{}) {
    return [=](const EntryTable& table, const std::vector<const void*>& dev, const FoldSpec& spec, const stk_frame_stats*, double* ms) {
        const int ne = table.size(), w = spec.w, h = spec.h, cn = spec.cn;
        const size_t rb = spec.src_row_bytes;
        MeshFoldArgs mf{};
        stk_status st = mesh_entry_fields(ctx, L, ne, w, h, cn, rb, spec.is_affine, mp, &mf, ms, levels, &P, &table.M);
        if (st) return st;
        if (!lp) return mesh_mean_fold(ctx, ne, spec, mf, (float*)(ctx->mesh.as<char>() + L.image), out, ms);
        const LocalLayout LL = local_layout((size_t)ne, ne, w, h, cn, (size_t)ne);
        char* lbase = ctx->local.as<char>();
        std::vector<const void*> fptr(ne);
        std::vector<float*> mptr(ne);
        for (int k = 0; k < ne; k++) { fptr[k] = dev[table.frame[k]]; mptr[k] = (float*)(lbase + LL.planes + (size_t)k * LL.plane); }
        if ((st = local_maps_enqueue(ctx, LL, fptr, mptr))) return st;
        if ((st = combine_begin(ctx))) return st;
        if ((st = local_maps_launch(ctx, LL, 0, (size_t)ne, cn, w, h, rb, lp))) return st;
        if ((st = combine_end(ctx, ms))) return st;
        return local_fold(ctx, LL, std::vector<stk_frame_weight>(ne, unit_record()), spec, lp->floor, lp->power, out, nullptr, ms, &mf);
    };
}


}  // namespace

void mesh_fold_clip_args(const MeshFoldArgs& m, ClipArgs& ca) {
    ca.fields = m.fields;
    ca.mesh_shift = 0;
    while ((1 << ca.mesh_shift) < m.step) ca.mesh_shift++;
    ca.mesh_gw = m.gw; ca.mesh_gh = m.gh;
    ca.mesh_inv = 1.0f / (float)m.step;
}

stk_status mesh_check_fold(stk_ctx* ctx, int step) {
    if (!grid_step_ok(step)) return fail(ctx, STK_INVALID_PARAMS, "mesh: step must be 8, 16, 32, 64, 128 or 256");
    if (ctx->opt_subpixel_bits != 0)
        return fail(ctx, STK_INVALID_PARAMS, "mesh: the displaced coordinates are exact ones: warp_subpixel_bits must be 0");
    if (ctx->opt_interp == STK_INTER_CUBIC)
        return fail(ctx, STK_NOT_IMPLEMENTED, "mesh: the mesh folds are bilinear; warp_interpolation = 2 (STK_INTER_CUBIC) is not implemented for them");
    return STK_OK;
}

stk_status mesh_match_fields_check(stk_ctx* ctx, const stk_frames* frames, const stk_mesh_params* mp) {
    stk_status st = mesh_validate(ctx, mp);
    if (st) return st;
    return mesh_check_depth(ctx, frames);
}

stk_status mesh_match_fields_reserve(stk_ctx* ctx, const stk_frames* frames, const stk_mesh_params* mp) {
    const size_t n = (size_t)frames->n;
    int gw, gh;
    mesh_grid_of(frames->width, frames->height, mp->step, &gw, &gh);
    return workspace_reserve(ctx, ctx->mesh, mesh_layout(n, n, n, n, gw, gh, 0).total, "mesh");
}

stk_status mesh_match_fields(stk_ctx* ctx, const stk_frames* frames, int n_entries, int is_affine, const stk_mesh_params* mp,
                             MeshFoldArgs* out, double* ms) {
    const size_t n = (size_t)frames->n;
    int gw, gh;
    mesh_grid_of(frames->width, frames->height, mp->step, &gw, &gh);
    return mesh_entry_fields(ctx, mesh_layout(n, n, n, n, gw, gh, 0), n_entries, frames->width, frames->height, frames->channels,
                             frame_row_bytes(frames), is_affine, mp, out, ms);
}

stk_status mesh_fold_table(stk_ctx* ctx, const stk_frames* frames, const EntryTable& table, const float* const* fields, int step,
                           MeshFoldArgs* out) {
    const int ne = table.size();
    const bool host = frames->location != STK_DEVICE;
    int gw, gh;
    mesh_grid_of(frames->width, frames->height, step, &gw, &gh);
    const MeshLayout L = mesh_layout((size_t)ne, host ? (size_t)ne : 0, 0, 0, gw, gh, (size_t)frames->width * frames->height * frames->channels);
    stk_status st = workspace_reserve(ctx, ctx->mesh, L.total, "mesh");
    if (st) return st;
    char* base = ctx->mesh.as<char>();
    std::vector<const float*> ptr(ne, nullptr);
    for (int k = 0; k < ne; k++) {
        const int i = table.frame[k];
        if (i == 0 || !fields[i]) continue;                // frame 0 is the grid's own frame; a null plane: not displaced
        if (host) {
            float* d = (float*)(base + L.fields + (size_t)k * L.fplane);
            HIP_TRY(hipMemcpyAsync(d, fields[i], (size_t)gw * gh * 2 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            ptr[k] = d;
        } else ptr[k] = fields[i];
    }
    HIP_TRY(hipMemcpyAsync(base + L.tptrs, ptr.data(), (size_t)ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));          // `ptr` leaves scope
    *out = MeshFoldArgs{(const float* const*)(base + L.tptrs), step, gw, gh};
    return STK_OK;
}

extern "C" {

stk_status stk_mesh_grid(int32_t width, int32_t height, int32_t step, int32_t* gw, int32_t* gh) {
    if (width <= 0 || height <= 0 || !grid_step_ok(step) || !gw || !gh) return STK_INVALID_PARAMS;
    mesh_grid_of(width, height, step, gw, gh);
    return STK_OK;
}

stk_status stk_local_align(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                           const stk_mesh_params* p, float* const* fields, int32_t* const* status) {
    return local_align_impl(ctx, frames, M, include, is_affine, p, 0, fields, status);
}

stk_status stk_local_align_pyramid(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                   const stk_mesh_params* p, int32_t levels, float* const* fields, int32_t* const* status) {
    stk_status st = check_frames(ctx, frames, false, false);
    if (st) return st;
    if ((st = mesh_validate(ctx, p))) return st;
    if ((st = pyr_validate(ctx, frames, p, levels))) return st;
    return local_align_impl(ctx, frames, M, include, is_affine, p, levels, fields, status);
}

stk_status stk_grey_pyramid(stk_ctx* ctx, const stk_frames* frame, int32_t levels, uint8_t* const* planes) {
    stk_status st = check_frames(ctx, frame, false, false);
    if (st) return st;
    if (frame->n != 1) return fail(ctx, STK_INVALID_PARAMS, "grey pyramid: one frame expected");
    if ((st = mesh_check_depth(ctx, frame))) return st;
    const int w = frame->width, h = frame->height, cn = frame->channels;
    if (levels < 2 || levels > 4) return fail(ctx, STK_INVALID_PARAMS, "grey pyramid: levels must be 2 .. 4");
    if ((std::min(w, h) >> (levels - 1)) < 1) return fail(ctx, STK_INVALID_PARAMS, "grey pyramid: min(width, height) >> (levels - 1) must be at least 1");
    if (!planes) return fail(ctx, STK_INVALID_PARAMS, "null planes");
    for (int l = 1; l < levels; l++)
        if (!planes[l]) return fail(ctx, STK_INVALID_PARAMS, "null pyramid plane");
    (void)hipSetDevice(ctx->device);
    timing_begin(ctx);
    const size_t rb = frame_row_bytes(frame), fb = rb * h;
    const bool host = frame->location == STK_HOST;
    const void* src = frame->data[0];
    if (host) {
        if ((st = workspace_reserve(ctx, ctx->frames, fb, "grey pyramid frame"))) return st;
        HIP_TRY(hipMemcpyAsync(ctx->frames.p, frame->data[0], frame_copy_bytes(frame), hipMemcpyHostToDevice, ctx->stream));
        src = ctx->frames.p;
    }
    const size_t bytes = mesh_pyr_offset(w, h, levels);
    if ((st = workspace_reserve(ctx, ctx->mesh, bytes, "mesh pyramid planes"))) return st;
    std::vector<WarpFrame> wf(1);
    make_warp_frame(wf[0], src, IDENTITY3, 1);
    if ((st = warp_table_upload(ctx, wf, rb, w, h, 1))) return st;
    MeshPyrArgs pa{};
    pa.frames = ctx->warpframes.as<WarpFrame>();
    pa.planes = ctx->mesh.as<uint8_t>();
    pa.entry_stride = bytes; pa.stride = rb; pa.first = 0; pa.n = 1; pa.w = w; pa.h = h; pa.levels = levels;
    if ((st = combine_begin(ctx))) return st;
    HIP_TRY(launch_mesh_pyr(pa, cn, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    for (int l = 1; l < levels; l++)
        HIP_TRY(hipMemcpyAsync(planes[l], pa.planes + mesh_pyr_offset(w, h, l), (size_t)(w >> l) * (size_t)(h >> l),
                               host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));          // `wf` leaves scope
    ctx->timing.prep_ms = ev_ms(ctx->ev[4], ctx->ev[5]);
    return STK_OK;
}

stk_status stk_ecc_match_local_aligned_pyramid(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                               const stk_mesh_params* mesh, int32_t levels, const stk_local_params* local,
                                               stk_image_f32* out, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = mesh_match_check(ctx, frames, mesh, local, out);
    if (st) return st;
    if ((st = pyr_validate(ctx, frames, mesh, levels))) return st;
    MeshLayout L;
    PyrLayout P;
    if ((st = mesh_match_reserve(ctx, frames, mesh, local, &L, levels, &P))) return st;
    return ecc_match_then(ctx, frames, params, scale_down_width, (float*)(ctx->mesh.as<char>() + L.image), stats,
                          mesh_match_finish(ctx, L, mesh, local, out, levels, P));
}

stk_status stk_keypoint_match_local_aligned_pyramid(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                                    float scale_down_width, const stk_mesh_params* mesh, int32_t levels,
                                                    const stk_local_params* local, stk_image_f32* out, int32_t* dropped,
                                                    stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = mesh_match_check(ctx, frames, mesh, local, out);
    if (st) return st;
    if ((st = pyr_validate(ctx, frames, mesh, levels))) return st;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null parameters");
    if (local && (st = local_check_border(ctx, params->border_mode, params->border_value))) return st;
    MeshLayout L;
    PyrLayout P;
    if ((st = mesh_match_reserve(ctx, frames, mesh, local, &L, levels, &P))) return st;
    return keypoint_match_then(ctx, frames, params, scale_down_width, (float*)(ctx->mesh.as<char>() + L.image), dropped, stats,
                               mesh_match_finish(ctx, L, mesh, local, out, levels, P));
}

}  // extern "C"

namespace {

// stk_local_align (levels = 0: the single-level kernel) and stk_local_align_pyramid (levels >= 1, checked)
stk_status local_align_impl(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                            const stk_mesh_params* p, int levels, float* const* fields, int32_t* const* status) {
    stk_status st = check_frames(ctx, frames, false, false);
    if (st) return st;
    if ((st = mesh_validate(ctx, p))) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (!fields) return fail(ctx, STK_INVALID_PARAMS, "null fields");
    if ((st = mesh_check_depth(ctx, frames))) return st;
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    std::vector<int> moving;
    for (int i = 1; i < n; i++) {
        if (include && !include[i]) continue;
        if (!fields[i]) return fail(ctx, STK_INVALID_PARAMS, "null field plane of an included frame");
        moving.push_back(i);
    }
    (void)hipSetDevice(ctx->device);
    timing_begin(ctx);
    if (moving.empty()) return STK_OK;
    int gw, gh;
    mesh_grid_of(w, h, p->step, &gw, &gh);
    const size_t nn = (size_t)gw * gh, rb = frame_row_bytes(frames), fb = rb * h;
    const bool host = frames->location == STK_HOST;
    // host frames go through the frame workspace in batches that fit it (at least "upload_batch" frames, and frame 0 with
    // one more), as in stk_local_sharpness: frame 0 stays in the first place, a batch's frames follow it
    int batch = (int)moving.size();
    if (host) {
        const size_t budget = std::max<size_t>(ctx->frames.cap, (size_t)ctx->opt_upload_batch * fb);
        batch = (int)std::min<size_t>(moving.size(), std::max<size_t>(2, budget / fb) - 1);
        if ((st = workspace_reserve(ctx, ctx->frames, fb * (size_t)(batch + 1), "local alignment frames"))) return st;
        HIP_TRY(hipMemcpyAsync(ctx->frames.p, frames->data[0], frame_copy_bytes(frames), hipMemcpyHostToDevice, ctx->stream));
    }
    const MeshLayout L = mesh_layout((size_t)batch + 1, host ? (size_t)batch : 0, (size_t)batch, (size_t)batch, gw, gh, 0);
    PyrLayout P{};
    if (levels > 0) P = pyr_layout(L.total, (size_t)batch + 1, gw, gh, w, h, levels);
    if ((st = workspace_reserve(ctx, ctx->mesh, std::max(L.total, P.total), "mesh"))) return st;
    char* base = ctx->mesh.as<char>();
    double ms = 0.0, pyr_ms = 0.0;
    for (size_t b0 = 0; b0 < moving.size(); b0 += (size_t)batch) {
        const int nb = (int)std::min<size_t>((size_t)batch, moving.size() - b0);
        std::vector<WarpFrame> wf(nb + 1);
        std::vector<float*> fdev(nb + 1, nullptr);
        std::vector<int32_t*> sdev(nb + 1, nullptr);
        std::vector<const double*> fwd(nb + 1, nullptr);
        make_warp_frame(wf[0], host ? (const void*)ctx->frames.p : frames->data[0], IDENTITY3, is_affine);
        for (int k = 1; k <= nb; k++) {
            const int i = moving[b0 + k - 1];
            const void* src = frames->data[i];
            if (host) {
                void* d = ctx->frames.as<uint8_t>() + fb * (size_t)k;
                HIP_TRY(hipMemcpyAsync(d, frames->data[i], frame_copy_bytes(frames), hipMemcpyHostToDevice, ctx->stream));
                src = d;
            }
            make_warp_frame(wf[k], src, M + 9 * (size_t)i, is_affine);
            fwd[k] = M + 9 * (size_t)i;
            fdev[k] = host ? (float*)(base + L.fields + (size_t)(k - 1) * L.fplane) : fields[i];
            sdev[k] = (!host && status && status[i]) ? status[i] : (int32_t*)(base + L.status + (size_t)(k - 1) * L.splane);
        }
        if ((st = warp_table_upload(ctx, wf, rb, w, h, is_affine))) return st;
        // (mesh_align_entries synchronises: `wf` and the pointer vectors outlive the copies)
        if (levels > 0)
            st = mesh_align_entries_pyr(ctx, L, P, nb + 1, w, h, cn, rb, is_affine, p, levels, gw, gh, fdev, sdev, fwd, b0 == 0, &ms, &pyr_ms);
        else st = mesh_align_entries(ctx, L, nb + 1, w, h, cn, rb, is_affine, p, gw, gh, fdev, sdev, &ms);
        if (st) return st;
        if (host) {
            for (int k = 1; k <= nb; k++) {
                const int i = moving[b0 + k - 1];
                HIP_TRY(hipMemcpyAsync(fields[i], fdev[k], nn * 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
                if (status && status[i]) HIP_TRY(hipMemcpyAsync(status[i], sdev[k], nn * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            }
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
    }
    ctx->timing.align_ms = ms;
    ctx->timing.prep_ms = pyr_ms;
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_mesh_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                          int32_t border_mode, const double* border_value, double alpha, const float* const* fields, int32_t step,
                          stk_image_f32* out) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (!fields) return fail(ctx, STK_INVALID_PARAMS, "null fields");
    if ((st = check_border_mode(ctx, border_mode))) return st;
    if ((st = mesh_check_fold(ctx, step))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    EntryTable table;
    entries_from_include(frames->n, M, include, table);
    for (int i : table.frame)
        if (i > 0 && !fields[i]) return fail(ctx, STK_INVALID_PARAMS, "null field plane of an included frame");
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "weighted: no frame included");
    if ((st = entry_table_begin(ctx, frames, table, is_affine))) return st;
    MeshFoldArgs mf{};
    if ((st = mesh_fold_table(ctx, frames, table, fields, step, &mf))) return st;
    // (mesh_fold_table's layout: the image follows the planes it uploaded)
    const bool host = frames->location != STK_DEVICE;
    const size_t ne = table.frame.size();
    const MeshLayout L = mesh_layout(ne, host ? ne : 0, 0, 0, mf.gw, mf.gh, (size_t)frames->width * frames->height * frames->channels);
    double ms = 0.0;
    if ((st = mesh_mean_fold(ctx, (int)ne, fold_spec(frames, alpha, border_mode, border_value, is_affine), mf,
                             (float*)(ctx->mesh.as<char>() + L.image), out, &ms)))
        return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

stk_status stk_mesh_local_weighted_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                         int32_t border_mode, const double* border_value, double alpha, const stk_frame_weight* per_frame,
                                         const float* const* maps, float floor, int32_t power, const float* const* fields, int32_t step,
                                         stk_image_f32* out, float* den_out) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!fields) return fail(ctx, STK_INVALID_PARAMS, "null fields");
    return local_weighted_stack_impl(ctx, frames, M, include, is_affine, border_mode, border_value, alpha, per_frame, maps, floor, power,
                                     fields, step, out, den_out);
}

stk_status stk_ecc_match_local_aligned(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                       const stk_mesh_params* mesh, const stk_local_params* local, stk_image_f32* out,
                                       stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = mesh_match_check(ctx, frames, mesh, local, out);
    if (st) return st;
    MeshLayout L;
    if ((st = mesh_match_reserve(ctx, frames, mesh, local, &L))) return st;
    return ecc_match_then(ctx, frames, params, scale_down_width, (float*)(ctx->mesh.as<char>() + L.image), stats,
                          mesh_match_finish(ctx, L, mesh, local, out));
}

stk_status stk_keypoint_match_local_aligned(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                            float scale_down_width, const stk_mesh_params* mesh, const stk_local_params* local,
                                            stk_image_f32* out, int32_t* dropped, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = mesh_match_check(ctx, frames, mesh, local, out);
    if (st) return st;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null parameters");
    if (local && (st = local_check_border(ctx, params->border_mode, params->border_value))) return st;
    MeshLayout L;
    if ((st = mesh_match_reserve(ctx, frames, mesh, local, &L))) return st;
    return keypoint_match_then(ctx, frames, params, scale_down_width, (float*)(ctx->mesh.as<char>() + L.image), dropped, stats,
                               mesh_match_finish(ctx, L, mesh, local, out));
}

}  // extern "C"
