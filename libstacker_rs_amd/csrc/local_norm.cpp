// local_norm.cpp — local normalisation: stk_local_moments, stk_local_norm_estimate, stk_local_norm_stack,
// stk_quantile_stack_local_norm, stk_clip_stack_local_norm, stk_robust_clip_stack_local_norm, stk_ecc_match_local_normalized,
// stk_keypoint_match_local_normalized and their *_clipped forms (an extension beyond the reference; definition in
// include/stacker.h, "local normalisation"; kernels in kernels_local_norm.hip, warp_body.h and kernels_clip.hip).
// ctx->local (grow-only like the other workspaces; the local-weighted combine's buffer, laid out here by NormLayout) holds
// the plane pointer table of the fold, the per-entry record table, a w x h x cn f32 image (the plain call's mean in the
// whole-stack forms, then a host output's staging copy), the w x h den plane, the cell moments of the entries and their
// planes. The frame table is combine.h's; the checks and the per-channel formulas are the weighted combine's (weighted.cpp,
// through context.h); the quantile's bands and selection are robust.cpp's (quantile_bands_norm), the two clips are
// robust.cpp's and robust_clip.cpp's (clip_passes_norm, robust_clip_bands with a plane table), with their own workspaces.
// The estimator and the fill are plain host code without a context: stk_local_norm_estimate is what the whole-stack forms
// call per frame.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

void norm_fold_clip_args(const NormFoldArgs& n, ClipArgs& ca) {
    int shift = 0;
    while ((1 << shift) < n.step) shift++;
    ca.norm = n.planes;
    ca.norm_shift = shift; ca.norm_gw = n.gw; ca.norm_gh = n.gh;
    ca.norm_inv = 1.0f / (float)n.step;
}

namespace {

const char* norm_params_error(const stk_local_norm_params* p) {
    if (!p) return "null local normalisation parameters";
    if (!grid_step_ok(p->step)) return "local normalisation: step must be 8, 16, 32, 64, 128 or 256";
    if (p->stat_step < 0 || p->stat_step > 64) return "local normalisation: stat_step must be 0 .. 64";
    if (p->normalize < 0 || p->normalize > 3) return "local normalisation: normalize must be 0 .. 3";
    if (p->coverage < 0 || p->coverage > 1) return "local normalisation: coverage must be 0 or 1";
    if (p->min_count < 0) return "local normalisation: min_count must be >= 0";
    if (p->fill < 0 || p->fill > 16) return "local normalisation: fill must be 0 .. 16";
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return "local normalisation parameters: reserved must be 0";
    return nullptr;
}
stk_status norm_validate(stk_ctx* ctx, const stk_local_norm_params* p) {
    const char* e = norm_params_error(p);
    return e ? fail(ctx, STK_INVALID_PARAMS, e) : STK_OK;
}
int norm_stat_step(const stk_local_norm_params* p) { return p->stat_step ? p->stat_step : 4; }

// The cell moments pass over the n_entries entries of ctx->warpframes (uploaded for the w x h destination): (n_entries - 1)
// x cells x cn x 6 doubles into `host`, entry 1 first. Synchronises; adds its device time to *ms.
stk_status norm_moments(stk_ctx* ctx, const NormLayout& L, int n_entries, const FoldSpec& spec, const NodeGrid& g, int stat_step,
                        double* host, double* ms) {
    if (n_entries < 2) return STK_OK;
    if (n_entries - 1 > 65535) return fail(ctx, STK_INVALID_PARAMS, "local normalisation: at most 65536 frames");
    char* base = ctx->local.as<char>();
    const WarpArgs a = fold_warp_args(ctx, n_entries, spec);
    ClipArgs ca{};
    ca.cells = (double*)(base + L.cells);
    ca.step = stat_step;
    ca.cell_shift = g.shift; ca.cell_w = g.cw; ca.cell_h = g.ch;
    const CombineOutputs o(host, ca.cells, (size_t)(n_entries - 1) * g.cells() * spec.cn * 6, sizeof(double));
    if (stk_status st = combine_begin(ctx)) return st;
    HIP_TRY(launch_local_moments(a, ca, spec.depth, ctx->stream));
    return combine_end(ctx, ms, &o);
}

// The planes of the table's entries (host memory, indexed like the table; null = none) into ctx->local with their pointer
// table. Synchronises.
stk_status norm_planes_upload(stk_ctx* ctx, const NormLayout& L, const std::vector<const float*>& planes, const NodeGrid& g, int cn,
                              NormFoldArgs* out) {
    char* base = ctx->local.as<char>();
    const size_t ne = planes.size();
    std::vector<const float*> ptr(ne, nullptr);
    for (size_t k = 0; k < ne; k++) {
        if (!planes[k]) continue;
        float* d = (float*)(base + L.planes + k * L.plane);
        HIP_TRY(hipMemcpyAsync(d, planes[k], g.nodes() * 2 * cn * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        ptr[k] = d;
    }
    HIP_TRY(hipMemcpyAsync(base + L.ptrs, ptr.data(), ne * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));          // `ptr` leaves scope
    *out = NormFoldArgs{(const float* const*)(base + L.ptrs), g.step, g.gw, g.gh};
    return STK_OK;
}

// The locally normalised mean over the entries of ctx->warpframes with the records `coef` and the plane table `nf`. Writes
// `out` and `den_out` (out's location); adds its device time to *ms.
stk_status norm_fold(stk_ctx* ctx, const NormLayout& L, const std::vector<stk_frame_weight>& coef, const NormFoldArgs& nf,
                     const FoldSpec& spec, int coverage, stk_image_f32* out, float* den_out, double* ms) {
    const int w = spec.w, h = spec.h, cn = spec.cn;
    char* base = ctx->local.as<char>();
    const CombineOutputs o(out, (float*)(base + L.image), (size_t)w * h * cn, {den_out, base + L.den, (size_t)w * h});
    const WarpArgs a = fold_warp_args(ctx, (int)coef.size(), spec);
    ClipArgs ca{};
    ca.coef = (const stk_frame_weight*)(base + L.coef);
    ca.coverage = coverage;
    ca.out = o.image();
    ca.out_stride = (size_t)w * cn;
    ca.den = o.side<float>(0);
    ca.den_stride = (size_t)w;
    norm_fold_clip_args(nf, ca);
    stk_status st = records_upload(ctx, base + L.coef, coef);
    if (st || (st = combine_begin(ctx))) return st;
    HIP_TRY(launch_norm_fold(a, ca, spec.depth, ctx->stream));
    return combine_end(ctx, ms, &o);
}

// Which combine runs through the planes, and its side outputs: at most one of quantile / clip / mad is set (none: the
// mean). den belongs to the mean, counts to the quantile (w x h) or to a clip (w x h x cn), kept to a clip.
struct NormCombine {
    const stk_quantile_params* quantile = nullptr;
    const stk_clip_params* clip = nullptr;
    const stk_robust_clip_params* mad = nullptr;      // the median / MAD clip
    float* den = nullptr;
    int32_t* counts = nullptr;
    float* kept = nullptr;
    bool selects() const { return quantile || mad; }  // goes through the selection kernels: N <= 4096
};

// the combine over the entries of ctx->warpframes with the records `coef` and the plane table `nf`
stk_status norm_combine(stk_ctx* ctx, const NormLayout& L, const NormCombine& nc, const std::vector<stk_frame_weight>& coef,
                        const NormFoldArgs& nf, const FoldSpec& spec, int coverage, stk_image_f32* out, double* ms) {
    if (nc.quantile) return quantile_bands_norm(ctx, coef, spec, coverage, nc.quantile, nf, out, nc.counts, ms);
    if (nc.clip) return clip_passes_norm(ctx, coef, spec, coverage, nc.clip, nf, out, nc.counts, nc.kept, ms);
    if (nc.mad) return robust_clip_bands(ctx, (int)coef.size(), &coef, spec, coverage, nc.mad, out, nc.counts, nc.kept, ms, &nf);
    return norm_fold(ctx, L, coef, nf, spec, coverage, out, nc.den, ms);
}

// the caller-held-warps forms of the combines, after the combine's own checks
stk_status norm_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int is_affine, int border_mode,
                      const double* border_value, double alpha, const NormCombine& nc, const stk_frame_weight* per_frame,
                      const float* const* norm, int step, int coverage, stk_image_f32* out) {
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (!grid_step_ok(step)) return fail(ctx, STK_INVALID_PARAMS, "local normalisation: step must be 8, 16, 32, 64, 128 or 256");
    stk_status st = combine_check_out(ctx, out, frames);
    if (st) return st;
    const int w = frames->width, h = frames->height, cn = frames->channels;
    EntryTable table;
    entries_from_include(frames->n, M, include, table);
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "local normalisation: no frame included");
    if (nc.selects() && (st = quantile_check_count(ctx, table.size()))) return st;
    std::vector<stk_frame_weight> coef;
    gather_records(table, per_frame, coef);
    if ((st = weighted_check_coefs(ctx, coef, cn))) return st;
    if ((st = entry_table_begin(ctx, frames, table, is_affine))) return st;
    const int ne = table.size();
    const NodeGrid g = node_grid(w, h, step);
    const NormLayout L = norm_layout(ne, w, h, cn, g, false, true);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "local normalisation"))) return st;
    std::vector<const float*> planes(ne, nullptr);
    for (int k = 0; k < ne; k++) planes[k] = norm ? norm[table.frame[k]] : nullptr;
    NormFoldArgs nf{};
    if ((st = norm_planes_upload(ctx, L, planes, g, cn, &nf))) return st;
    const FoldSpec spec = fold_spec(frames, alpha, border_mode, border_value, is_affine);
    double ms = 0.0;
    st = norm_combine(ctx, L, nc, coef, nf, spec, coverage, out, &ms);
    ctx->timing.finalize_ms = st ? 0.0 : ms;
    return st;
}

// the checks the two whole-stack forms share, in the order the errors are reported
stk_status norm_match_check(stk_ctx* ctx, const stk_frames* frames, const stk_local_norm_params* p, const NormCombine& nc,
                            const stk_image_f32* out) {
    stk_status st = norm_validate(ctx, p);
    if (st) return st;
    if (nc.quantile && (st = quantile_validate(ctx, nc.quantile))) return st;
    if (nc.clip && (st = clip_validate(ctx, nc.clip))) return st;
    if (nc.mad && (st = robust_clip_validate(ctx, nc.mad))) return st;
    if (nc.quantile && nc.den) return fail(ctx, STK_INVALID_PARAMS, "local normalisation: den belongs to the mean, not to the quantile");
    if (!nc.quantile && !nc.clip && !nc.mad && nc.counts)
        return fail(ctx, STK_INVALID_PARAMS, "local normalisation: counts belong to the quantile, not to the mean");
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    if (nc.selects() && (st = quantile_check_count(ctx, frames->n))) return st;
    if (frames->n - 1 > 65535) return fail(ctx, STK_INVALID_PARAMS, "local normalisation: at most 65536 frames");
    return STK_OK;
}

// their workspace (the plain call's mean lands in its image, unused), sized for all n frames
stk_status norm_match_reserve(stk_ctx* ctx, const stk_frames* frames, const stk_local_norm_params* p, NormLayout* L) {
    (void)hipSetDevice(ctx->device);
    const NodeGrid g = node_grid(frames->width, frames->height, p->step);
    *L = norm_layout(frames->n, frames->width, frames->height, frames->channels, g, true, true);
    return workspace_reserve(ctx, ctx->local, L->total, "local normalisation");
}

// and their combine over the kept frames: cell moments, estimator, planes, then the combine
CombineFinish norm_match_finish(stk_ctx* ctx, const NormLayout& L, int n, const stk_local_norm_params* p, const NormCombine& nc,
                                const float* weights, stk_image_f32* out, float* const* norm_out, stk_frame_weight* applied) {
    return [=](const EntryTable& table, const std::vector<const void*>&, const FoldSpec& spec, const stk_frame_stats*, double* ms) {
        const int ne = table.size(), cn = spec.cn;
        const NodeGrid g = node_grid(spec.w, spec.h, p->step);
        const size_t rec = g.cells() * cn * 6, pl = g.nodes() * 2 * cn;
        std::vector<double> mom((size_t)std::max(ne - 1, 0) * rec);
        stk_status st = norm_moments(ctx, L, ne, spec, g, norm_stat_step(p), mom.data(), ms);
        if (st) return st;
        std::vector<stk_frame_weight> coef(ne, unit_record()), global(ne, unit_record());
        std::vector<float> store((size_t)std::max(ne - 1, 0) * pl);
        std::vector<const float*> planes(ne, nullptr);
        for (int k = 0; k < ne; k++) {
            coef[k].weight = weights ? weights[table.frame[k]] : 1.0f;
            if (k == 0) continue;
            float* P = store.data() + (size_t)(k - 1) * pl;
            if (stk_local_norm_estimate(spec.w, spec.h, cn, p, mom.data() + (size_t)(k - 1) * rec, P, &global[k], nullptr))
                return fail(ctx, STK_INVALID_PARAMS, "local normalisation: the estimator refused its arguments");
            planes[k] = P;
            if (norm_out && norm_out[table.frame[k]]) std::memcpy(norm_out[table.frame[k]], P, pl * sizeof(float));
        }
        if ((st = weighted_check_coefs(ctx, coef, cn))) return st;
        if (applied) {
            for (int i = 0; i < n; i++) { applied[i] = unit_record(); applied[i].weight = 0.0f; }
            for (int k = 0; k < ne; k++) { applied[table.frame[k]] = global[k]; applied[table.frame[k]].weight = coef[k].weight; }
        }
        NormFoldArgs nf{};
        if ((st = norm_planes_upload(ctx, L, planes, g, cn, &nf))) return st;
        return norm_combine(ctx, L, nc, coef, nf, spec, p->coverage, out, ms);
    };
}

// the two whole-stack forms of every combine: the plain call, then norm_match_finish over its kept frames
stk_status norm_match_ecc(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                          const stk_local_norm_params* norm, const NormCombine& nc, const float* weights, stk_image_f32* out,
                          float* const* norm_out, stk_frame_weight* applied, stk_frame_stats* stats) {
    stk_status st = norm_match_check(ctx, frames, norm, nc, out);
    if (st) return st;
    NormLayout L;
    if ((st = norm_match_reserve(ctx, frames, norm, &L))) return st;
    return ecc_match_then(ctx, frames, params, scale_down_width, (float*)(ctx->local.as<char>() + L.image), stats,
                          norm_match_finish(ctx, L, frames->n, norm, nc, weights, out, norm_out, applied));
}

stk_status norm_match_keypoint(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                               const stk_local_norm_params* norm, const NormCombine& nc, const float* weights, stk_image_f32* out,
                               int32_t* dropped, float* const* norm_out, stk_frame_weight* applied, stk_frame_stats* stats) {
    stk_status st = norm_match_check(ctx, frames, norm, nc, out);
    if (st) return st;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null parameters");
    // the mean alone needs the weighted combine's border under coverage = 1; participation puts no condition on it
    const bool mean = !nc.quantile && !nc.clip && !nc.mad;
    if (mean && norm->coverage && (st = weighted_check_border(ctx, params->border_mode, params->border_value, 1))) return st;
    NormLayout L;
    if ((st = norm_match_reserve(ctx, frames, norm, &L))) return st;
    return keypoint_match_then(ctx, frames, params, scale_down_width, (float*)(ctx->local.as<char>() + L.image), dropped, stats,
                               norm_match_finish(ctx, L, frames->n, norm, nc, weights, out, norm_out, applied));
}

// exactly one of the two clips of a *_local_normalized_clipped call
stk_status norm_clip_choice(stk_ctx* ctx, const stk_clip_params* clip, const stk_robust_clip_params* robust, int32_t* counts, float* kept,
                            NormCombine* nc) {
    if ((clip != nullptr) == (robust != nullptr))
        return fail(ctx, STK_INVALID_PARAMS, "local normalisation: exactly one of the sigma clip and the median / MAD clip parameters must be given");
    nc->clip = clip; nc->mad = robust; nc->counts = counts; nc->kept = kept;
    return STK_OK;
}

// the checks the two caller-held clip forms share: stk_clip_stack_weighted's, with the clip's own between
stk_status norm_clip_stack_check(stk_ctx* ctx, const stk_frames* frames, int border_mode, int coverage) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    // (as stk_clip_stack_weighted: coverage = 1 puts no condition on the border mode or value)
    if ((st = check_border_mode(ctx, border_mode))) return st;
    if (coverage < 0 || coverage > 1) return fail(ctx, STK_INVALID_PARAMS, "weighted: coverage must be 0 or 1");
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_local_norm_estimate(int32_t width, int32_t height, int32_t channels, const stk_local_norm_params* p, const double* cells,
                                   float* plane, stk_frame_weight* global_out, int32_t* valid_out) {
    if (norm_params_error(p) || width <= 0 || height <= 0 || (channels != 1 && channels != 3 && channels != 4) || !cells || !plane)
        return STK_INVALID_PARAMS;
    const int cn = channels;
    const NodeGrid g = node_grid(width, height, p->step);
    const int gw = g.gw, gh = g.gh, nn = gw * gh;
    const double min_count = (double)(p->min_count ? p->min_count : 16);
    // the global moments: all cells in row-major order
    std::vector<double> gm((size_t)cn * 6, 0.0);
    for (size_t q = 0; q < g.cells(); q++)
        for (int k = 0; k < cn * 6; k++) gm[k] = gm[k] + cells[q * cn * 6 + k];
    stk_frame_weight glob;
    weighted_estimate(gm.data(), cn, p->normalize, &glob);
    glob.weight = 1.0f;
    // per node: the window's moments, the formulas, the validity
    std::vector<uint8_t> valid((size_t)nn * cn, 0);
    std::vector<double> nm((size_t)cn * 6);
    for (int j = 0; j < gh; j++)
        for (int k = 0; k < gw; k++) {
            std::fill(nm.begin(), nm.end(), 0.0);
            for (int dj = -1; dj <= 0; dj++)
                for (int dk = -1; dk <= 0; dk++) {
                    const int J = j + dj, K = k + dk;
                    if (J < 0 || J >= g.ch || K < 0 || K >= g.cw) continue;
                    const double* cm = cells + ((size_t)J * g.cw + K) * cn * 6;
                    for (int q = 0; q < cn * 6; q++) nm[q] = nm[q] + cm[q];
                }
            stk_frame_weight e;
            weighted_estimate(nm.data(), cn, p->normalize, &e);
            const int node = j * gw + k;
            int bits = 0;
            for (int c = 0; c < cn; c++) {
                const bool ok = nm[(size_t)c * 6] >= min_count && !(e.flags & (1 << c)) && e.gain[c] >= 0.25f && e.gain[c] <= 4.0f;
                valid[(size_t)node * cn + c] = ok;
                bits |= ok ? 1 << c : 0;
                plane[(size_t)node * 2 * cn + c] = e.gain[c];
                plane[(size_t)node * 2 * cn + cn + c] = e.offset[c];
            }
            if (valid_out) valid_out[node] = bits;
        }
    // the fill: Jacobi passes per channel on (g, o), the mesh fill's arithmetic with the channel's validity as m
    std::vector<float> A(plane, plane + (size_t)nn * 2 * cn), B(A.size());
    std::vector<uint8_t> mb(valid.size());
    for (int pass = 0; pass < p->fill; pass++) {
        for (int i = 0; i < nn; i++) {
            const int j = i / gw, k = i - j * gw;
            for (int c = 0; c < cn; c++) {
                float d0 = A[(size_t)i * 2 * cn + c], d1 = A[(size_t)i * 2 * cn + cn + c];
                uint8_t m = valid[(size_t)i * cn + c];
                if (!m) {
                    float den = 0.0f, n0 = 0.0f, n1 = 0.0f;
                    for (int dj = -1; dj <= 1; dj++)
                        for (int dk = -1; dk <= 1; dk++) {
                            const int jj = j + dj, kk = k + dk;
                            if ((unsigned)jj >= (unsigned)gh || (unsigned)kk >= (unsigned)gw) continue;
                            const size_t q = (size_t)jj * gw + kk;
                            if (!valid[q * cn + c]) continue;
                            const float wgt = (float)((2 - (dj < 0 ? -dj : dj)) * (2 - (dk < 0 ? -dk : dk)));
                            den = den + wgt;
                            n0 = n0 + wgt * A[q * 2 * cn + c];
                            n1 = n1 + wgt * A[q * 2 * cn + cn + c];
                        }
                    if (den > 0.0f) { d0 = n0 / den; d1 = n1 / den; m = 1; }
                }
                B[(size_t)i * 2 * cn + c] = d0; B[(size_t)i * 2 * cn + cn + c] = d1; mb[(size_t)i * cn + c] = m;
            }
        }
        A.swap(B); valid.swap(mb);
    }
    for (int i = 0; i < nn; i++)
        for (int c = 0; c < cn; c++) {
            const bool m = valid[(size_t)i * cn + c] != 0;
            plane[(size_t)i * 2 * cn + c] = m ? A[(size_t)i * 2 * cn + c] : glob.gain[c];
            plane[(size_t)i * 2 * cn + cn + c] = m ? A[(size_t)i * 2 * cn + cn + c] : glob.offset[c];
        }
    if (global_out) *global_out = glob;
    return STK_OK;
}

stk_status stk_local_moments(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                             int32_t border_mode, const double* border_value, double alpha, int32_t step, int32_t stat_step,
                             double* moments) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (!moments) return fail(ctx, STK_INVALID_PARAMS, "null moments");
    if ((st = weighted_check_border(ctx, border_mode, border_value, 0))) return st;
    if (!grid_step_ok(step)) return fail(ctx, STK_INVALID_PARAMS, "local normalisation: step must be 8, 16, 32, 64, 128 or 256");
    if (stat_step < 1 || stat_step > 64) return fail(ctx, STK_INVALID_PARAMS, "local moments: stat_step must be 1 .. 64");
    if (include && !include[0]) return fail(ctx, STK_INVALID_PARAMS, "local moments: frame 0 must be included");
    const int n = frames->n, cn = frames->channels;
    EntryTable table;
    entries_from_include(n, M, include, table);
    if (table.frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "local normalisation: no frame included");
    if (table.size() - 1 > 65535) return fail(ctx, STK_INVALID_PARAMS, "local normalisation: at most 65536 frames");
    if ((st = entry_table_begin(ctx, frames, table, is_affine))) return st;
    const int ne = table.size();
    const NodeGrid g = node_grid(frames->width, frames->height, step);
    const NormLayout L = norm_layout(ne, frames->width, frames->height, cn, g, true, false);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "local normalisation"))) return st;
    const size_t rec = g.cells() * cn * 6;
    std::vector<double> mom((size_t)std::max(ne - 1, 0) * rec);
    double ms = 0.0;
    if ((st = norm_moments(ctx, L, ne, fold_spec(frames, alpha, border_mode, border_value, is_affine), g, stat_step, mom.data(), &ms)))
        return st;
    ctx->timing.finalize_ms = ms;
    std::memset(moments, 0, (size_t)n * rec * sizeof(double));
    for (int k = 1; k < ne; k++) std::memcpy(moments + (size_t)table.frame[k] * rec, mom.data() + (size_t)(k - 1) * rec, rec * sizeof(double));
    return STK_OK;
}

stk_status stk_local_norm_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                int32_t border_mode, const double* border_value, double alpha, const stk_frame_weight* per_frame,
                                const float* const* norm, int32_t step, int32_t coverage, stk_image_f32* out, float* den_out) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if ((st = weighted_check_border(ctx, border_mode, border_value, coverage))) return st;
    NormCombine nc;
    nc.den = den_out;
    return norm_stack(ctx, frames, M, include, is_affine, border_mode, border_value, alpha, nc, per_frame, norm, step, coverage, out);
}

stk_status stk_quantile_stack_local_norm(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include,
                                         int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                         const stk_quantile_params* quantile, const stk_frame_weight* per_frame,
                                         const float* const* norm, int32_t step, int32_t coverage, stk_image_f32* out, int32_t* counts) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    // (as stk_quantile_stack_weighted: coverage = 1 puts no condition on the border mode or value)
    if ((st = check_border_mode(ctx, border_mode))) return st;
    if (coverage < 0 || coverage > 1) return fail(ctx, STK_INVALID_PARAMS, "weighted: coverage must be 0 or 1");
    if ((st = quantile_validate(ctx, quantile))) return st;
    NormCombine nc;
    nc.quantile = quantile; nc.counts = counts;
    return norm_stack(ctx, frames, M, include, is_affine, border_mode, border_value, alpha, nc, per_frame, norm, step, coverage, out);
}

stk_status stk_ecc_match_local_normalized(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                          const stk_local_norm_params* norm, const stk_quantile_params* quantile, const float* weights,
                                          stk_image_f32* out, float* den_out, int32_t* counts, float* const* norm_out,
                                          stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    NormCombine nc;
    nc.quantile = quantile; nc.den = den_out; nc.counts = counts;
    return norm_match_ecc(ctx, frames, params, scale_down_width, norm, nc, weights, out, norm_out, applied, stats);
}

stk_status stk_keypoint_match_local_normalized(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                               float scale_down_width, const stk_local_norm_params* norm,
                                               const stk_quantile_params* quantile, const float* weights, stk_image_f32* out,
                                               int32_t* dropped, float* den_out, int32_t* counts, float* const* norm_out,
                                               stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    NormCombine nc;
    nc.quantile = quantile; nc.den = den_out; nc.counts = counts;
    return norm_match_keypoint(ctx, frames, params, scale_down_width, norm, nc, weights, out, dropped, norm_out, applied, stats);
}

stk_status stk_clip_stack_local_norm(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                                     int32_t border_mode, const double* border_value, double alpha, const stk_clip_params* clip,
                                     const stk_frame_weight* per_frame, const float* const* norm, int32_t step, int32_t coverage,
                                     stk_image_f32* out, int32_t* counts, float* kept_weight) {
    stk_status st = norm_clip_stack_check(ctx, frames, border_mode, coverage);
    if (st) return st;
    if ((st = clip_validate(ctx, clip))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    NormCombine nc;
    nc.clip = clip; nc.counts = counts; nc.kept = kept_weight;
    return norm_stack(ctx, frames, M, include, is_affine, border_mode, border_value, alpha, nc, per_frame, norm, step, coverage, out);
}

stk_status stk_robust_clip_stack_local_norm(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include,
                                            int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                            const stk_robust_clip_params* clip, const stk_frame_weight* per_frame,
                                            const float* const* norm, int32_t step, int32_t coverage, stk_image_f32* out,
                                            int32_t* counts, float* kept_weight) {
    stk_status st = norm_clip_stack_check(ctx, frames, border_mode, coverage);
    if (st) return st;
    if ((st = robust_clip_validate(ctx, clip))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    NormCombine nc;
    nc.mad = clip; nc.counts = counts; nc.kept = kept_weight;
    return norm_stack(ctx, frames, M, include, is_affine, border_mode, border_value, alpha, nc, per_frame, norm, step, coverage, out);
}

stk_status stk_ecc_match_local_normalized_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                                  float scale_down_width, const stk_local_norm_params* norm, const stk_clip_params* clip,
                                                  const stk_robust_clip_params* robust, const float* weights, stk_image_f32* out,
                                                  int32_t* counts, float* kept_weight, float* const* norm_out,
                                                  stk_frame_weight* applied, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    NormCombine nc;
    if (stk_status st = norm_clip_choice(ctx, clip, robust, counts, kept_weight, &nc)) return st;
    return norm_match_ecc(ctx, frames, params, scale_down_width, norm, nc, weights, out, norm_out, applied, stats);
}

stk_status stk_keypoint_match_local_normalized_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                                       float scale_down_width, const stk_local_norm_params* norm,
                                                       const stk_clip_params* clip, const stk_robust_clip_params* robust,
                                                       const float* weights, stk_image_f32* out, int32_t* dropped, int32_t* counts,
                                                       float* kept_weight, float* const* norm_out, stk_frame_weight* applied,
                                                       stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    NormCombine nc;
    if (stk_status st = norm_clip_choice(ctx, clip, robust, counts, kept_weight, &nc)) return st;
    return norm_match_keypoint(ctx, frames, params, scale_down_width, norm, nc, weights, out, dropped, norm_out, applied, stats);
}

}  // extern "C"
