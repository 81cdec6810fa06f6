// reject.cpp — blot-and-compare rejection maps for drizzle: stk_reject_maps, and the pass itself (reject_run) for the
// whole-stack forms in drizzle.cpp (an extension beyond the reference; definition in include/stacker.h, stk_reject_params;
// kernel in kernels_reject.hip). ctx->reject (grow-only like the other workspaces) holds, in this order: the entry table,
// the two counters per entry, then whatever planes the caller of reject_layout asks for: in stk_reject_maps the staging
// copies of a host caller's clean image, counts and planes, or the copies of a device caller's in-place planes; in the
// whole-stack forms the clean image, its counts and the maps.
#include <cmath>
#include <cstring>

#include "context.h"
#include "reject.h"

using namespace stk;

stk_status reject_validate(stk_ctx* ctx, const stk_reject_params* p) {
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null reject parameters");
    if (ctx->opt_subpixel_bits != 0)
        return fail(ctx, STK_INVALID_PARAMS, "reject maps need warp_subpixel_bits = 0: the blot is defined on exact coordinates only");
    if (!std::isfinite(p->snr1) || !std::isfinite(p->snr2) || !(p->snr1 > 0.0f) || !(p->snr2 > 0.0f))
        return fail(ctx, STK_INVALID_PARAMS, "reject maps: snr1 and snr2 must be finite and > 0");
    if (!std::isfinite(p->scale1) || !std::isfinite(p->scale2) || p->scale1 < 0.0f || p->scale2 < 0.0f)
        return fail(ctx, STK_INVALID_PARAMS, "reject maps: scale1 and scale2 must be finite and >= 0");
    if (!std::isfinite(p->read_noise) || p->read_noise < 0.0f) return fail(ctx, STK_INVALID_PARAMS, "reject maps: read_noise must be finite and >= 0");
    if (!std::isfinite(p->poisson_gain) || p->poisson_gain < 0.0f)
        return fail(ctx, STK_INVALID_PARAMS, "reject maps: poisson_gain must be finite and >= 0");
    if (p->min_count < 0) return fail(ctx, STK_INVALID_PARAMS, "reject maps: min_count must be >= 0");
    if (p->reserved != 0) return fail(ctx, STK_INVALID_PARAMS, "reject parameters: reserved must be 0");
    return STK_OK;
}

// The pass over the table's entries, `dev[table.frame[k]]` under the FORWARD matrices table.M[k], with the records `coef`
// (per entry). clean, counts (or null), in[k] (or null; never out[k]) and out[k] are device memory; ctx->reject is reserved
// for L. Writes the planes, synchronises, leaves the counters per entry in rejected / judged (or null) and adds the launch's
// device time to *ms.
stk_status reject_run(stk_ctx* ctx, const RejectLayout& L, const stk_frames* frames, const std::vector<const void*>& dev,
                      const EntryTable& table, int is_affine, double alpha, const std::vector<stk_frame_weight>& coef, const float* clean,
                      const int32_t* counts, const stk_reject_params* p, const std::vector<const float*>& in,
                      const std::vector<float*>& out, int64_t* rejected, int64_t* judged, double* ms) {
    const int ne = table.size();
    char* base = ctx->reject.as<char>();
    std::vector<RejectEntry> tab(ne);
    for (int k = 0; k < ne; k++) {
        RejectEntry& e = tab[k];
        std::memset(&e, 0, sizeof(e));
        e.f.src = dev[table.frame[k]];
        for (int j = 0; j < 9; j++) { e.f.Md[j] = table.M[k][j]; e.f.M[j] = (float)table.M[k][j]; }
        for (int c = 0; c < 4; c++) { e.gain[c] = coef[k].gain[c]; e.offset[c] = coef[k].offset[c]; }
        e.map_in = in[k];
        e.map_out = out[k];
    }
    unsigned long long* tallies = (unsigned long long*)(base + L.tallies);
    HIP_TRY(hipMemcpyAsync(base + L.entries, tab.data(), tab.size() * sizeof(RejectEntry), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(tallies, 0, (size_t)ne * 2 * sizeof(unsigned long long), ctx->stream));
    RejectArgs a{};
    a.entries = (const RejectEntry*)(base + L.entries);
    a.n_entries = ne;
    a.sw = frames->width; a.sh = frames->height; a.cn = frames->channels;
    a.src_stride = frame_row_bytes(frames) / (frames->depth / 8);
    a.alpha = (float)alpha;
    a.is_affine = is_affine;
    a.clean = clean;
    a.counts = counts;
    a.min_count = p->min_count;
    a.snr1 = p->snr1; a.snr2 = p->snr2; a.scale1 = p->scale1; a.scale2 = p->scale2;
    a.rn2 = p->read_noise * p->read_noise; a.pg = p->poisson_gain;
    a.tallies = tallies;
    std::vector<unsigned long long> host((size_t)ne * 2);
    const CombineOutputs o(host.data(), tallies, host.size(), sizeof(unsigned long long));
    stk_status st = combine_begin(ctx);
    if (st) return st;
    HIP_TRY(launch_reject(a, frames->depth, ctx->stream));
    if ((st = combine_end(ctx, ms, &o))) return st;     // (synchronises: the host tables leave scope)
    for (int k = 0; k < ne; k++) {
        if (rejected) rejected[k] = (int64_t)host[2 * (size_t)k];
        if (judged) judged[k] = (int64_t)host[2 * (size_t)k + 1];
    }
    return STK_OK;
}

extern "C" {

stk_status stk_reject_maps(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                           double alpha, const stk_frame_weight* per_frame, const float* clean, const int32_t* clean_counts,
                           const stk_reject_params* reject, const float* const* maps_in, float* const* maps_out,
                           int64_t* rejected, int64_t* judged) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = check_frames(ctx, frames, false, false);        // warp_interpolation is ignored: the option pair is not asked
    if (st) return st;
    if ((st = reject_validate(ctx, reject))) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (!clean) return fail(ctx, STK_INVALID_PARAMS, "null clean image");
    if (!maps_out) return fail(ctx, STK_INVALID_PARAMS, "null output maps");
    const int n = frames->n, sw = frames->width, sh = frames->height, cn = frames->channels;
    const bool host = frames->location != STK_DEVICE;
    EntryTable table;
    entries_from_include(n, M, include, table);
    const std::vector<int>& entry_frame = table.frame;
    size_t n_in = 0, n_alias = 0;
    for (int i : entry_frame) {
        if (!maps_out[i]) return fail(ctx, STK_INVALID_PARAMS, "reject maps: an included frame has no output plane");
        if (maps_in && maps_in[i]) { n_in++; if (maps_in[i] == maps_out[i]) n_alias++; }
    }
    if (entry_frame.empty()) return fail(ctx, STK_INVALID_PARAMS, "reject maps: no frame included");
    std::vector<stk_frame_weight> coef;
    gather_records(table, per_frame, coef);
    if ((st = weighted_check_coefs(ctx, coef, cn))) return st;
    const int ne = table.size();
    (void)hipSetDevice(ctx->device);
    timing_begin(ctx);
    // host: the clean image, the counts, the input planes and the output planes are staged; device: the in-place planes
    const RejectLayout L = reject_layout(ne, sw, sh, cn, host, host && clean_counts, host ? n_in + (size_t)ne : n_alias);
    if ((st = workspace_reserve(ctx, ctx->reject, L.total, "reject maps"))) return st;
    std::vector<const void*> dev;
    if ((st = resolve_frames(ctx, frames, dev))) return st;
    char* base = ctx->reject.as<char>();
    const size_t plane_bytes = (size_t)sw * sh * sizeof(float);
    const float* dclean = clean;
    const int32_t* dcounts = clean_counts;
    if (host) {
        HIP_TRY(hipMemcpyAsync(base + L.clean, clean, plane_bytes * cn, hipMemcpyHostToDevice, ctx->stream));
        dclean = (const float*)(base + L.clean);
        if (clean_counts) {
            HIP_TRY(hipMemcpyAsync(base + L.counts, clean_counts, (size_t)sw * sh * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
            dcounts = (const int32_t*)(base + L.counts);
        }
    }
    std::vector<const float*> in(ne, nullptr);
    std::vector<float*> out(ne, nullptr);
    size_t slot = 0;
    for (int k = 0; k < ne; k++) {
        const int i = entry_frame[k];
        const float* mi = maps_in ? maps_in[i] : nullptr;
        out[k] = host ? (float*)(base + L.planes + slot++ * L.plane) : maps_out[i];
        if (mi && (host || mi == maps_out[i])) {
            float* d = (float*)(base + L.planes + slot++ * L.plane);
            HIP_TRY(hipMemcpyAsync(d, mi, plane_bytes, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
            mi = d;
        }
        in[k] = mi;
    }
    std::vector<int64_t> rej(ne), jud(ne);
    double ms = 0.0;
    if ((st = reject_run(ctx, L, frames, dev, table, is_affine != 0, alpha, coef, dclean, dcounts, reject, in, out, rej.data(),
                         jud.data(), &ms)))
        return st;
    if (host) {
        for (int k = 0; k < ne; k++)
            HIP_TRY(hipMemcpyAsync(maps_out[entry_frame[k]], out[k], plane_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (rejected) std::memset(rejected, 0, (size_t)n * sizeof(int64_t));
    if (judged) std::memset(judged, 0, (size_t)n * sizeof(int64_t));
    for (int k = 0; k < ne; k++) {
        if (rejected) rejected[entry_frame[k]] = rej[k];
        if (judged) judged[entry_frame[k]] = jud[k];
    }
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

}  // extern "C"
