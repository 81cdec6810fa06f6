// star.cpp — star registration: stk_star_detect, stk_star_align, stk_star_match (an extension beyond the reference;
// definition in include/stacker.h, stk_star_params; kernel in kernels_star.hip, the host matching in star_match.cpp).
// ctx->local (StarLayout, workspace.h) holds the frame pointer table and, per (frame, tile), the peak count and the
// record slots; one copy of the counts and one of the records bring a stack's detection back. The triangle and vote steps
// of the frames run on the context's host pool (frame 0's triangles are built once); the fits are findHomography's
// batched device path (homography.h), unchanged, one batch per stack as in keypoint.cpp; the fold is the plain one over the
// table of frame 0 and the kept frames.
// The *_deep calls (include/stacker.h, stk_star_deep_params; kernel in kernels_star_deep.hip) are the same code with another
// launch (StarMode) and the fold at the frames' own depth under the caller's alpha.
// Star measurement (include/stacker.h, stk_star_measure_params; kernel in kernels_star_measure.hip, the host half in
// star_shape_host.h): ctx->local (StarMeasureLayout) holds the frame pointer table, the (px, py) pairs of the stars whose
// aperture lies inside the frame, their count per frame and the record slots; one copy brings a stack's records back.
// stk_star_match_quality_weighted runs the alignment, measures the stars that detection found on the frames still resident
// in HBM, and folds once with the quality weights.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>

#include "context.h"
#include "host_pool.h"
#include "star_match.h"
#include "star_shape_host.h"

using namespace stk;

namespace {

// run fn(i) for i in [0, n) on the context's host pool (pure host work), as keypoint.cpp does
void star_parallel_for(stk_ctx* ctx, int n, const std::function<void(int)>& fn) {
    const int threads = ctx->opt_kp_workers;
    if (threads <= 1 || n <= 1) { for (int i = 0; i < n; i++) fn(i); return; }
    if (ctx->shared_pool) { ctx->shared_pool->run(n, fn); return; }
    if (!ctx->host_pool || ctx->host_pool->size() != threads - 1) {
        host_pool_destroy(ctx->host_pool);
        ctx->host_pool = new HostPool(threads - 1);          // the caller is the remaining thread
    }
    ctx->host_pool->run(n, fn);
}

// which detection launch a call uses: the 8-bit kernel (stk_star_*), or the key kernel (stk_star_*_deep) with its scale
struct StarMode { bool deep; float f32_scale; };

stk_status star_check(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, bool stack_form, bool folds,
                      const StarMode& mode = StarMode{false, 1.0f}) {
    stk_status st = check_frames(ctx, frames, stack_form, folds);
    if (st) return st;
    bool ni = false;
    stk_star_params q;
    const stk_star_params* checked = params;
    if (mode.deep && params && params->min_contrast > 255 && params->min_contrast <= 65535) {   // key units: 1 .. 65535
        q = *params; q.min_contrast = 255; checked = &q;
    }
    if (const char* msg = star::validate(checked, &ni)) return fail(ctx, ni ? STK_NOT_IMPLEMENTED : STK_INVALID_PARAMS, msg);
    if (folds && (params->border_mode < 0 || params->border_mode > 4))
        return fail(ctx, params->border_mode == STK_BORDER_TRANSPARENT ? STK_NOT_IMPLEMENTED : STK_INVALID_PARAMS, "unsupported border mode");
    if (!mode.deep && frames->depth != 8)
        return fail(ctx, STK_NOT_IMPLEMENTED, "star detection takes 8-bit frames: the statistics and moments are defined on the 8-bit integer grey");
    if (stack_form && frames->n < 2) return fail(ctx, STK_NOT_ENOUGH_FILES, "star registration needs a reference frame and at least one moving frame");
    return STK_OK;
}

// the deep calls' own argument: checked before anything else of the call
stk_status star_deep_mode(stk_ctx* ctx, const stk_frames* frames, const stk_star_deep_params* deep, StarMode& mode) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!deep) return fail(ctx, STK_INVALID_PARAMS, "null star deep parameters");
    if (deep->reserved != 0) return fail(ctx, STK_INVALID_PARAMS, "star deep: reserved must be 0");
    mode = StarMode{true, 1.0f};
    if (frames && frames->depth == 32) {
        if (!std::isfinite(deep->f32_scale) || !(deep->f32_scale > 0.0f)) return fail(ctx, STK_INVALID_PARAMS, "star deep: f32_scale must be finite and > 0");
        mode.f32_scale = deep->f32_scale;
    }
    return STK_OK;
}

bool star_before(const StarRecord& a, const StarRecord& b) {
    if (a.S != b.S) return a.S > b.S;
    if (a.py != b.py) return a.py < b.py;
    return a.px < b.px;
}

// Detection of the whole stack: dev = the frames in HBM by frame index, lists[i] = frame i's stars (at most max_stars,
// brightest first), n_peaks[i] = its peaks before any truncation. prep_ms of the timing: the launches' device time.
stk_status star_detect_impl(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* p, const StarMode& mode,
                            std::vector<const void*>& dev, std::vector<std::vector<stk_star>>& lists, std::vector<int32_t>& n_peaks) {
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const size_t rb = frame_row_bytes(frames), tiles = (size_t)star_tiles(w, h);
    stk_status st = resolve_frames(ctx, frames, dev);
    if (st) return st;
    const StarLayout L = star_layout((size_t)n, tiles);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "star"))) return st;
    char* base = ctx->local.as<char>();
    const float ks = (float)((double)p->kappa * 1.4826);
    HIP_TRY(hipMemcpyAsync(base + L.fptrs, dev.data(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    for (int f0 = 0; f0 < n; f0 += 65535) {
        const int nl = std::min(65535, n - f0);
        const void* const* fp = (const void* const*)(base + L.fptrs) + f0;
        int32_t* cnt = (int32_t*)(base + L.counts) + (size_t)f0 * tiles;
        StarRecord* rec = (StarRecord*)(base + L.records) + (size_t)f0 * tiles * STAR_TILE_CAP;
        if (mode.deep)
            HIP_TRY(launch_star_detect_deep(fp, nl, frames->depth, cn, w, h, rb, p->radius, ks, p->min_contrast, p->min_pixels, mode.f32_scale,
                                            cnt, rec, ctx->stream));
        else
            HIP_TRY(launch_star_detect(fp, nl, cn, w, h, rb, p->radius, ks, p->min_contrast, p->min_pixels, cnt, rec, ctx->stream));
    }
    HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
    std::vector<int32_t> counts((size_t)n * tiles);
    std::vector<StarRecord> records((size_t)n * tiles * STAR_TILE_CAP);
    HIP_TRY(hipMemcpyAsync(counts.data(), base + L.counts, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(records.data(), base + L.records, records.size() * sizeof(StarRecord), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.prep_ms += ev_ms(ctx->ev[0], ctx->ev[1]);
    lists.assign(n, {});
    n_peaks.assign(n, 0);
    star_parallel_for(ctx, n, [&](int i) {
        std::vector<StarRecord> all;
        int64_t total = 0;
        for (size_t t = 0; t < tiles; t++) {
            const int c = counts[(size_t)i * tiles + t];
            total += c;
            const StarRecord* r = &records[((size_t)i * tiles + t) * STAR_TILE_CAP];
            all.insert(all.end(), r, r + std::min(c, STAR_TILE_CAP));
        }
        n_peaks[i] = (int32_t)std::min<int64_t>(total, INT32_MAX);
        std::sort(all.begin(), all.end(), star_before);
        if ((int)all.size() > p->max_stars) all.resize(p->max_stars);
        std::vector<stk_star>& o = lists[i];
        o.resize(all.size());
        for (size_t k = 0; k < all.size(); k++) {
            const StarRecord& r = all[k];
            o[k].x = (float)((double)r.px + (double)r.Sx / (double)r.S);
            o[k].y = (float)((double)r.py + (double)r.Sy / (double)r.S);
            o[k].flux = (float)r.S;
            o[k].px = r.px; o[k].py = r.py; o[k].peak = r.peak; o[k].npix = r.npix; o[k].reserved = 0;
        }
    });
    return STK_OK;
}

// one batched fit over the frames that have at least 4 pairs (pairs[i]: moving index, reference index); outc by frame
stk_status star_fit(stk_ctx* ctx, const stk_star_params* p, const std::vector<std::vector<stk_star>>& lists,
                    const std::vector<std::vector<int32_t>>& pairs, std::vector<geom::HgOutcome>& outc, std::vector<char>& ran) {
    const int n = (int)lists.size();
    outc.assign(n, geom::HgOutcome{});
    ran.assign(n, 0);
    std::vector<std::vector<float>> from(n), to(n);
    std::vector<geom::HgProblem> probs;
    std::vector<int> owner;
    for (int i = 1; i < n; i++) {
        const size_t np = pairs[i].size() / 2;
        if (np < 4) continue;
        from[i].resize(np * 2); to[i].resize(np * 2);
        for (size_t k = 0; k < np; k++) {
            const stk_star& m = lists[i][pairs[i][2 * k]];
            const stk_star& r = lists[0][pairs[i][2 * k + 1]];
            from[i][2 * k] = m.x; from[i][2 * k + 1] = m.y;
            to[i][2 * k] = r.x; to[i][2 * k + 1] = r.y;
        }
        probs.push_back({from[i].data(), to[i].data(), (int)np, nullptr});
        owner.push_back(i);
    }
    if (probs.empty()) return STK_OK;
    std::vector<geom::HgOutcome> got(probs.size());
    const int hst = geom::find_homography_batch(ctx, ctx->stream, ctx->hg, probs.data(), (int)probs.size(), p->method,
                                                p->ransac_reproj_threshold, got.data());
    if (hst) return (stk_status)hst;
    for (size_t k = 0; k < probs.size(); k++) { outc[owner[k]] = got[k]; ran[owner[k]] = 1; }
    return STK_OK;
}

// detection and steps 1 - 6: the stats of all n frames, the frames in HBM, the number of moving frames dropped. Every
// moving frame dropped: STK_INVALID_PARAMS behind the filled stats.
stk_status star_align_impl(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* p, const StarMode& mode, stk_frame_stats* stats,
                           std::vector<const void*>& dev, int32_t* dropped, std::vector<std::vector<stk_star>>* lists_out = nullptr) {
    const int n = frames->n;
    std::vector<std::vector<stk_star>> own_lists;
    std::vector<std::vector<stk_star>>& lists = lists_out ? *lists_out : own_lists;
    std::vector<int32_t> n_peaks;
    stk_status st = star_detect_impl(ctx, frames, p, mode, dev, lists, n_peaks);
    if (st) return st;
    HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
    std::memset(stats, 0, sizeof(stk_frame_stats) * (size_t)n);
    for (int i = 0; i < n; i++) {
        stats[i].n_keypoints = (int32_t)lists[i].size();
        stats[i].status = i == 0 ? 0 : 1;
        stats[i].warp[0] = stats[i].warp[4] = stats[i].warp[8] = 1;
    }
    const int m = p->match_stars, n0 = (int)lists[0].size();
    std::vector<std::vector<int32_t>> pairs(n);
    if (n0 >= p->min_stars) {
        std::vector<star::Triangle> tri0;
        star::triangles(lists[0].data(), n0, m, p->neighbours, tri0);
        star_parallel_for(ctx, n - 1, [&](int k) {
            const int i = k + 1, ni = (int)lists[i].size();
            if (ni < p->min_stars) return;
            std::vector<star::Triangle> tri;
            star::triangles(lists[i].data(), ni, m, p->neighbours, tri);
            star::vote_pairs(tri, std::min(m, ni), tri0, std::min(m, n0), p->tri_tolerance, p->min_votes, pairs[i]);
        });
    }
    std::vector<geom::HgOutcome> fit, fit2;
    std::vector<char> ran, ran2;
    if ((st = star_fit(ctx, p, lists, pairs, fit, ran))) return st;
    std::vector<int32_t> n_matches(n, 0);
    for (int i = 1; i < n; i++) n_matches[i] = (int32_t)(pairs[i].size() / 2);
    if (p->refine) {
        std::vector<std::vector<int32_t>> guided(n);
        star_parallel_for(ctx, n - 1, [&](int k) {
            const int i = k + 1;
            if (!ran[i] || fit[i].rc != 0 || !fit[i].found) return;
            star::guided_pairs(lists[i].data(), (int)lists[i].size(), lists[0].data(), n0, fit[i].H, p->ransac_reproj_threshold, guided[i]);
        });
        if ((st = star_fit(ctx, p, lists, guided, fit2, ran2))) return st;
        for (int i = 1; i < n; i++) {
            if (!ran2[i]) continue;
            n_matches[i] = (int32_t)(guided[i].size() / 2);
            if (fit2[i].rc == 0 && fit2[i].found && fit2[i].n_inliers >= fit[i].n_inliers) fit[i] = fit2[i];
        }
    }
    int nd = 0;
    for (int i = 1; i < n; i++) {
        stats[i].n_matches = n_matches[i];
        const bool ok = ran[i] && fit[i].rc == 0 && fit[i].found && fit[i].n_inliers >= p->min_inliers;
        if (!ok) { nd++; continue; }
        stats[i].status = 0;
        stats[i].n_inliers = fit[i].n_inliers;
        for (int k = 0; k < 9; k++) stats[i].warp[k] = fit[i].H[k];
    }
    HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.align_ms += ev_ms(ctx->ev[2], ctx->ev[3]);
    if (dropped) *dropped = nd;
    if (nd == n - 1)
        return fail(ctx, STK_INVALID_PARAMS, "All images discarded: no moving frame could be registered against the reference's stars");
    return STK_OK;
}

// stk_star_detect / stk_star_detect_deep behind their checks
stk_status star_detect_call(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, const StarMode& mode, stk_star* stars,
                            int32_t* n_stars, int32_t* n_peaks) {
    stk_status st = star_check(ctx, frames, params, false, false, mode);
    if (st) return st;
    if (!stars || !n_stars) return fail(ctx, STK_INVALID_PARAMS, "null star outputs");
    timing_begin(ctx);
    std::vector<const void*> dev;
    std::vector<std::vector<stk_star>> lists;
    std::vector<int32_t> peaks;
    if ((st = star_detect_impl(ctx, frames, params, mode, dev, lists, peaks))) return st;
    std::memset(stars, 0, sizeof(stk_star) * (size_t)frames->n * (size_t)params->max_stars);
    for (int i = 0; i < frames->n; i++) {
        n_stars[i] = (int32_t)lists[i].size();
        if (n_peaks) n_peaks[i] = peaks[i];
        if (!lists[i].empty()) std::memcpy(stars + (size_t)i * params->max_stars, lists[i].data(), sizeof(stk_star) * lists[i].size());
    }
    return STK_OK;
}

stk_status star_align_call(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, const StarMode& mode, int32_t* dropped,
                           stk_frame_stats* stats) {
    stk_status st = star_check(ctx, frames, params, true, false, mode);
    if (st) return st;
    if (!stats) return fail(ctx, STK_INVALID_PARAMS, "null stats");
    timing_begin(ctx);
    std::vector<const void*> dev;
    return star_align_impl(ctx, frames, params, mode, stats, dev, dropped);
}

// the alignment, then the plain mean with the fold of fold_spec_keypoint's shape: the given depth and alpha, the params'
// border, never affine
stk_status star_match_call(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, const StarMode& mode, int depth, double alpha,
                           stk_image_f32* out, int32_t* dropped, stk_frame_stats* stats) {
    stk_status st = star_check(ctx, frames, params, true, true, mode);
    if (st) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    timing_begin(ctx);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    std::vector<const void*> dev;
    int32_t nd = 0;
    if ((st = star_align_impl(ctx, frames, params, mode, stats, dev, &nd))) { if (dropped) *dropped = nd; return st; }
    if (dropped) *dropped = nd;
    const size_t nel = (size_t)w * h * cn;
    stk_image_f32 sum = *out;
    if (out->location != STK_DEVICE) {
        if ((st = workspace_reserve(ctx, ctx->acc, nel * sizeof(float), "star sum"))) return st;
        sum.data = ctx->acc.as<float>(); sum.location = STK_DEVICE;
    }
    EntryTable table;
    entries_from_stats(n, stats, true, table);
    if ((st = entry_table_upload(ctx, frames, dev, table, 0))) return st;
    HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    if ((st = warp_fold_enqueue(ctx, table.size(), depth, w, h, cn, frame_row_bytes(frames), alpha, params->border_mode,
                                params->border_value, 0, sum.data, image_stride_floats(&sum), 0)))
        return st;
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const float warp_ms = ev_ms(ctx->ev[4], ctx->ev[5]);
    const stk_timing keep = ctx->timing;
    st = stk_finalize_mean(ctx, &sum, n - nd, out);
    const double fin = ctx->timing.finalize_ms;
    ctx->timing = keep; ctx->timing.warp_ms = warp_ms; ctx->timing.finalize_ms = fin;
    return st;
}

const StarMode kStarU8{false, 1.0f};

// The shapes of the stars `stars` (n x max_stars, n_stars[i] in use) on the frames `dev` (in HBM, by frame index): n x
// max_stars shapes, zeroed behind n_stars[i], the derived values filled. A star whose aperture is not inside the frame is
// flagged here and never reaches the device list. Synchronises; adds the launches' device time to prep_ms.
stk_status star_measure_impl(stk_ctx* ctx, const stk_frames* frames, const std::vector<const void*>& dev, float f32_scale,
                             const stk_star_measure_params* mp, const stk_star* stars, const int32_t* n_stars, int max_stars,
                             stk_star_shape* shapes) {
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, R = mp->radius;
    const StarMeasureLayout L = star_measure_layout((size_t)n, (size_t)max_stars);
    stk_status st = workspace_reserve(ctx, ctx->local, L.total, "star measure");
    if (st) return st;
    char* base = ctx->local.as<char>();
    std::vector<int32_t> pairs((size_t)n * max_stars * 2, 0), counts((size_t)n, 0), slot_of((size_t)n * max_stars, 0);
    std::memset(shapes, 0, sizeof(stk_star_shape) * (size_t)n * max_stars);
    for (int i = 0; i < n; i++) {
        int c = 0;
        for (int k = 0; k < n_stars[i]; k++) {
            const size_t at = (size_t)i * max_stars + k;
            stk_star_shape& o = shapes[at];
            const int px = stars[at].px, py = stars[at].py;
            o.px = px; o.py = py;
            if (px < R || py < R || px > w - 1 - R || py > h - 1 - R) { o.flags = 1; continue; }
            const size_t d = (size_t)i * max_stars + c;
            pairs[2 * d] = px; pairs[2 * d + 1] = py; slot_of[d] = k;
            c++;
        }
        counts[i] = c;
    }
    const float ks = (float)((double)mp->kappa * 1.4826);
    HIP_TRY(hipMemcpyAsync(base + L.fptrs, dev.data(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(base + L.stars, pairs.data(), pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(base + L.counts, counts.data(), counts.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    for (int f0 = 0; f0 < n; f0 += 65535) {
        const int nl = std::min(65535, n - f0);
        StarMeasureArgs a{};
        a.frames = (const void* const*)(base + L.fptrs) + f0;
        a.stars = (const int32_t*)(base + L.stars) + (size_t)f0 * max_stars * 2;
        a.counts = (const int32_t*)(base + L.counts) + f0;
        a.records = (StarMeasureRecord*)(base + L.records) + (size_t)f0 * max_stars;
        a.w = w; a.h = h; a.stride = frame_row_bytes(frames); a.max_stars = max_stars;
        a.radius = R; a.ring_inner = mp->ring_inner; a.ring_outer = mp->ring_outer;
        a.ks = ks; a.min_contrast = mp->min_contrast; a.min_pixels = mp->min_pixels; a.saturation = mp->saturation;
        HIP_TRY(launch_star_measure(a, nl, frames->depth, frames->channels, f32_scale, ctx->stream));
    }
    HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
    std::vector<StarMeasureRecord> rec((size_t)n * max_stars);
    HIP_TRY(hipMemcpyAsync(rec.data(), base + L.records, rec.size() * sizeof(StarMeasureRecord), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.prep_ms += ev_ms(ctx->ev[0], ctx->ev[1]);
    for (int i = 0; i < n; i++)
        for (int c = 0; c < counts[i]; c++) {                             // (slots from counts[i] on were not written: not read)
            const size_t d = (size_t)i * max_stars + c;
            const StarMeasureRecord& r = rec[d];
            stk_star_shape& o = shapes[(size_t)i * max_stars + slot_of[d]];
            o.S = r.S; o.Sx = r.Sx; o.Sy = r.Sy; o.Sxx = r.Sxx; o.Syy = r.Syy; o.Sxy = r.Sxy;
            o.bg = r.bg; o.mad = r.mad; o.thr = r.thr; o.npix = r.npix; o.peak = r.peak; o.n_ring = r.n_ring; o.flags = r.flags;
        }
    shape::derive(shapes, n * max_stars);
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_star_detect(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, stk_star* stars, int32_t* n_stars,
                           int32_t* n_peaks) {
    return star_detect_call(ctx, frames, params, kStarU8, stars, n_stars, n_peaks);
}

stk_status stk_star_align(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, int32_t* dropped,
                          stk_frame_stats* stats) {
    return star_align_call(ctx, frames, params, kStarU8, dropped, stats);
}

stk_status stk_star_match(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, stk_image_f32* out, int32_t* dropped,
                          stk_frame_stats* stats) {
    return star_match_call(ctx, frames, params, kStarU8, 8, 1.0 / 255.0, out, dropped, stats);
}

stk_status stk_star_detect_deep(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, const stk_star_deep_params* deep,
                                stk_star* stars, int32_t* n_stars, int32_t* n_peaks) {
    StarMode mode{};
    if (const stk_status st = star_deep_mode(ctx, frames, deep, mode)) return st;
    return star_detect_call(ctx, frames, params, mode, stars, n_stars, n_peaks);
}

stk_status stk_star_align_deep(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, const stk_star_deep_params* deep,
                               int32_t* dropped, stk_frame_stats* stats) {
    StarMode mode{};
    if (const stk_status st = star_deep_mode(ctx, frames, deep, mode)) return st;
    return star_align_call(ctx, frames, params, mode, dropped, stats);
}

stk_status stk_star_match_deep(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, const stk_star_deep_params* deep,
                               double alpha, stk_image_f32* out, int32_t* dropped, stk_frame_stats* stats) {
    StarMode mode{};
    if (const stk_status st = star_deep_mode(ctx, frames, deep, mode)) return st;
    if (!std::isfinite(alpha)) return fail(ctx, STK_INVALID_PARAMS, "star match: alpha must be finite");
    return star_match_call(ctx, frames, params, mode, frames ? frames->depth : 8, alpha, out, dropped, stats);
}

stk_status stk_star_shape_derive(stk_star_shape* shapes, int32_t count) { return shape::derive(shapes, count); }

stk_status stk_star_frame_quality(const stk_star_shape* shapes, const int32_t* n_stars, int32_t n, int32_t max_stars, stk_star_quality* out) {
    return shape::frame_quality(shapes, n_stars, n, max_stars, out);
}

stk_status stk_star_quality_scores(const stk_star_quality* quality, int32_t n, double* scores) {
    return shape::quality_scores(quality, n, scores);
}

stk_status stk_star_quality_weights(const stk_star_quality* quality, int32_t n, const stk_star_quality_params* params, int32_t reference,
                                    const int32_t* include_or_null, const float* weights_or_null, float* weights_out,
                                    int32_t* include_out_or_null, int32_t* rejected_or_null) {
    return shape::quality_weights(quality, n, params, reference, include_or_null, weights_or_null, weights_out, include_out_or_null,
                                  rejected_or_null);
}

stk_status stk_star_measure(stk_ctx* ctx, const stk_frames* frames, const stk_star_deep_params* deep, const stk_star_measure_params* params,
                            const stk_star* stars, const int32_t* n_stars, int32_t max_stars, stk_star_shape* shapes) {
    StarMode mode{};
    if (const stk_status st = star_deep_mode(ctx, frames, deep, mode)) return st;
    stk_status st = check_frames(ctx, frames, false, false);
    if (st) return st;
    if (const char* msg = shape::validate(params)) return fail(ctx, STK_INVALID_PARAMS, msg);
    if (!stars || !n_stars || !shapes) return fail(ctx, STK_INVALID_PARAMS, "null star lists or shapes");
    if (max_stars < 1 || max_stars > 4096) return fail(ctx, STK_INVALID_PARAMS, "star measure: max_stars must be 1 .. 4096");
    for (int i = 0; i < frames->n; i++)
        if (n_stars[i] < 0 || n_stars[i] > max_stars) return fail(ctx, STK_INVALID_PARAMS, "star measure: n_stars must be 0 .. max_stars");
    timing_begin(ctx);
    (void)hipSetDevice(ctx->device);
    std::vector<const void*> dev;
    if ((st = resolve_frames(ctx, frames, dev))) return st;
    return star_measure_impl(ctx, frames, dev, mode.f32_scale, params, stars, n_stars, max_stars, shapes);
}

stk_status stk_star_match_quality_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params,
                                           const stk_star_deep_params* deep, const stk_star_measure_params* measure,
                                           const stk_star_quality_params* quality, double alpha, int32_t coverage, const float* weights,
                                           stk_image_f32* out, float* coverage_out, int32_t* dropped, int32_t* rejected,
                                           stk_frame_weight* applied, stk_frame_stats* stats, stk_star_quality* quality_out) {
    StarMode mode{};
    if (const stk_status st = star_deep_mode(ctx, frames, deep, mode)) return st;
    if (!std::isfinite(alpha)) return fail(ctx, STK_INVALID_PARAMS, "star match: alpha must be finite");
    stk_status st = star_check(ctx, frames, params, true, true, mode);
    if (st) return st;
    if (const char* msg = shape::validate(measure)) return fail(ctx, STK_INVALID_PARAMS, msg);
    if (const char* msg = shape::validate(quality)) return fail(ctx, STK_INVALID_PARAMS, msg);
    if ((st = weighted_check_border(ctx, params->border_mode, params->border_value, coverage))) return st;
    if ((st = combine_check_out(ctx, out, frames))) return st;
    timing_begin(ctx);
    const int n = frames->n, ms_cap = params->max_stars;
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    std::vector<const void*> dev;
    std::vector<std::vector<stk_star>> lists;
    int32_t nd = 0;
    st = star_align_impl(ctx, frames, params, mode, stats, dev, &nd, &lists);
    if (dropped) *dropped = nd;
    if (st) return st;
    // the stars detection found, as stk_star_detect_deep lays them out; the frames are still resident
    std::vector<stk_star> stars((size_t)n * ms_cap);
    std::vector<int32_t> n_stars((size_t)n);
    std::memset(stars.data(), 0, sizeof(stk_star) * stars.size());
    for (int i = 0; i < n; i++) {
        n_stars[i] = (int32_t)lists[i].size();
        if (!lists[i].empty()) std::memcpy(&stars[(size_t)i * ms_cap], lists[i].data(), sizeof(stk_star) * lists[i].size());
    }
    std::vector<stk_star_shape> shapes((size_t)n * ms_cap);
    if ((st = star_measure_impl(ctx, frames, dev, mode.f32_scale, measure, stars.data(), n_stars.data(), ms_cap, shapes.data()))) return st;
    std::vector<stk_star_quality> own_q;
    if (!quality_out) { own_q.resize(n); quality_out = own_q.data(); }
    shape::frame_quality(shapes.data(), n_stars.data(), n, ms_cap, quality_out);
    std::vector<int32_t> include((size_t)n), pass((size_t)n);
    for (int i = 0; i < n; i++) include[i] = stats[i].status == 0;
    std::vector<float> wq((size_t)n);
    int32_t nr = 0;
    if ((st = shape::quality_weights(quality_out, n, quality, 0, include.data(), weights, wq.data(), pass.data(), &nr)))
        return fail(ctx, st, "star quality weights: the reference frame has no measured star, no frame passes, or a weight is not finite and >= 0");
    if (rejected) *rejected = nr;
    std::vector<stk_frame_weight> rec((size_t)n, unit_record());
    for (int i = 0; i < n; i++) rec[i].weight = wq[i];
    if (applied) std::memcpy(applied, rec.data(), sizeof(stk_frame_weight) * (size_t)n);
    std::vector<double> M((size_t)n * 9);
    for (int i = 0; i < n; i++) std::memcpy(&M[(size_t)i * 9], stats[i].warp, sizeof(double) * 9);
    EntryTable table;
    entries_from_include(n, M.data(), pass.data(), table);
    std::vector<stk_frame_weight> coef;
    gather_records(table, rec.data(), coef);
    if ((st = weighted_check_coefs(ctx, coef, frames->channels))) return st;
    if ((st = entry_table_upload(ctx, frames, dev, table, 0))) return st;
    double ms = 0.0;
    if ((st = weighted_fold_records(ctx, coef, fold_spec(frames, alpha, params->border_mode, params->border_value, 0), coverage, out,
                                    coverage_out, &ms)))
        return st;
    ctx->timing.finalize_ms = ms;
    return STK_OK;
}

}  // extern "C"
