// quality.cpp — score and rank a whole stack (include/stacker.h: stk_stack_sharpness, stk_rank_frames,
// stk_ecc_match_ranked, stk_keypoint_match_ranked): the first half of the reference's example program
// (examples/main.rs:35-64 — four sharpness metrics per file, sort by one of them, skip the worst, reverse) in front of
// the stacking calls. The metrics of all frames come from one device pass (kernels_quality.hip) and travel to the host
// in one copy behind one synchronisation; sorting and selecting are host code on n x 4 doubles.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <numeric>

#include "context.h"

using namespace stk;

// The closing formulas of the four metrics from a frame's sums: cv::mean / cv::meanStdDev multiply by the reciprocal of
// the pixel count (lib.rs:1030-1166). s: the sum of the filtered values, sq: the sum of their squares (LAPV, GLVN).
double sharpness_finish(int metric, double s, double sq, int width, int height) {
    const double scale = 1. / ((double)width * height);
    if (metric == STK_SHARPNESS_LAPM || metric == STK_SHARPNESS_TENG) return s * scale;
    const double mean = s * scale;
    const double sigma = std::sqrt(std::max(sq * scale - mean * mean, 0.));
    return metric == STK_SHARPNESS_LAPV ? sigma * sigma : (sigma * sigma) / std::max(mean, DBL_EPSILON);
}

namespace {

// TENG at ksize 7 adds up to 2 x (64 x 10 x 255)^2 = 5.33e10 per pixel: int64 (9.2e18) holds 1.7e8 such pixels
constexpr size_t QUALITY_MAX_PIXELS = (size_t)1 << 27;
constexpr size_t QUALITY_PARTIALS_BYTES = (size_t)256 << 20;   // tile partials of one launch (4K: 98 kB per frame)

bool ksize_ok(int k) { return k == 1 || k == 3 || k == 5 || k == 7; }

stk_status quality_check(stk_ctx* ctx, const stk_frames* f, int ksize) {
    if (f->depth != 8)
        return fail(ctx, STK_NOT_IMPLEMENTED,
                    "stack sharpness takes 8-bit frames: the reference scores 8-bit greys (examples/main.rs:40), and the exact "
                    "int64 sums of the pass do not hold 16-bit or float input");
    if (!ksize_ok(ksize)) return fail(ctx, STK_INVALID_PARAMS, "Kernel size must be 1, 3, 5, or 7");   // lib.rs:1105-1109
    if ((size_t)f->width * f->height > QUALITY_MAX_PIXELS)
        return fail(ctx, STK_NOT_IMPLEMENTED, "stack sharpness: frames above 2^27 pixels could overflow the int64 sums");
    return STK_OK;
}

// scores: n x 4 doubles in STK_SHARPNESS_* order. ms (optional): device time of the pass (host-fed stacks: with the copies)
stk_status quality_scores(stk_ctx* ctx, const stk_frames* f, int ksize, double* scores, double* ms) {
    (void)hipSetDevice(ctx->device);
    const int n = f->n, w = f->width, h = f->height, cn = f->channels;
    const size_t rb = frame_row_bytes(f), fb = rb * h;
    const size_t tiles = (size_t)quality_tiles(w, h);
    const bool host = f->location == STK_HOST;
    // host frames go through the frame workspace in batches that fit it (at least "upload_batch" frames)
    int batch = n;
    if (host) {
        const size_t budget = std::max<size_t>(ctx->frames.cap, (size_t)ctx->opt_upload_batch * fb);
        batch = (int)std::min<size_t>((size_t)n, std::max<size_t>(1, budget / fb));
        HIP_TRY(ctx->frames.reserve(fb * (size_t)batch));
    }
    const int per_launch = (int)std::min<size_t>({(size_t)batch, (size_t)65535, std::max<size_t>(1, QUALITY_PARTIALS_BYTES / (tiles * 48))});
    const size_t n_ptrs = host ? (size_t)batch : (size_t)n;
    const size_t off_records = (n_ptrs * sizeof(void*) + 15) & ~(size_t)15, off_partials = off_records + (size_t)n * 48;
    HIP_TRY(ctx->quality.reserve(off_partials + (size_t)per_launch * tiles * 48));
    const void** ptrs_dev = ctx->quality.as<const void*>();
    long long* records = reinterpret_cast<long long*>(ctx->quality.as<uint8_t>() + off_records);
    long long* partials = reinterpret_cast<long long*>(ctx->quality.as<uint8_t>() + off_partials);
    std::vector<const void*> ptrs(n_ptrs);                         // (outlives the copy: the call synchronises below)
    for (size_t i = 0; i < n_ptrs; i++) ptrs[i] = host ? (const void*)(ctx->frames.as<uint8_t>() + fb * i) : f->data[i];
    HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    HIP_TRY(hipMemcpyAsync(ptrs_dev, ptrs.data(), n_ptrs * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    for (int b0 = 0; b0 < n; b0 += batch) {
        const int nb = std::min(batch, n - b0);
        if (host)      // stream order keeps the previous batch's kernels ahead of the copies that overwrite its frames
            for (int i = 0; i < nb; i++)
                HIP_TRY(hipMemcpyAsync(ctx->frames.as<uint8_t>() + fb * (size_t)i, f->data[b0 + i], frame_copy_bytes(f), hipMemcpyHostToDevice, ctx->stream));
        for (int l0 = 0; l0 < nb; l0 += per_launch) {
            const int nl = std::min(per_launch, nb - l0);
            HIP_TRY(launch_quality(ptrs_dev + (host ? l0 : b0 + l0), nl, cn, w, h, rb, ksize, partials, records + (size_t)(b0 + l0) * 6, ctx->stream));
        }
    }
    HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
    std::vector<long long> rec((size_t)n * 6);
    HIP_TRY(hipMemcpyAsync(rec.data(), records, rec.size() * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ms) *ms = ev_ms(ctx->ev[0], ctx->ev[1]);
    for (int i = 0; i < n; i++) {
        const long long* r = rec.data() + (size_t)i * 6;             // LAPM x4 | LAPV sum, squares | TENG | GLVN sum, squares
        double* o = scores + (size_t)i * 4;
        o[STK_SHARPNESS_LAPM] = sharpness_finish(STK_SHARPNESS_LAPM, (double)r[0] * 0.25, 0.0, w, h);
        o[STK_SHARPNESS_LAPV] = sharpness_finish(STK_SHARPNESS_LAPV, (double)r[1], (double)r[2], w, h);
        o[STK_SHARPNESS_TENG] = sharpness_finish(STK_SHARPNESS_TENG, (double)r[3], 0.0, w, h);
        o[STK_SHARPNESS_GLVN] = sharpness_finish(STK_SHARPNESS_GLVN, (double)r[4], (double)r[5], w, h);
    }
    return STK_OK;
}

// examples/main.rs:53,64 on one column of the scores. Returns the status and, on failure, why.
stk_status rank_impl(const double* scores, int n, const stk_select_params* sel, int32_t* order, int32_t* n_kept, float* weights,
                     const char** why) {
    *why = "";
    if (!scores || !sel || !order || !n_kept) { *why = "rank: null argument"; return STK_INVALID_PARAMS; }
    if (n <= 0) { *why = "Not enough files"; return STK_NOT_ENOUGH_FILES; }
    if (sel->metric < STK_SHARPNESS_LAPM || sel->metric > STK_SHARPNESS_GLVN) { *why = "unknown sharpness metric"; return STK_INVALID_PARAMS; }
    if (sel->drop_worst < 0) { *why = "rank: drop_worst must be >= 0"; return STK_INVALID_PARAMS; }
    if (!(sel->keep_fraction >= 0.0f && sel->keep_fraction <= 1.0f)) { *why = "rank: keep_fraction must be 0 (off) or in (0, 1]"; return STK_INVALID_PARAMS; }
    if (sel->keep_fraction > 0.0f && sel->drop_worst != 0) { *why = "rank: keep_fraction and drop_worst exclude each other"; return STK_INVALID_PARAMS; }
    if (sel->weight_mode != STK_QUALITY_WEIGHT_NONE && sel->weight_mode != STK_QUALITY_WEIGHT_SCORE) { *why = "rank: unknown weight mode"; return STK_INVALID_PARAMS; }
    auto key = [&](int i) { return scores[(size_t)i * 4 + sel->metric]; };
    std::vector<int32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    // partial_cmp(..).unwrap_or(Equal): a NaN is equal to everything, which is no ordering a sort may be given as it is.
    // Defined as what a straight insertion sort (Rust's sort_by on slices of up to 20, the example's case) makes of it: a
    // NaN stays where it is and no frame moves across it. That is a stable sort of each NaN-free run on its own, which
    // costs O(n log n) whatever n is (a column without a NaN is one run).
    const auto less = [&](int32_t a, int32_t b) { return key(a) < key(b); };
    for (int lo = 0; lo < n;) {
        int hi = lo;
        while (hi < n && !std::isnan(key(hi))) hi++;
        std::stable_sort(idx.begin() + lo, idx.begin() + hi, less);
        lo = hi + 1;
    }
    long long kept = (long long)n - sel->drop_worst;
    if (sel->keep_fraction > 0.0f) kept = std::max<long long>(1, (long long)std::ceil((double)sel->keep_fraction * n));
    if (kept < 1) { *why = "Not enough files"; return STK_NOT_ENOUGH_FILES; }
    kept = std::min<long long>(kept, n);
    // skip the worst, reverse: the best frame first; then the dropped ones (best first too), so that order is a permutation
    for (int i = 0; i < n; i++) order[i] = idx[n - 1 - i];
    *n_kept = (int32_t)kept;
    if (weights) {
        const double best = key(order[0]);
        for (int i = 0; i < n; i++)
            weights[i] = (sel->weight_mode == STK_QUALITY_WEIGHT_SCORE && i < kept && best != 0.0) ? (float)(key(order[i]) / best) : 1.0f;
    }
    return STK_OK;
}

// score, select, and the kept frames' pointers in ranked order
stk_status ranked_list(stk_ctx* ctx, const stk_frames* frames, const stk_select_params* sel, int32_t* order, int32_t* n_kept,
                       double* scores_out, std::vector<const void*>& kept, double* ms) {
    if (!sel || !order || !n_kept) return fail(ctx, STK_INVALID_PARAMS, "ranked: null select parameters or outputs");
    stk_status st = quality_check(ctx, frames, sel->ksize);
    if (st) return st;
    std::vector<double> scores((size_t)frames->n * 4);
    if ((st = quality_scores(ctx, frames, sel->ksize, scores.data(), ms))) return st;
    const char* why = "";
    if ((st = rank_impl(scores.data(), frames->n, sel, order, n_kept, nullptr, &why))) return fail(ctx, st, why);
    if (scores_out) std::memcpy(scores_out, scores.data(), scores.size() * sizeof(double));
    kept.resize(*n_kept);
    for (int i = 0; i < *n_kept; i++) kept[i] = frames->data[order[i]];
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_stack_sharpness(stk_ctx* ctx, const stk_frames* frames, int32_t ksize, double* scores) {
    stk_status st = check_frames(ctx, frames, false, false);
    if (st) return st;
    if (!scores) return fail(ctx, STK_INVALID_PARAMS, "null scores");
    if ((st = quality_check(ctx, frames, ksize))) return st;
    timing_begin(ctx);
    double ms = 0.0;
    if ((st = quality_scores(ctx, frames, ksize, scores, &ms))) return st;
    ctx->timing.prep_ms = ms;
    return STK_OK;
}

stk_status stk_rank_frames(const double* scores, int32_t n, const stk_select_params* select, int32_t* order, int32_t* n_kept,
                           float* weights_or_null) {
    const char* why = "";
    return rank_impl(scores, n, select, order, n_kept, weights_or_null, &why);
}

stk_status stk_ecc_match_ranked(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                stk_image_f32* out, stk_frame_stats* stats, const stk_select_params* select, int32_t* order,
                                int32_t* n_kept, double* scores) {
    stk_status st = check_frames(ctx, frames, true);
    if (st) return st;
    std::vector<const void*> kept;
    double ms = 0.0;
    if ((st = ranked_list(ctx, frames, select, order, n_kept, scores, kept, &ms))) return st;
    stk_frames sub = *frames;
    sub.data = kept.data(); sub.n = (int32_t)kept.size();
    if ((st = stk_ecc_match(ctx, &sub, params, scale_down_width, out, stats))) return st;
    ctx->timing.prep_ms += ms;
    return STK_OK;
}

stk_status stk_keypoint_match_ranked(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                                     stk_image_f32* out, int32_t* dropped, stk_frame_stats* stats, const stk_select_params* select,
                                     int32_t* order, int32_t* n_kept, double* scores) {
    stk_status st = check_frames(ctx, frames, true);
    if (st) return st;
    std::vector<const void*> kept;
    double ms = 0.0;
    if ((st = ranked_list(ctx, frames, select, order, n_kept, scores, kept, &ms))) return st;
    stk_frames sub = *frames;
    sub.data = kept.data(); sub.n = (int32_t)kept.size();
    if ((st = stk_keypoint_match(ctx, &sub, params, scale_down_width, out, dropped, stats))) return st;
    ctx->timing.prep_ms += ms;
    return STK_OK;
}

}  // extern "C"
