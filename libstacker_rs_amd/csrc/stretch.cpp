// stretch.cpp — the display stretch of a finished stack: stk_image_stats, stk_stretch, stk_auto_stretch, and the host
// helpers stk_stretch_auto and stk_stretch_table (an extension beyond the reference; definition in include/stacker.h,
// "display stretch"; kernels in post/kernels_stretch.hip, the host half in stretch_host.h).
// ctx->local (StretchLayout, workspace.h) holds the selection's words, the copy of a host image, the copy of a host mask,
// the table and the staged output of a host image. A host image is uploaded once per call and the result goes back with one
// strided copy that writes the pixel bytes of each row and nothing else. The statistics read the count of each channel back
// once, after the first pass, to form the ranks; everything else of a call is queued behind it without a wait.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "context.h"
#include "spans.h"
#include "stretch_host.h"

using namespace stk;

namespace {

stk_status st_image_check(stk_ctx* ctx, const stk_image_f32* im) {
    if (!im || !im->data) return fail(ctx, STK_INVALID_PARAMS, "stretch: null image");
    if (im->width <= 0 || im->height <= 0 || (im->channels != 1 && im->channels != 3 && im->channels != 4))
        return fail(ctx, STK_INVALID_PARAMS, "stretch: bad geometry of the image (1, 3 or 4 channels)");
    if ((size_t)im->width * im->height >= (size_t)1 << 31) return fail(ctx, STK_INVALID_PARAMS, "stretch: the image is too large");
    if (im->location != STK_HOST && im->location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, "stretch: bad location of the image");
    if (im->row_stride_bytes && (im->row_stride_bytes % 4 || im->row_stride_bytes < (size_t)im->width * im->channels * 4))
        return fail(ctx, STK_INVALID_PARAMS, "stretch: bad row stride of the image");
    return STK_OK;
}

// The round that stk_timing.warp_ms brackets: round 1 of the values' selection. The environment variable STK_STRETCH_TIME_ROUND
// ("<phase><round>", phase v or m, round 0 .. 3: "v2", "m0"), read at every call, picks another: the hook by which
// tools/stretch_time.py times each round of a call in one process. (v0 is the first pass, which prep_ms holds: it reads 0.)
void st_timed_round(int& phase, int& round) {
    phase = 0; round = 1;
    const char* e = std::getenv("STK_STRETCH_TIME_ROUND");
    if (e && (e[0] == 'v' || e[0] == 'm') && e[1] >= '0' && e[1] < '0' + ST_ROUNDS && !e[2]) { phase = e[0] == 'm'; round = e[1] - '0'; }
}

// The form of the histogram launches: the one that measured faster. The environment variable
// STK_STRETCH_HIST_FORM ("direct" or "merged"), read at every call, overrides it: the hook by which the tests run both forms
// against the restatement and tools/stretch_time.py times them side by side in one process.
constexpr int ST_FORM_DEFAULT = ST_FORM_MERGED;
int st_hist_form() {
    const char* e = std::getenv("STK_STRETCH_HIST_FORM");
    if (e && !std::strcmp(e, "merged")) return ST_FORM_MERGED;
    if (e && !std::strcmp(e, "direct")) return ST_FORM_DIRECT;
    return ST_FORM_DEFAULT;
}

// (both runs add their launches to stk_timing.finalize_ms: the whole form is their sum)
stk_status stats_run(stk_ctx* ctx, const stk_image_f32* in, const float* mask, size_t mask_stride_bytes, int32_t mask_location,
                     const double* quantiles, int nq, stk_image_stat* stats) {
    stk_status st = st_image_check(ctx, in);
    if (st) return st;
    if (!stats) return fail(ctx, STK_INVALID_PARAMS, "image statistics: null records");
    if (const char* e = stretch::validate_quantiles(quantiles, nq)) return fail(ctx, STK_INVALID_PARAMS, e);
    const int w = in->width, h = in->height, cn = in->channels, cc = std::min(cn, 3);
    const size_t mrow = (size_t)w * 4, mstride = mask_stride_bytes ? mask_stride_bytes : mrow;
    if (mask) {
        if (mask_location != STK_HOST && mask_location != STK_DEVICE) return fail(ctx, STK_INVALID_PARAMS, "image statistics: bad location of the mask");
        if (mstride < mrow || mstride % 4) return fail(ctx, STK_INVALID_PARAMS, "image statistics: bad row stride of the mask");
    }
    const size_t row = (size_t)w * cn * 4, istride = image_stride_floats(in) * 4;
    const bool host = in->location == STK_HOST, mask_host = mask && mask_location == STK_HOST;
    {
        // the records are host memory: they may not lie over a host image, a host mask or the quantiles
        SpanSet reads;
        if (host) reads.add(in->data, istride * (size_t)(h - 1) + row);
        if (mask_host) reads.add(mask, mstride * (size_t)(h - 1) + mrow);
        if (nq) reads.add(quantiles, (size_t)nq * sizeof(double));
        reads.seal();
        if (reads.overlaps(stats, 4 * sizeof(stk_image_stat))) return fail(ctx, STK_INVALID_PARAMS, "image statistics: the records overlap an input");
    }

    (void)hipSetDevice(ctx->device);
    const StretchLayout L = stretch_layout(cc, host ? row * (size_t)h : 0, mask_host ? mrow * (size_t)h : 0, 0, 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "image statistics"))) return st;
    char* base = ctx->local.as<char>();

    StStatArgs a{};
    a.in = in->data; a.in_stride = istride / 4;
    if (host) {
        HIP_TRY(hipMemcpy2DAsync(base + L.image, row, in->data, istride, row, h, hipMemcpyHostToDevice, ctx->stream));
        a.in = (const float*)(base + L.image); a.in_stride = row / 4;
    }
    a.mask = mask; a.mask_stride = mstride / 4;
    if (mask_host) {
        HIP_TRY(hipMemcpy2DAsync(base + L.mask, mrow, mask, mstride, mrow, h, hipMemcpyHostToDevice, ctx->stream));
        a.mask = (const float*)(base + L.mask); a.mask_stride = (size_t)w;
    }
    a.state = (uint32_t*)(base + L.state);
    a.w = w; a.h = h; a.cn = cn; a.channels = cc;
    a.form = st_hist_form();

    // the first bracket: the counts, min and max and the first digit of the values
    a.round = 0; a.slot0 = 0; a.slots = 1 + nq;
    HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    HIP_TRY(launch_stretch_stat_reset(a, ctx->stream));
    HIP_TRY(launch_stretch_stat_hist(a, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
    std::vector<uint32_t> words(st_state_words(cc));
    HIP_TRY(hipMemcpyAsync(words.data(), a.state, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int64_t N[3] = {};
    for (int c = 0; c < cc; c++) {
        for (int b = 0; b < ST_BINS; b++) N[c] += words[st_bins_at(cc, c, 0) + b];
        a.rank[c][0] = (uint32_t)((N[c] + 1) / 2);
        for (int i = 0; i < nq; i++) a.rank[c][1 + i] = N[c] ? (uint32_t)stretch::quantile_rank(quantiles[i], N[c]) : 0u;
        a.rank[c][ST_MAD] = a.rank[c][0];
    }

    // the second bracket: the rest of the values' selection, then the MAD's
    int tphase, tround;
    st_timed_round(tphase, tround);
    const bool timed = tphase || tround;
    HIP_TRY(hipEventRecord(ctx->ev[7], ctx->stream));
    for (int phase = 0; phase < 2; phase++) {
        a.slot0 = phase ? ST_MAD : 0; a.slots = phase ? 1 : 1 + nq;
        for (int r = 0; r < ST_ROUNDS; r++) {
            a.round = r;
            if (phase && r == 1) HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
            if (timed && phase == tphase && r == tround) HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
            if (phase || r) HIP_TRY(launch_stretch_stat_hist(a, ctx->stream));
            HIP_TRY(launch_stretch_stat_pick(a, ctx->stream));
            if (timed && phase == tphase && r == tround) HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));
            if (phase && r == 1) HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
        }
    }
    HIP_TRY(hipEventRecord(ctx->ev[6], ctx->stream));
    const size_t head = (size_t)cc * (ST_HEAD + 2 * ST_SLOTS);
    HIP_TRY(hipMemcpyAsync(words.data(), a.state, head * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::memset(stats, 0, 4 * sizeof(stk_image_stat));
    for (int c = 0; c < cc; c++) {
        if (!N[c]) continue;
        stk_image_stat& s = stats[c];
        s.count = N[c];
        s.min = stretch::value_of_key(words[(size_t)c * ST_HEAD]);
        s.max = stretch::value_of_key(words[(size_t)c * ST_HEAD + 1]);
        s.median = stretch::value_of_key(words[st_sel_at(cc, c, 0)]);
        for (int i = 0; i < nq; i++) s.q[i] = stretch::value_of_key(words[st_sel_at(cc, c, 1 + i)]);
        std::memcpy(&s.mad, &words[st_sel_at(cc, c, ST_MAD)], sizeof(float));
    }
    ctx->timing.finalize_ms += ev_ms(ctx->ev[0], ctx->ev[1]) + ev_ms(ctx->ev[7], ctx->ev[6]);
    ctx->timing.prep_ms = ev_ms(ctx->ev[0], ctx->ev[1]);
    ctx->timing.warp_ms = timed ? ev_ms(ctx->ev[2], ctx->ev[3]) : 0.0;
    ctx->timing.align_ms = ev_ms(ctx->ev[4], ctx->ev[5]);
    return STK_OK;
}

stk_status stretch_run(stk_ctx* ctx, const stk_image_f32* in, const stk_stretch_params* p, const float* table, int knots, stk_image_out* out) {
    stk_status st = st_image_check(ctx, in);
    if (st) return st;
    if (!out || !out->data) return fail(ctx, STK_INVALID_PARAMS, "stretch: null output");
    const int w = in->width, h = in->height, cn = in->channels, cc = std::min(cn, 3);
    if (const char* e = stretch::validate(p, cn, table, knots)) return fail(ctx, STK_INVALID_PARAMS, e);
    if (out->width != w || out->height != h || out->channels != cn || out->location != in->location || out->depth != p->out_depth)
        return fail(ctx, STK_INVALID_PARAMS, "stretch: the output must have the image's geometry and location and the parameters' depth");
    const size_t eb = (size_t)p->out_depth / 8, orow = (size_t)w * cn * eb, ostride = out->row_stride_bytes ? out->row_stride_bytes : orow;
    if (ostride < orow || ostride % eb) return fail(ctx, STK_INVALID_PARAMS, "stretch: bad row stride of the output");
    const size_t row = (size_t)w * cn * 4, istride = image_stride_floats(in) * 4;
    const bool tabled = p->curve == STK_STRETCH_TABLE, host = in->location == STK_HOST;
    const size_t tbytes = tabled ? ((size_t)knots + 1) * sizeof(float) : 0;
    {
        const bool in_place = p->out_depth == STK_DEPTH_F32 && out->data == (void*)in->data && ostride == istride;
        SpanSet reads;
        if (!in_place) reads.add(in->data, istride * (size_t)(h - 1) + row);
        if (tabled && host) reads.add(table, tbytes);
        reads.seal();
        if (reads.overlaps(out->data, ostride * (size_t)(h - 1) + orow))
            return fail(ctx, STK_INVALID_PARAMS, "stretch: the output overlaps the image or the table (an f32 output may only be the image itself: same pointer, same row stride)");
    }

    (void)hipSetDevice(ctx->device);
    const StretchLayout L = stretch_layout(0, host ? row * (size_t)h : 0, 0, tbytes, host ? orow * (size_t)h : 0);
    if ((st = workspace_reserve(ctx, ctx->local, L.total, "stretch"))) return st;
    char* base = ctx->local.as<char>();

    StStretchArgs a{};
    a.in = in->data; a.in_stride = istride / 4;
    a.out = out->data; a.out_stride = ostride / eb;
    if (host) {
        HIP_TRY(hipMemcpy2DAsync(base + L.image, row, in->data, istride, row, h, hipMemcpyHostToDevice, ctx->stream));
        a.in = (const float*)(base + L.image); a.in_stride = row / 4;
        a.out = base + L.out; a.out_stride = orow / eb;
    }
    if (tabled) {
        HIP_TRY(hipMemcpyAsync(base + L.table, table, tbytes, hipMemcpyHostToDevice, ctx->stream));
        a.table = (const float*)(base + L.table);
    }
    a.w = w; a.h = h; a.cn = cn; a.depth = p->out_depth; a.curve = p->curve; a.colour = cn >= 3 ? p->colour : 0; a.knots = tabled ? knots : 0;
    for (int c = 0; c < cc; c++) {
        a.black[c] = p->black[c];
        a.r[c] = p->white[c] - p->black[c];
        a.mid[c] = p->midtone[c];
        a.mm1[c] = p->midtone[c] - 1.0f;
        a.k[c] = 2.0f * p->midtone[c] - 1.0f;
    }
    a.out_scale = p->out_scale;
    for (int c = 0; c < cc; c++)
        if (!(a.r[c] > 0.0f) || !std::isfinite(a.r[c])) return fail(ctx, STK_INVALID_PARAMS, "stretch: white - black must be a positive finite f32");
    HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    HIP_TRY(launch_stretch(a, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
    if (host) HIP_TRY(hipMemcpy2DAsync(out->data, ostride, a.out, orow, orow, h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.finalize_ms += ev_ms(ctx->ev[0], ctx->ev[1]);
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_stretch_auto(const stk_image_stat* stats, int32_t channels, const stk_stretch_auto_params* params, stk_stretch_params* out) {
    return stretch::auto_params(stats, channels, params, out);
}

stk_status stk_stretch_table(int32_t kind, double param, int32_t knots, float* table) { return stretch::table(kind, param, knots, table); }

stk_status stk_image_stats(stk_ctx* ctx, const stk_image_f32* in, const float* mask, size_t mask_stride_bytes, int32_t mask_location,
                           const double* quantiles, int32_t n_quantiles, stk_image_stat* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    timing_begin(ctx);
    return stats_run(ctx, in, mask, mask_stride_bytes, mask_location, quantiles, n_quantiles, stats);
}

stk_status stk_stretch(stk_ctx* ctx, const stk_image_f32* in, const stk_stretch_params* params, const float* table, int32_t knots, stk_image_out* out) {
    if (!ctx) return STK_INVALID_PARAMS;
    if (!params) return fail(ctx, STK_INVALID_PARAMS, "null stretch parameters");
    timing_begin(ctx);
    return stretch_run(ctx, in, params, table, knots, out);
}

stk_status stk_auto_stretch(stk_ctx* ctx, const stk_image_f32* in, const float* mask, size_t mask_stride_bytes, int32_t mask_location,
                            const stk_stretch_auto_params* auto_params, int32_t curve, int32_t colour, float out_scale, const float* table,
                            int32_t knots, stk_image_out* out, stk_image_stat* stats_out, stk_stretch_params* params_out) {
    if (!ctx) return STK_INVALID_PARAMS;
    const stk_stretch_auto_params ap = auto_params ? *auto_params : stretch::auto_defaults();
    if (const char* e = stretch::validate_auto(&ap)) return fail(ctx, STK_INVALID_PARAMS, e);
    if (!out) return fail(ctx, STK_INVALID_PARAMS, "stretch: null output");
    stk_status st = st_image_check(ctx, in);
    if (st) return st;
    // what the stretch will refuse is refused before the statistics run: the parameters with a stand-in black and white
    stk_stretch_params p{};
    p.curve = curve; p.colour = colour; p.out_depth = out->depth; p.out_scale = out_scale;
    for (int c = 0; c < 4; c++) { p.black[c] = 0.0f; p.white[c] = 1.0f; p.midtone[c] = 0.5f; }
    if (const char* e = stretch::validate(&p, in->channels, table, knots)) return fail(ctx, STK_INVALID_PARAMS, e);
    timing_begin(ctx);
    stk_image_stat stats[4];
    const double q = ap.white_quantile;
    if ((st = stats_run(ctx, in, mask, mask_stride_bytes, mask_location, &q, ap.white_mode == 2 ? 1 : 0, stats))) return st;
    stk_stretch_params rule;
    if (stretch::auto_params(stats, in->channels, &ap, &rule) != STK_OK) return fail(ctx, STK_INVALID_PARAMS, "auto stretch: the rule refused the statistics");
    std::memcpy(p.black, rule.black, sizeof p.black);
    std::memcpy(p.white, rule.white, sizeof p.white);
    std::memcpy(p.midtone, rule.midtone, sizeof p.midtone);
    if ((st = stretch_run(ctx, in, &p, table, knots, out))) return st;
    if (stats_out) std::memcpy(stats_out, stats, sizeof stats);
    if (params_out) *params_out = p;
    return STK_OK;
}

}  // extern "C"
