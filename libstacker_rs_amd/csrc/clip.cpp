// clip.cpp — sigma-clipped stacking: stk_clip_stack, stk_ecc_match_clipped, stk_keypoint_match_clipped (an extension
// beyond the reference; definition in include/stacker.h, kernels in kernels_clip.hip).
// The combine starts from the plain mean c and runs iterations + 1 passes over the frames the fold added, each pass one
// launch of the fold kernel in its clip mode reading and rewriting the c / L / U planes (ctx->clip, 3 x 4 B per pixel and
// channel: 300 MB at 4K BGR, grow-only like the other workspaces). The whole-stack forms run the plain call first — its
// output IS c — and take the warps and the kept set from its stats; the frames are still resident in HBM (device stacks
// in place, host-fed stacks in ctx->frames where the upload left them), so nothing is uploaded again.
#include <cmath>
#include <cstring>

#include "context.h"

using namespace stk;

// (shared with robust.cpp: context.h)
stk_status clip_validate(stk_ctx* ctx, const stk_clip_params* p) {
    if (!p) return fail(ctx, STK_INVALID_PARAMS, "null clip parameters");
    if (!(p->kappa_low > 0.0f) || !std::isfinite(p->kappa_low) || !(p->kappa_high > 0.0f) || !std::isfinite(p->kappa_high))
        return fail(ctx, STK_INVALID_PARAMS, "sigma clipping: kappa_low and kappa_high must be finite and > 0");
    if (p->iterations < 1 || p->iterations > 16)
        return fail(ctx, STK_INVALID_PARAMS, "sigma clipping: iterations must be 1 .. 16, got " + std::to_string(p->iterations));
    return STK_OK;
}

stk_status clip_check_out(stk_ctx* ctx, const stk_image_f32* out, const stk_frames* f) {
    stk_status st = image_check(ctx, out, f->width, f->height, f->channels);
    if (st) return st;
    if (out->row_stride_bytes && out->row_stride_bytes != (size_t)f->width * f->channels * sizeof(float))
        return fail(ctx, STK_INVALID_PARAMS, "output must be tightly packed");
    return STK_OK;
}

namespace {

// The clip passes over the n_frames entries of ctx->warpframes; the c plane (ctx->clip) holds the plain mean. Writes `out`
// and `counts` (out's location) and sets stk_timing.finalize_ms to the passes' device time.
stk_status clip_passes(stk_ctx* ctx, int n_frames, int depth, int w, int h, int cn, size_t src_row_bytes, double alpha,
                       int border_mode, const double* border_value, int is_affine, const stk_clip_params* p,
                       stk_image_f32* out, int32_t* counts) {
    const size_t nel = (size_t)w * h * cn;
    float* c = ctx->clip.as<float>();
    WarpArgs a{};
    a.frames = ctx->warpframes.as<WarpFrame>();
    a.n_frames = n_frames;
    a.sw = w; a.sh = h; a.cn = cn;
    a.src_stride = src_row_bytes / (depth / 8);
    a.alpha = (float)alpha;
    a.border_mode = border_mode;
    for (int k = 0; k < 4; k++) a.bv[k] = border_value ? (float)border_value[k] : 0.f;
    a.acc = nullptr; a.dw = w; a.dh = h; a.acc_stride = 0;
    a.is_affine = is_affine; a.subpixel_bits = ctx->opt_subpixel_bits; a.tune = 0; a.interp = ctx->opt_interp;
    const bool host = out->location != STK_DEVICE;
    ClipArgs ca{};
    ca.c = c; ca.L = c + nel; ca.U = c + 2 * nel;
    ca.plane_stride = (size_t)w * cn;
    // a host output goes through the planes themselves: each thread reads its c, L, U before it writes out / counts there
    ca.out = host ? c : out->data;
    ca.out_stride = (size_t)w * cn;
    ca.counts = counts ? (host ? (int*)ca.L : counts) : nullptr;
    ca.kappa_low = p->kappa_low; ca.kappa_high = p->kappa_high;
    HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    for (int t = 1; t <= p->iterations + 1; t++) {
        ca.first = t == 1;
        ca.last = t == p->iterations + 1;
        HIP_TRY(launch_clip_pass(a, ca, depth, ctx->stream));
    }
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    if (host) {
        HIP_TRY(hipMemcpyAsync(out->data, c, nel * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (counts) HIP_TRY(hipMemcpyAsync(counts, ca.L, nel * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.finalize_ms = ev_ms(ctx->ev[4], ctx->ev[5]);
    return STK_OK;
}

}  // namespace

extern "C" {

stk_status stk_clip_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include, int32_t is_affine,
                          int32_t border_mode, const double* border_value, double alpha, const stk_clip_params* clip,
                          stk_image_f32* out, int32_t* counts) {
    stk_status st = check_frames(ctx, frames, false);
    if (st) return st;
    if (!M) return fail(ctx, STK_INVALID_PARAMS, "null matrix");
    if (border_mode < 0 || border_mode > 4)
        return fail(ctx, border_mode == STK_BORDER_TRANSPARENT ? STK_NOT_IMPLEMENTED : STK_INVALID_PARAMS,
                    "border mode not supported (BORDER_TRANSPARENT leaves the reference's output uninitialised)");
    if ((st = clip_validate(ctx, clip))) return st;
    if ((st = clip_check_out(ctx, out, frames))) return st;
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    int n_in = 0;
    for (int i = 0; i < n; i++) n_in += (!include || include[i]) ? 1 : 0;
    if (n_in == 0) return fail(ctx, STK_INVALID_PARAMS, "sigma clipping: no frame included");
    (void)hipSetDevice(ctx->device);
    timing_begin(ctx);
    std::vector<const void*> dev;
    if ((st = resolve_frames(ctx, frames, dev))) return st;
    const size_t nel = (size_t)w * h * cn, rb = frame_row_bytes(frames);
    HIP_TRY(ctx->clip.reserve(3 * nel * sizeof(float)));
    std::vector<WarpFrame> wf;
    wf.reserve(n_in);
    for (int i = 0; i < n; i++) {
        if (include && !include[i]) continue;
        wf.emplace_back();
        make_warp_frame(wf.back(), dev[i], M + 9 * (size_t)i, is_affine);
    }
    // c = the plain mean: the fold, then stk_finalize_mean's scale
    float* c = ctx->clip.as<float>();
    HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
    if ((st = warp_fold(ctx, wf, frames->depth, w, h, cn, rb, alpha, border_mode, border_value, is_affine, c, (size_t)w * cn, 0))) return st;
    HIP_TRY(launch_scale(c, c, nel, (float)(1.0 / (double)n_in), ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));
    if ((st = clip_passes(ctx, (int)wf.size(), frames->depth, w, h, cn, rb, alpha, border_mode, border_value, is_affine, clip, out, counts)))
        return st;
    ctx->timing.warp_ms = ev_ms(ctx->ev[2], ctx->ev[3]);
    return STK_OK;
}

stk_status stk_ecc_match_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                 const stk_clip_params* clip, stk_image_f32* out, int32_t* counts, stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = clip_validate(ctx, clip);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = clip_check_out(ctx, out, frames))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const size_t nel = (size_t)w * h * cn;
    HIP_TRY(ctx->clip.reserve(3 * nel * sizeof(float)));
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    // the plain call, on this context's own device, straight into the c plane
    stk_image_f32 cimg{ctx->clip.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = ecc_match_single(ctx, frames, params, scale_down_width, &cimg, stats))) return st;
    const stk_timing keep = ctx->timing;
    // every frame is a sample (a failed frame fails the plain call): frame 0 through the identity, frame i through its
    // warp — the table launch_warp_frames_from_ecc / ecc_shard_impl built from the same f32 warps
    const int is_affine = params->motion_type != STK_MOTION_HOMOGRAPHY;
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    std::vector<WarpFrame> wf(n);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    make_warp_frame(wf[0], dev[0], I3, is_affine);
    for (int i = 1; i < n; i++) make_warp_frame(wf[i], dev[i], stats[i].warp, is_affine);
    const size_t rb = frame_row_bytes(frames);
    if ((st = warp_table_upload(ctx, wf, rb, w, h, is_affine))) return st;
    st = clip_passes(ctx, n, frames->depth, w, h, cn, rb, 1.0 / 255.0, STK_BORDER_CONSTANT, nullptr, is_affine, clip, out, counts);
    const double fin = ctx->timing.finalize_ms;
    ctx->timing = keep; ctx->timing.finalize_ms = fin;
    return st;
}

stk_status stk_keypoint_match_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                                      const stk_clip_params* clip, stk_image_f32* out, int32_t* dropped, int32_t* counts,
                                      stk_frame_stats* stats) {
    if (!ctx) return STK_INVALID_PARAMS;
    stk_status st = clip_validate(ctx, clip);
    if (st) return st;
    if ((st = check_frames(ctx, frames, true))) return st;
    if ((st = clip_check_out(ctx, out, frames))) return st;
    (void)hipSetDevice(ctx->device);
    const int n = frames->n, w = frames->width, h = frames->height, cn = frames->channels;
    const size_t nel = (size_t)w * h * cn;
    HIP_TRY(ctx->clip.reserve(3 * nel * sizeof(float)));
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    stk_image_f32 cimg{ctx->clip.as<float>(), w, h, cn, STK_DEVICE, 0};
    if ((st = keypoint_match_single(ctx, frames, params, scale_down_width, &cimg, dropped, stats))) return st;
    const stk_timing keep = ctx->timing;
    // the samples: frame 0 through the identity and the frames with a homography (status 0), in stack order, with the
    // params' border — what stk_keypoint_match_shard folded
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    std::vector<WarpFrame> wf;
    wf.reserve(n);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    wf.emplace_back();
    make_warp_frame(wf.back(), dev[0], I3, 0);
    for (int i = 1; i < n; i++) {
        if (stats[i].status != 0) continue;
        wf.emplace_back();
        make_warp_frame(wf.back(), dev[i], stats[i].warp, 0);
    }
    const size_t rb = frame_row_bytes(frames);
    if ((st = warp_table_upload(ctx, wf, rb, w, h, 0))) return st;
    st = clip_passes(ctx, (int)wf.size(), 8, w, h, cn, rb, 1.0 / 255.0, params->border_mode, params->border_value, 0, clip, out, counts);
    const double fin = ctx->timing.finalize_ms;
    ctx->timing = keep; ctx->timing.finalize_ms = fin;
    return st;
}

}  // extern "C"
