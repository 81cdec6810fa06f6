// combine.cpp — the host front end every combine shares: declarations and contracts in combine.h.
#include "context.h"

using namespace stk;

FoldSpec fold_spec(const stk_frames* frames, double alpha, int border_mode, const double* border_value, int is_affine) {
    return FoldSpec{frames->depth, frames->width, frames->height, frames->channels, frame_row_bytes(frames), alpha, border_mode,
                    border_value, is_affine};
}

FoldSpec fold_spec_ecc(const stk_frames* frames, const stk_ecc_params* params) {
    return fold_spec(frames, 1.0 / 255.0, STK_BORDER_CONSTANT, nullptr, params->motion_type != STK_MOTION_HOMOGRAPHY);
}

FoldSpec fold_spec_keypoint(const stk_frames* frames, const stk_keypoint_params* params) {
    FoldSpec spec = fold_spec(frames, 1.0 / 255.0, params->border_mode, params->border_value, 0);
    spec.depth = 8;
    return spec;
}

WarpArgs fold_warp_args(stk_ctx* ctx, int n_entries, const FoldSpec& s) {
    WarpArgs a{};
    a.frames = ctx->warpframes.as<WarpFrame>();
    a.n_frames = n_entries;
    a.sw = s.w; a.sh = s.h; a.cn = s.cn;
    a.src_stride = s.src_row_bytes / (s.depth / 8);
    a.alpha = (float)s.alpha;
    a.border_mode = s.border_mode;
    for (int k = 0; k < 4; k++) a.bv[k] = s.border_value ? (float)s.border_value[k] : 0.f;
    a.acc = nullptr; a.dw = s.w; a.dh = s.h; a.acc_stride = 0;
    a.is_affine = s.is_affine; a.subpixel_bits = ctx->opt_subpixel_bits; a.tune = 0; a.interp = ctx->opt_interp;
    return a;
}

stk_status entry_table_upload(stk_ctx* ctx, const stk_frames* frames, const std::vector<const void*>& dev, const EntryTable& table,
                              int is_affine) {
    std::vector<WarpFrame> wf(table.frame.size());
    for (size_t k = 0; k < wf.size(); k++) make_warp_frame(wf[k], dev[table.frame[k]], table.M[k], is_affine);
    stk_status st = warp_table_upload(ctx, wf, frame_row_bytes(frames), frames->width, frames->height, is_affine);
    if (st) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));       // `wf` leaves scope
    return STK_OK;
}

stk_status entry_table_begin(stk_ctx* ctx, const stk_frames* frames, const EntryTable& table, int is_affine) {
    (void)hipSetDevice(ctx->device);
    timing_begin(ctx);
    std::vector<const void*> dev;
    stk_status st = resolve_frames(ctx, frames, dev);
    if (st) return st;
    return entry_table_upload(ctx, frames, dev, table, is_affine);
}

stk_frame_weight unit_record() {
    stk_frame_weight e;
    for (int c = 0; c < 4; c++) { e.gain[c] = 1.0f; e.offset[c] = 0.0f; }
    e.weight = 1.0f; e.flags = 0;
    return e;
}

void gather_records(const EntryTable& table, const stk_frame_weight* per_frame, std::vector<stk_frame_weight>& coef) {
    coef.clear();
    for (int i : table.frame) coef.push_back(per_frame ? per_frame[i] : unit_record());
}

stk_status check_border_mode(stk_ctx* ctx, int border_mode) {
    if (border_mode < 0 || border_mode > 4)
        return fail(ctx, border_mode == STK_BORDER_TRANSPARENT ? STK_NOT_IMPLEMENTED : STK_INVALID_PARAMS,
                    "border mode not supported (BORDER_TRANSPARENT leaves the reference's output uninitialised)");
    return STK_OK;
}

stk_status combine_check_out(stk_ctx* ctx, const stk_image_f32* out, const stk_frames* f) {
    stk_status st = image_check(ctx, out, f->width, f->height, f->channels);
    if (st) return st;
    if (out->row_stride_bytes && out->row_stride_bytes != (size_t)f->width * f->channels * sizeof(float))
        return fail(ctx, STK_INVALID_PARAMS, "output must be tightly packed");
    return STK_OK;
}

namespace {

// exactly one of ep / kp is asked, by `keypoint` (either may be null: the plain call reports that)
stk_status match_then(stk_ctx* ctx, const stk_frames* frames, bool keypoint, const stk_ecc_params* ep, const stk_keypoint_params* kp,
                      float scale_down_width, float* mean, int32_t* dropped, stk_frame_stats* stats, const CombineFinish& finish) {
    const int n = frames->n;
    std::vector<stk_frame_stats> own;
    if (!stats) { own.resize(n); stats = own.data(); }
    stk_image_f32 mimg{mean, frames->width, frames->height, frames->channels, STK_DEVICE, 0};
    stk_status st = keypoint ? keypoint_match_single(ctx, frames, kp, scale_down_width, &mimg, dropped, stats)
                             : ecc_match_single(ctx, frames, ep, scale_down_width, &mimg, stats);
    if (st) return st;
    const stk_timing keep = ctx->timing;
    const FoldSpec spec = keypoint ? fold_spec_keypoint(frames, kp) : fold_spec_ecc(frames, ep);
    std::vector<const void*> dev;
    resident_frames(ctx, frames, dev);
    EntryTable table;
    entries_from_stats(n, stats, keypoint, table);
    double ms = 0.0;
    st = entry_table_upload(ctx, frames, dev, table, spec.is_affine);
    if (!st) st = finish(table, dev, spec, stats, &ms);
    ctx->timing = keep; ctx->timing.finalize_ms = st ? 0.0 : ms;
    return st;
}

}  // namespace

stk_status ecc_match_then(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width, float* mean,
                          stk_frame_stats* stats, const CombineFinish& finish) {
    return match_then(ctx, frames, false, params, nullptr, scale_down_width, mean, nullptr, stats, finish);
}

stk_status keypoint_match_then(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params, float scale_down_width,
                               float* mean, int32_t* dropped, stk_frame_stats* stats, const CombineFinish& finish) {
    return match_then(ctx, frames, true, nullptr, params, scale_down_width, mean, dropped, stats, finish);
}
