// demosaic_check.h — the argument checks of stk_demosaic and stk_cfa_mask (include/stacker.h, stk_mosaic) and the sizes
// the call works with. Included behind context.h; host arithmetic only, so a host-only program drives every refusal
// (tests/sanitize/demosaic_harness.cpp).
#pragma once
#include <string>

#include "spans.h"

namespace stk {

struct DemosaicPlan {
    int ow, oh;                 // the outputs' size: the mosaic's, or half of it (superpixel)
    size_t in_stride, in_span;  // bytes from row to row of a plane; bytes of a plane up to its last sample
    size_t out_row, out_stride, out_span;   // bytes of an output row's pixels; from row to row; of an output up to its last pixel
};

inline stk_status demosaic_check(const stk_mosaic* m, int method, int out_depth, void* const* out, size_t out_row_stride_bytes,
                                 DemosaicPlan* plan, std::string* why) {
    auto refuse = [&](stk_status st, const char* msg) { *why = msg; return st; };
    if (!m) return refuse(STK_INVALID_PARAMS, "demosaic: null mosaic");
    if (!m->data || !out) return refuse(STK_INVALID_PARAMS, "demosaic: null planes or outputs");
    if (m->n < 1) return refuse(STK_INVALID_PARAMS, "demosaic: no planes");
    if (m->pattern < STK_CFA_RGGB || m->pattern > STK_CFA_BGGR) return refuse(STK_INVALID_PARAMS, "demosaic: pattern must be STK_CFA_RGGB .. STK_CFA_BGGR");
    if (method < STK_DEMOSAIC_BILINEAR || method > STK_DEMOSAIC_SUPERPIXEL) return refuse(STK_INVALID_PARAMS, "demosaic: method must be STK_DEMOSAIC_BILINEAR .. STK_DEMOSAIC_SUPERPIXEL");
    if (m->depth != STK_DEPTH_U8 && m->depth != STK_DEPTH_U16 && m->depth != STK_DEPTH_F32) return refuse(STK_INVALID_PARAMS, "demosaic: depth must be 8, 16 or 32");
    if (m->location != STK_HOST && m->location != STK_DEVICE) return refuse(STK_INVALID_PARAMS, "demosaic: bad location");
    if (out_depth != m->depth && out_depth != STK_DEPTH_F32)
        return refuse(STK_INVALID_PARAMS, m->depth == 32 ? "demosaic: f32 mosaics go to STK_DEPTH_F32 only" : "demosaic: out_depth must be the mosaic's depth or STK_DEPTH_F32");
    const int least = method == STK_DEMOSAIC_SUPERPIXEL ? 2 : 3;
    if (m->width < least || m->height < least)
        return refuse(STK_INVALID_PARAMS, least == 2 ? "demosaic: a superpixel mosaic is at least 2 x 2" : "demosaic: the mosaic must be at least 3 x 3 (one reflection)");
    if ((size_t)m->width * m->height > (size_t)1 << 30) return refuse(STK_INVALID_PARAMS, "demosaic: mosaic too large");
    const size_t el = (size_t)m->depth / 8, oel = (size_t)out_depth / 8, row = (size_t)m->width * el;
    DemosaicPlan P{};
    P.ow = method == STK_DEMOSAIC_SUPERPIXEL ? m->width / 2 : m->width;
    P.oh = method == STK_DEMOSAIC_SUPERPIXEL ? m->height / 2 : m->height;
    P.in_stride = m->row_stride_bytes ? m->row_stride_bytes : row;
    if (P.in_stride < row || P.in_stride % el) return refuse(STK_INVALID_PARAMS, "demosaic: bad row stride of the mosaic");
    P.in_span = P.in_stride * (size_t)(m->height - 1) + row;
    P.out_row = (size_t)P.ow * 3 * oel;
    P.out_stride = out_row_stride_bytes ? out_row_stride_bytes : P.out_row;
    if (P.out_stride < P.out_row || P.out_stride % oel) return refuse(STK_INVALID_PARAMS, "demosaic: bad output row stride");
    P.out_span = P.out_stride * (size_t)(P.oh - 1) + P.out_row;
    for (int i = 0; i < m->n; i++)
        if (!m->data[i] || !out[i]) return refuse(STK_INVALID_PARAMS, "demosaic: null plane or output pointer");
    if (m->n > 65535) return refuse(STK_NOT_IMPLEMENTED, "demosaic: more than 65535 planes");
    if (demosaic_grid_rows(m->height, m->pattern, method) > 65535) return refuse(STK_NOT_IMPLEMENTED, "demosaic: more tile rows than a grid dimension holds");
    // no output may overlap a plane: outputs and planes lie in the same memory space
    SpanSet in;
    for (int i = 0; i < m->n; i++) in.add(m->data[i], P.in_span);
    in.seal();
    for (int i = 0; i < m->n; i++)
        if (in.overlaps(out[i], P.out_span)) return refuse(STK_INVALID_PARAMS, "demosaic: an output overlaps a plane of the mosaic");
    *plan = P;
    return STK_OK;
}

inline stk_status cfa_mask_check(int width, int height, int pattern, int channel, const float* plane, int location, std::string* why) {
    auto refuse = [&](const char* msg) { *why = msg; return STK_INVALID_PARAMS; };
    if (!plane) return refuse("cfa mask: null plane");
    if (width < 1 || height < 1 || (size_t)width * height > (size_t)1 << 30) return refuse("cfa mask: bad size");
    if (pattern < STK_CFA_RGGB || pattern > STK_CFA_BGGR) return refuse("cfa mask: pattern must be STK_CFA_RGGB .. STK_CFA_BGGR");
    if (channel < 0 || channel > 2) return refuse("cfa mask: channel must be 0 (B), 1 (G) or 2 (R)");
    if (location != STK_HOST && location != STK_DEVICE) return refuse("cfa mask: bad location");
    return STK_OK;
}

}  // namespace stk
