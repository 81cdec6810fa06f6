// drizzle.h — what drizzle.cpp and kernels_drizzle.hip share (definition: include/stacker.h, stk_drizzle_params).
#pragma once
#include "common.h"

namespace stk {

// The frame table is the fold's (WarpFrame: src and the f32 output -> source matrix A_i; flags and Md are not read). The
// other per-entry tables are indexed like it.
struct DrizzleArgs {
    const WarpFrame* frames;
    int n_frames;
    int sw, sh, cn;
    size_t src_stride;               // elements per source row
    float alpha;
    int is_affine;
    const float* foot;               // affine entries: (hx, hy) per entry, clamped on the host; not read for homographies
    const stk_frame_weight* coef;    // gain / offset / weight per entry
    const float* const* maps;        // null: no maps; else per entry a tightly packed sw x sh plane, or null = all ones
    float hp, hmax, fill;            // 0.5f * pixfrac; 1.5f - 0.5f * pixfrac
    float* out;                      // ow x oh x cn, tightly packed
    float* den;                      // ow x oh, or null
    int ow, oh;
    // the mesh form (stk_mesh_drizzle_stack); fields == null: the plain kernels
    const float* const* fields;      // per entry a gh x gw x 2 f32 field on the grid of 1 << mesh_shift over sw x sh, or null = not displaced
    int mesh_shift, mesh_gw, mesh_gh;
    float mesh_inv;                  // 1.0f / step
    float mesh_g, mesh_tx, mesh_ty;  // the output grid's map onto frame 0, (float) of the host's g, tx, ty
    float mesh_s;                    // the scale
};

hipError_t launch_drizzle(const DrizzleArgs& a, int depth, hipStream_t s);

}  // namespace stk
