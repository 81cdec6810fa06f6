// reject.h — what reject.cpp and kernels_reject.hip share (definition: include/stacker.h, stk_reject_params).
#pragma once
#include "common.h"

namespace stk {

// One table entry per included frame. f is the fold's table entry, because the fold's coordinate fragment reads one: src
// and M, here the FORWARD matrix cast to f32 (frame pixels -> frame-0 coordinates), not inverted; flags and Md are not read.
struct RejectEntry {
    WarpFrame f;
    float gain[4], offset[4];
    const float* map_in;             // sw x sh, or null = all ones; never the plane map_out points to (the host copies an aliased plane)
    float* map_out;                  // sw x sh
};

struct RejectArgs {
    const RejectEntry* entries;
    int n_entries;
    int sw, sh, cn;
    size_t src_stride;               // elements per source row
    float alpha;
    int is_affine;
    const float* clean;              // sh x sw x cn, tightly packed
    const int* counts;               // sh x sw, or null
    int min_count;
    float snr1, snr2, scale1, scale2;
    float rn2, pg;                   // read_noise * read_noise (rounded to f32); poisson_gain
    unsigned long long* tallies;     // per entry: rejected, judged; zeroed before the launch
};

constexpr int REJECT_TW = 64, REJECT_TH = 16;      // the tile of one workgroup of 256 threads

hipError_t launch_reject(const RejectArgs& a, int depth, hipStream_t s);

}  // namespace stk
