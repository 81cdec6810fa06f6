// noise_host.h — the host half of noise estimation (include/stacker.h, stk_noise_stat): the reduction of one frame
// channel's two histograms to its statistics, and the inverse-variance frame weights. Inline, no HIP type and no stk_ctx,
// so that a host-only program can call them (tests/sanitize/noise_harness.cpp); noise.cpp exports them as
// stk_noise_from_hist and stk_noise_weights. All sums are integers; the floating operations are the ones the header
// names, each rounded on its own (-ffp-contract=off).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/stacker.h"

namespace stk {
namespace noise {

constexpr int NOISE_ROUNDS = 16;
constexpr double NOISE_TRUNCATION = 1.0136;      // 1 / sqrt(1 - 6 phi(3) / (2 Phi(3) - 1)): a Gaussian cut at 3 sigma

// the k-th smallest key of a histogram (k >= 0; k = 0 and an empty histogram: 0; k above the total: bins - 1)
inline int32_t kth_smallest(const uint32_t* h, int32_t bins, int64_t k) {
    int64_t cum = 0;
    for (int32_t b = 0; b < bins; b++) {
        cum += h[b];
        if (cum >= k) return b;
    }
    return bins - 1;
}

inline stk_status from_hist(const uint32_t* hv, int32_t bv, const uint32_t* hr, int32_t br, int32_t overflow_bin, stk_noise_stat* out) {
    if (!hv || !hr || !out || bv < 1 || bv > 65536 || br < 2 || br > 65536 || overflow_bin < 0 || overflow_bin > 1) return STK_INVALID_PARAMS;
    std::memset(out, 0, sizeof(*out));
    // 1. median and MAD of the values, from the cumulative counts
    std::vector<int64_t> cum((size_t)bv);
    int64_t n = 0;
    for (int32_t b = 0; b < bv; b++) { n += hv[b]; cum[b] = n; }
    const int64_t k = (n + 1) / 2;
    int32_t med = 0;
    while (med < bv - 1 && cum[med] < k) med++;
    int32_t mad = 0;
    for (; mad < bv - 1; mad++) {                                     // #{|v - med| <= d} = cum(med + d) - cum(med - d - 1)
        const int32_t hi = std::min(med + mad, bv - 1), lo = med - mad - 1;
        if (cum[hi] - (lo >= 0 ? cum[lo] : 0) >= k) break;
    }
    out->median = med; out->mad = mad;
    // 2. the median of the capped |r|
    int64_t m = 0;
    for (int32_t b = 0; b < br; b++) m += hr[b];
    out->res_median = kth_smallest(hr, br, (m + 1) / 2);
    // 3. - 5. the 3-sigma truncated second moment, iterated to a fixed cut
    double s = std::max(1.4826 * (double)out->res_median, 0.5);
    const int32_t top = overflow_bin ? br - 2 : br - 1;
    int32_t prev = -1, cut = 0;
    int64_t N = 0;
    bool zero = false;
    for (int round = 0; round < NOISE_ROUNDS; round++) {
        cut = (int32_t)std::min(std::floor(3.0 * s), (double)top);
        if (cut == prev) break;
        prev = cut;
        int64_t Q = 0;
        N = 0;
        for (int32_t b = 0; b <= cut; b++) { N += hr[b]; Q += (int64_t)b * b * (int64_t)hr[b]; }
        if (N == 0 || Q == 0) { zero = true; break; }
        s = std::sqrt((double)Q / (double)N) * NOISE_TRUNCATION;
    }
    out->sigma = zero ? 0.0 : s / 6.0;                                // the mask's coefficients have squared sum 36
    out->kept = N;
    out->flags = (zero ? 1 : 0) | ((overflow_bin && cut == top) ? 2 : 0);
    return STK_OK;
}

inline stk_status weights(const stk_noise_stat* stats, int32_t n, int32_t channels, const stk_frame_weight* records, const int32_t* include,
                          const float* user, double sigma_floor, float* out) {
    if (!stats || !out || n < 1 || (channels != 1 && channels != 3 && channels != 4)) return STK_INVALID_PARAMS;
    if (!std::isfinite(sigma_floor) || !(sigma_floor > 0.0)) return STK_INVALID_PARAMS;
    const int C = std::min(channels, 3);
    std::vector<double> V((size_t)n, 0.0);
    int ref = -1;
    for (int32_t i = 0; i < n; i++) {
        if (user && (!std::isfinite(user[i]) || user[i] < 0.0f)) return STK_INVALID_PARAMS;
        if (include && !include[i]) continue;
        if (ref < 0) ref = i;
        double v = 0.0;
        for (int c = 0; c < C; c++) {
            const double sg = stats[(size_t)i * 4 + c].sigma, g = records ? (double)records[i].gain[c] : 1.0;
            if (!std::isfinite(sg) || sg < 0.0 || !std::isfinite(g)) return STK_INVALID_PARAMS;
            const double t = g * std::max(sg, sigma_floor);
            v += t * t;
        }
        if (!(v > 0.0) || !std::isfinite(v)) return STK_INVALID_PARAMS;     // (every gain 0: the frame has no variance to weigh by)
        V[i] = v;
    }
    if (ref < 0) return STK_INVALID_PARAMS;
    for (int32_t i = 0; i < n; i++) {
        if (include && !include[i]) { out[i] = 0.0f; continue; }
        const double u = user ? (double)user[i] : 1.0;
        out[i] = (float)(u * V[ref] / V[i]);
    }
    return STK_OK;
}

}  // namespace noise
}  // namespace stk
