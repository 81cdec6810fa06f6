// wavelet_host.h — the host half of the wavelet layers (include/stacker.h, "wavelet layers"): the parameter checks, the
// noise table of the filter, sigma from the first layer's median and the thresholds. Inline, no HIP type and no stk_ctx, so
// that a host-only program can call them (tests/sanitize/wavelet_harness.cpp); wavelet.cpp exports the table as
// stk_wavelet_noise_table. f64, each operation rounded on its own (-ffp-contract=off).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/stacker.h"

namespace stk {
namespace wavelet {

constexpr int MAX_LEVELS = 8;

// null when the parameters are in range for a w x h image, else what is wrong with them
inline const char* validate(const stk_wavelet_params* p, int w, int h) {
    if (!p) return "null wavelet parameters";
    if (p->levels < 1 || p->levels > MAX_LEVELS) return "wavelet: levels must be 1 .. 8";
    if (w < (1 << p->levels) + 1 || h < (1 << p->levels) + 1) return "wavelet: width and height must be at least 2^levels + 1";
    if (p->mode != STK_WAVELET_HARD && p->mode != STK_WAVELET_SOFT) return "wavelet: unknown mode";
    if (p->reserved != 0) return "wavelet parameters: reserved must be 0";
    for (int j = 0; j < MAX_LEVELS; j++) {
        if (!std::isfinite(p->gain[j])) return "wavelet: every gain must be finite";
        if (!std::isfinite(p->threshold[j]) || !(p->threshold[j] >= 0.0f)) return "wavelet: every threshold must be finite and >= 0";
        if (!(p->layer_amount[j] >= 0.0f && p->layer_amount[j] <= 1.0f)) return "wavelet: every layer_amount must be 0 .. 1";
    }
    if (!std::isfinite(p->residual_gain)) return "wavelet: residual_gain must be finite";
    if (!(p->amount >= 0.0f && p->amount <= 1.0f)) return "wavelet: amount must be 0 .. 1";
    if (p->sigma_given)
        for (int c = 0; c < 4; c++)
            if (!std::isfinite(p->sigma[c]) || !(p->sigma[c] >= 0.0f)) return "wavelet: every given sigma must be finite and >= 0";
    return nullptr;
}

// true where the thresholds need a sigma that the caller did not give
inline bool needs_estimate(const stk_wavelet_params* p) {
    if (p->sigma_given) return false;
    for (int j = 0; j < p->levels; j++)
        if (p->threshold[j] > 0.0f) return true;
    return false;
}

// e_0 .. e_{levels-1}: the standard deviation of layer j of unit white noise, from the filter itself. a_j is the 1-D impulse
// response of the cascade up to c_j: a_0 = the unit impulse, a_{j+1} = a_j convolved with the B3 spline at spacing 2^j. The
// 2-D responses are separable, so e_j^2 = |a_j x a_j - a_{j+1} x a_{j+1}|^2 = (sum a_j^2)^2 - 2 (sum a_j a_{j+1})^2 + (sum a_{j+1}^2)^2.
inline stk_status noise_table(int levels, double* e) {
    if (!e || levels < 1 || levels > MAX_LEVELS) return STK_INVALID_PARAMS;
    static const double B3[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    const int half = 2 * ((1 << levels) - 1);                             // the reach of a_levels: 2 (2^J - 1)
    const int n = 2 * half + 1;
    std::vector<double> a((size_t)n, 0.0), b((size_t)n, 0.0);
    a[(size_t)half] = 1.0;
    for (int j = 0; j < levels; j++) {
        const int s = 1 << j;
        for (int i = 0; i < n; i++) {
            double v = 0.0;
            for (int k = -2; k <= 2; k++) {
                const int at = i - k * s;
                if (at >= 0 && at < n) v += B3[k + 2] * a[(size_t)at];
            }
            b[(size_t)i] = v;
        }
        double aa = 0.0, ab = 0.0, bb = 0.0;
        for (int i = 0; i < n; i++) {
            aa += a[(size_t)i] * a[(size_t)i];
            ab += a[(size_t)i] * b[(size_t)i];
            bb += b[(size_t)i] * b[(size_t)i];
        }
        e[j] = std::sqrt(aa * aa - 2.0 * (ab * ab) + bb * bb);
        a.swap(b);
    }
    return STK_OK;
}

// sigma of a channel from the lower median of |w_0|
inline float sigma_from_median(float median, double e0) { return (float)(1.4826 * (double)median / e0); }

// t_j = (float)(threshold_j sigma e_j), j < levels; the entries from `levels` on are 0
inline void thresholds(const stk_wavelet_params* p, float sigma, const double* e, float* t) {
    for (int j = 0; j < MAX_LEVELS; j++) t[j] = j < p->levels ? (float)((double)p->threshold[j] * (double)sigma * e[j]) : 0.0f;
}

}  // namespace wavelet
}  // namespace stk
