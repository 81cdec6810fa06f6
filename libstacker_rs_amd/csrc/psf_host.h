// psf_host.h — the host half of deconvolution (include/stacker.h, "deconvolution"): the parameter and PSF checks, the PSF
// model from a covariance and the covariance of a frame's star shapes. Inline, no HIP type and no stk_ctx, so that a
// host-only program can call them (tests/sanitize/psf_harness.cpp); deconvolve.cpp exports them as stk_psf_model and
// stk_psf_from_shapes. f64, each operation rounded on its own (-ffp-contract=off); exp, pow and log are libm's, the
// functions Python's math module calls, so that tests/deconvolve_restate.py matches bit for bit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/stacker.h"

namespace stk {
namespace psf {

constexpr int MAX_RADIUS = 16;

inline bool positive_definite(double cxx, double cyy, double cxy) {
    if (!std::isfinite(cxx) || !std::isfinite(cyy) || !std::isfinite(cxy)) return false;
    const double det = cxx * cyy - cxy * cxy;
    return cxx > 0.0 && cyy > 0.0 && std::isfinite(det) && det > 0.0;
}

// null when the parameters are in range for a w x h image, else what is wrong with them
inline const char* validate(const stk_deconv_params* p, int w, int h) {
    if (!p) return "null deconvolution parameters";
    if (p->iterations < 1 || p->iterations > 1000) return "deconvolve: iterations must be 1 .. 1000";
    if (p->radius < 1 || p->radius > MAX_RADIUS) return "deconvolve: radius must be 1 .. 16";
    if (w < p->radius + 1 || h < p->radius + 1) return "deconvolve: width and height must be at least radius + 1";
    if (!std::isfinite(p->floor) || !(p->floor > 0.0f)) return "deconvolve: floor must be finite and > 0";
    if (!std::isfinite(p->pedestal)) return "deconvolve: pedestal must be finite";
    if (!std::isfinite(p->lambda) || !(p->lambda >= 0.0f)) return "deconvolve: lambda must be finite and >= 0";
    if (!std::isfinite(p->tv_eps) || !(p->tv_eps > 0.0f)) return "deconvolve: tv_eps must be finite and > 0";
    if (!(p->amount >= 0.0f && p->amount <= 1.0f)) return "deconvolve: amount must be 0 .. 1";
    if (p->reserved != 0) return "deconvolution parameters: reserved must be 0";
    return nullptr;
}

// every tap finite and >= 0, the f64 sum in row-major order within 1e-3 of 1
inline const char* validate_taps(const float* taps, int radius) {
    if (!taps) return "deconvolve: null PSF";
    const int n = (2 * radius + 1) * (2 * radius + 1);
    double sum = 0.0;
    for (int k = 0; k < n; k++) {
        if (!std::isfinite(taps[k]) || taps[k] < 0.0f) return "deconvolve: every PSF tap must be finite and >= 0";
        sum += (double)taps[k];
    }
    if (!(std::fabs(sum - 1.0) <= 1e-3)) return "deconvolve: the PSF must sum to 1 within 1e-3";
    return nullptr;
}

inline stk_status model(int kind, double beta, int radius, double cxx, double cyy, double cxy, float* out) {
    if (!out || radius < 1 || radius > MAX_RADIUS || (kind != STK_PSF_GAUSSIAN && kind != STK_PSF_MOFFAT)) return STK_INVALID_PARAMS;
    if (!positive_definite(cxx, cyy, cxy)) return STK_INVALID_PARAMS;
    if (kind == STK_PSF_MOFFAT && (!std::isfinite(beta) || !(beta > 1.0))) return STK_INVALID_PARAMS;
    const double det = cxx * cyy - cxy * cxy;
    const double g = kind == STK_PSF_MOFFAT ? (std::pow(2.0, 1.0 / beta) - 1.0) / (2.0 * std::log(2.0)) : 0.0;
    const int side = 2 * radius + 1;
    std::vector<double> v((size_t)side * side);
    double sum = 0.0;
    for (int j = -radius; j <= radius; j++)
        for (int i = -radius; i <= radius; i++) {
            const double x = (double)i, y = (double)j;
            const double q = ((cyy * x) * x - ((2.0 * cxy) * x) * y + (cxx * y) * y) / det;
            const double f = kind == STK_PSF_MOFFAT ? std::pow(1.0 + q * g, -beta) : std::exp(-q / 2.0);
            v[(size_t)(j + radius) * side + (i + radius)] = f;
            sum += f;
        }
    if (!std::isfinite(sum) || !(sum > 0.0)) return STK_INVALID_PARAMS;
    for (size_t k = 0; k < v.size(); k++) out[k] = (float)(v[k] / sum);
    return STK_OK;
}

inline stk_status from_shapes(const stk_star_shape* shapes, int count, double min_snr, double scale, double* cxx, double* cyy,
                              double* cxy, int32_t* used) {
    if (used) *used = 0;
    if (count < 0 || (count > 0 && !shapes) || !cxx || !cyy || !cxy) return STK_INVALID_PARAMS;
    if (!std::isfinite(min_snr) || !std::isfinite(scale) || !(scale > 0.0)) return STK_INVALID_PARAMS;
    std::vector<double> a, b, c;
    for (int k = 0; k < count; k++) {
        const stk_star_shape& s = shapes[k];
        if (s.flags != 0 || !(s.snr >= min_snr)) continue;
        if (!std::isfinite(s.cxx) || !std::isfinite(s.cyy) || !std::isfinite(s.cxy)) return STK_INVALID_PARAMS;   // (no order among NaNs)
        a.push_back(s.cxx); b.push_back(s.cyy); c.push_back(s.cxy);
    }
    const size_t m = a.size();
    if (used) *used = (int32_t)m;
    if (m == 0) return STK_INVALID_PARAMS;
    const size_t kth = (m + 1) / 2 - 1;
    const double s2 = scale * scale;
    double r[3];
    std::vector<double>* col[3] = {&a, &b, &c};
    for (int t = 0; t < 3; t++) {
        std::nth_element(col[t]->begin(), col[t]->begin() + kth, col[t]->end());
        r[t] = (*col[t])[kth] * s2;
    }
    if (!positive_definite(r[0], r[1], r[2])) return STK_INVALID_PARAMS;
    *cxx = r[0]; *cyy = r[1]; *cxy = r[2];
    return STK_OK;
}

}  // namespace psf
}  // namespace stk
