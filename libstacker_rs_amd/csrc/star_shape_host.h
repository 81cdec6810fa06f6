// star_shape_host.h — the host half of star measurement (include/stacker.h, stk_star_measure_params): the parameter checks,
// the derived values of a shape, a frame's quality, the scores and the quality weights. Inline, no HIP type and no stk_ctx, so
// that a host-only program can call them (tests/sanitize/star_quality_harness.cpp); star_measure.cpp exports them as
// stk_star_shape_derive, stk_star_frame_quality, stk_star_quality_scores and stk_star_quality_weights. f64 throughout, each
// operation rounded on its own (-ffp-contract=off): only + - x / and sqrt, so that a numpy restatement matches bit for bit.
//
// What the values are. Isophotal moments, as SExtractor's are: sums over the aperture's pixels at or above bg + thr. The FWHM
// of a Gaussian comes out a few per cent low, because the threshold cuts the wings; noise gives round stars an ecc floor of
// 0.2 - 0.35. The values compare frames with each other. They do not fit PSFs.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/stacker.h"

namespace stk {
namespace shape {

constexpr double FWHM_PER_SIGMA = 2.3548200450309493;      // 2 sqrt(2 ln 2)

// null when the parameters are in range, else what is wrong with them
inline const char* validate(const stk_star_measure_params* p) {
    if (!p) return "null star measure parameters";
    if (p->radius < 2 || p->radius > 12) return "star measure: radius must be 2 .. 12";
    if (p->ring_inner <= p->radius || p->ring_inner > 15) return "star measure: ring_inner must be radius + 1 .. 15";
    if (p->ring_outer < p->ring_inner || p->ring_outer > 16) return "star measure: ring_outer must be ring_inner .. 16";
    if (!std::isfinite(p->kappa) || p->kappa < 0.0f) return "star measure: kappa must be finite and >= 0";
    if (p->min_contrast < 1 || p->min_contrast > 65535) return "star measure: min_contrast must be 1 .. 65535";
    if (p->min_pixels < 1) return "star measure: min_pixels must be >= 1";
    if (p->saturation < 0 || p->saturation > 65535) return "star measure: saturation must be 0 or 1 .. 65535";
    if (p->reserved != 0) return "star measure: reserved must be 0";
    return nullptr;
}

inline const char* validate(const stk_star_quality_params* p) {
    if (!p) return "null star quality parameters";
    if (!std::isfinite(p->fwhm_max) || p->fwhm_max < 0.0) return "star quality: fwhm_max must be finite and >= 0";
    if (!std::isfinite(p->ecc_max) || p->ecc_max < 0.0) return "star quality: ecc_max must be finite and >= 0";
    if (p->min_measured < 1) return "star quality: min_measured must be >= 1";
    if (p->fwhm_power < 0 || p->fwhm_power > 4 || p->ecc_power < 0 || p->ecc_power > 4 || p->snr_power < 0 || p->snr_power > 4)
        return "star quality: the powers must be 0 .. 4";
    if (p->reserved != 0) return "star quality: reserved must be 0";
    return nullptr;
}

inline stk_status derive(stk_star_shape* s, int32_t count) {
    if (count < 0 || (count > 0 && !s)) return STK_INVALID_PARAMS;
    for (int32_t i = 0; i < count; i++) {
        stk_star_shape& o = s[i];
        o.x = o.y = o.cxx = o.cyy = o.cxy = o.fwhm = o.ecc = o.snr = 0.0;
        o.flags &= ~8;
        if (o.flags != 0 || o.S == 0) continue;                           // (S == 0 is flags bit 2 in a measured shape)
        const double S = (double)o.S;
        const double mx = (double)o.Sx / S, my = (double)o.Sy / S;
        o.x = (double)o.px + mx; o.y = (double)o.py + my;
        o.cxx = (double)o.Sxx / S - mx * mx;
        o.cyy = (double)o.Syy / S - my * my;
        o.cxy = (double)o.Sxy / S - mx * my;
        const double tr = o.cxx + o.cyy, dd = o.cxx - o.cyy;
        const double df = std::sqrt(dd * dd + 4.0 * (o.cxy * o.cxy));
        const double l1 = (tr + df) / 2.0, l2 = (tr - df) / 2.0;
        if (!(l2 > 0.0)) { o.flags |= 8; continue; }
        o.fwhm = FWHM_PER_SIGMA * std::sqrt(tr / 2.0);
        o.ecc = std::sqrt(std::max(1.0 - l2 / l1, 0.0));
        o.snr = S / (std::max(1.4826 * (double)o.mad, 0.5) * std::sqrt((double)o.npix));
    }
    return STK_OK;
}

// the lower median: the ((m + 1) / 2)-th smallest of v (m >= 1); v is reordered
inline double lower_median(std::vector<double>& v) {
    const size_t k = (v.size() + 1) / 2 - 1;
    std::nth_element(v.begin(), v.begin() + (std::ptrdiff_t)k, v.end());
    return v[k];
}

inline stk_status frame_quality(const stk_star_shape* shapes, const int32_t* n_stars, int32_t n, int32_t max_stars, stk_star_quality* out) {
    if (!shapes || !n_stars || !out || n < 1 || max_stars < 1) return STK_INVALID_PARAMS;
    for (int32_t i = 0; i < n; i++)
        if (n_stars[i] < 0 || n_stars[i] > max_stars) return STK_INVALID_PARAMS;
    std::vector<double> v[5];
    for (int32_t i = 0; i < n; i++) {
        stk_star_quality& q = out[i];
        std::memset(&q, 0, sizeof(q));
        q.n_stars = n_stars[i];
        for (auto& c : v) c.clear();
        const stk_star_shape* s = shapes + (size_t)i * max_stars;
        for (int32_t k = 0; k < n_stars[i]; k++) {
            if (s[k].flags != 0) continue;
            v[0].push_back(s[k].fwhm); v[1].push_back(s[k].ecc); v[2].push_back(s[k].snr);
            v[3].push_back((double)s[k].bg); v[4].push_back(1.4826 * (double)s[k].mad);
        }
        q.n_measured = (int32_t)v[0].size();
        if (!q.n_measured) continue;
        q.fwhm = lower_median(v[0]); q.ecc = lower_median(v[1]); q.snr = lower_median(v[2]);
        q.bg = lower_median(v[3]); q.noise = lower_median(v[4]);
    }
    return STK_OK;
}

inline stk_status quality_scores(const stk_star_quality* q, int32_t n, double* scores) {
    if (!q || !scores || n < 1) return STK_INVALID_PARAMS;
    for (int32_t i = 0; i < n; i++) {
        const bool m = q[i].n_measured > 0;
        double* o = scores + (size_t)i * 4;
        o[STK_STAR_SCORE_FWHM] = m ? 1.0 / q[i].fwhm : 0.0;
        o[STK_STAR_SCORE_ROUND] = m ? 1.0 - q[i].ecc : 0.0;
        o[STK_STAR_SCORE_SNR] = q[i].snr;
        o[STK_STAR_SCORE_COUNT] = (double)q[i].n_measured;
    }
    return STK_OK;
}

inline stk_status quality_weights(const stk_star_quality* q, int32_t n, const stk_star_quality_params* p, int32_t reference,
                                  const int32_t* include, const float* user, float* weights_out, int32_t* include_out, int32_t* rejected) {
    if (!q || !weights_out || n < 1 || validate(p)) return STK_INVALID_PARAMS;
    if (reference < -1 || reference >= n) return STK_INVALID_PARAMS;
    if (reference >= 0 && ((include && !include[reference]) || q[reference].n_measured <= 0)) return STK_INVALID_PARAMS;
    for (int32_t i = 0; i < n; i++) {
        if (user && (!std::isfinite(user[i]) || user[i] < 0.0f)) return STK_INVALID_PARAMS;
        if (!std::isfinite(q[i].fwhm) || !std::isfinite(q[i].ecc) || !std::isfinite(q[i].snr) || q[i].fwhm < 0.0 || q[i].ecc < 0.0 || q[i].snr < 0.0)
            return STK_INVALID_PARAMS;
    }
    std::vector<char> pass((size_t)n, 0);
    int32_t n_pass = 0, n_rej = 0;
    double F = 0.0, E = 0.0, Z = 0.0;
    for (int32_t i = 0; i < n; i++) {
        if (include && !include[i]) continue;
        bool ok = q[i].n_measured >= p->min_measured && (p->fwhm_max == 0.0 || q[i].fwhm <= p->fwhm_max) &&
                  (p->ecc_max == 0.0 || q[i].ecc <= p->ecc_max);
        if (i == reference) ok = true;
        if (!ok) { n_rej++; continue; }
        pass[i] = 1;
        const double r = 1.0 - q[i].ecc;
        F = n_pass ? std::min(F, q[i].fwhm) : q[i].fwhm;
        E = n_pass ? std::max(E, r) : r;
        Z = n_pass ? std::max(Z, q[i].snr) : q[i].snr;
        n_pass++;
    }
    if (!n_pass) return STK_INVALID_PARAMS;
    for (int32_t i = 0; i < n; i++) {
        if (include_out) include_out[i] = pass[i];
        if (!pass[i]) { weights_out[i] = 0.0f; continue; }
        double w = user ? (double)user[i] : 1.0;
        const double ff = q[i].fwhm == 0.0 ? 1.0 : F / q[i].fwhm;
        const double fe = E == 0.0 ? 1.0 : (1.0 - q[i].ecc) / E;
        const double fz = Z == 0.0 ? 1.0 : q[i].snr / Z;
        for (int k = 0; k < p->fwhm_power; k++) w = w * ff;
        for (int k = 0; k < p->ecc_power; k++) w = w * fe;
        for (int k = 0; k < p->snr_power; k++) w = w * fz;
        weights_out[i] = (float)w;
    }
    if (rejected) *rejected = n_rej;
    return STK_OK;
}

}  // namespace shape
}  // namespace stk
