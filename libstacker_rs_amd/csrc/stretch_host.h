// stretch_host.h — the host half of the display stretch (include/stacker.h, "display stretch"): the parameter checks, the
// ranks of the statistics, the auto rule and the table builder. Inline, no HIP type and no stk_ctx, so that a host-only
// program can call them (tests/sanitize/stretch_harness.cpp); stretch.cpp exports the rule and the builder as
// stk_stretch_auto and stk_stretch_table. f64, each operation rounded on its own (-ffp-contract=off).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/stacker.h"

namespace stk {
namespace stretch {

constexpr int MAX_QUANTILES = 4, MAX_KNOTS = 65536;

inline stk_stretch_auto_params auto_defaults() {
    stk_stretch_auto_params a{};
    a.shadows_clip = -2.8; a.target_background = 0.25; a.white = 1.0; a.white_quantile = 0.999;
    return a;
}

// null when the quantiles may be asked for, else what is wrong with them
inline const char* validate_quantiles(const double* q, int n) {
    if (n < 0 || n > MAX_QUANTILES) return "image statistics: at most four quantiles";
    if (n && !q) return "image statistics: null quantiles";
    for (int i = 0; i < n; i++)
        if (!std::isfinite(q[i]) || !(q[i] >= 0.0 && q[i] <= 1.0)) return "image statistics: every quantile must be finite and 0 .. 1";
    return nullptr;
}

// the rank (from 1) of the quantile p among N >= 1 samples
inline int64_t quantile_rank(double p, int64_t N) {
    const int64_t k = (int64_t)std::ceil(p * (double)N);
    return k < 1 ? 1 : k > N ? N : k;
}

// null when the parameters are in range for an image of `channels` channels, else what is wrong with them; `table`: knots + 1
// floats, read under STK_STRETCH_TABLE
inline const char* validate(const stk_stretch_params* p, int channels, const float* table, int knots) {
    if (!p) return "null stretch parameters";
    if (channels != 1 && channels != 3 && channels != 4) return "stretch: 1, 3 or 4 channels";
    if (p->curve != STK_STRETCH_LINEAR && p->curve != STK_STRETCH_MTF && p->curve != STK_STRETCH_TABLE) return "stretch: unknown curve";
    if (p->colour != 0 && p->colour != 1) return "stretch: colour must be 0 or 1";
    if (p->out_depth != STK_DEPTH_U8 && p->out_depth != STK_DEPTH_U16 && p->out_depth != STK_DEPTH_F32) return "stretch: unknown out_depth";
    if (p->reserved != 0) return "stretch parameters: reserved must be 0";
    if (!std::isfinite(p->out_scale)) return "stretch: out_scale must be finite";
    const int cc = channels < 3 ? channels : 3;
    for (int c = 0; c < cc; c++) {
        if (!std::isfinite(p->black[c]) || !std::isfinite(p->white[c]) || !(p->white[c] > p->black[c])) return "stretch: black and white must be finite with white > black";
        if (p->curve == STK_STRETCH_MTF && !(p->midtone[c] > 0.0f && p->midtone[c] < 1.0f)) return "stretch: every midtone must be in (0, 1)";
    }
    if (p->curve == STK_STRETCH_TABLE) {
        if (knots < 2 || knots > MAX_KNOTS) return "stretch: knots must be 2 .. 65536";
        if (!table) return "stretch: null table";
        for (int k = 0; k <= knots; k++)
            if (!(table[k] >= 0.0f && table[k] <= 1.0f)) return "stretch: every table value must be finite and 0 .. 1";
    }
    return nullptr;
}

inline const char* validate_auto(const stk_stretch_auto_params* a) {
    if (!a) return "null auto-stretch parameters";
    if (!(a->shadows_clip <= 0.0) || !std::isfinite(a->shadows_clip)) return "auto stretch: shadows_clip must be finite and <= 0";
    if (!(a->target_background > 0.0 && a->target_background < 1.0)) return "auto stretch: target_background must be in (0, 1)";
    if (!std::isfinite(a->white)) return "auto stretch: white must be finite";
    if (!(a->white_quantile >= 0.0 && a->white_quantile <= 1.0)) return "auto stretch: white_quantile must be 0 .. 1";
    if (a->linked != 0 && a->linked != 1) return "auto stretch: linked must be 0 or 1";
    if (a->white_mode < 0 || a->white_mode > 2) return "auto stretch: white_mode must be 0 .. 2";
    return nullptr;
}

// mtf(t, x) = ((t - 1) x) / ((2 t - 1) x - t)
inline double mtf(double t, double x) { return ((t - 1.0) * x) / ((2.0 * t - 1.0) * x - t); }

// the rule of one channel from (median, mad, min, w)
inline void rule(const stk_stretch_auto_params& a, double median, double mad, double mn, double w, float* black, float* white, float* midtone) {
    const double lo = median + (a.shadows_clip * 1.4826) * mad;
    const double c0 = mn > lo ? mn : lo;
    if (w <= c0) w = c0 + 1.0;
    const double x0 = (median - c0) / (w - c0);
    double m = 0.5;
    if (x0 != 0.0) {
        m = mtf(a.target_background, x0);
        m = m < 1e-6 ? 1e-6 : m > 1.0 - 1e-6 ? 1.0 - 1e-6 : m;
    }
    *black = (float)c0; *white = (float)w; *midtone = (float)m;
}

inline stk_status auto_params(const stk_image_stat* stats, int channels, const stk_stretch_auto_params* params_or_null, stk_stretch_params* out) {
    if (!stats || !out || (channels != 1 && channels != 3 && channels != 4)) return STK_INVALID_PARAMS;
    const stk_stretch_auto_params a = params_or_null ? *params_or_null : auto_defaults();
    if (validate_auto(&a)) return STK_INVALID_PARAMS;
    const int cc = channels < 3 ? channels : 3;
    double w[3] = {};
    for (int c = 0; c < cc; c++) {
        const stk_image_stat& s = stats[c];
        if (s.count < 0 || !std::isfinite(s.min) || !std::isfinite(s.max) || !std::isfinite(s.median) || !std::isfinite(s.mad) || !std::isfinite(s.q[0]))
            return STK_INVALID_PARAMS;
        w[c] = a.white_mode == 0 ? a.white : a.white_mode == 1 ? (double)s.max : (double)s.q[0];
    }
    stk_stretch_params p{};
    p.curve = STK_STRETCH_MTF; p.out_depth = STK_DEPTH_F32; p.out_scale = 1.0f;
    for (int c = 0; c < 4; c++) { p.black[c] = 0.0f; p.white[c] = 1.0f; p.midtone[c] = 0.5f; }
    if (a.linked) {
        double median = 0.0, mad = 0.0, mn = 0.0, ww = 0.0;
        for (int c = 0; c < cc; c++) { median += (double)stats[c].median; mad += (double)stats[c].mad; mn += (double)stats[c].min; ww += w[c]; }
        median /= (double)cc; mad /= (double)cc; mn /= (double)cc; ww /= (double)cc;
        for (int c = 0; c < cc; c++) rule(a, median, mad, mn, ww, &p.black[c], &p.white[c], &p.midtone[c]);
    } else {
        for (int c = 0; c < cc; c++) rule(a, (double)stats[c].median, (double)stats[c].mad, (double)stats[c].min, w[c], &p.black[c], &p.white[c], &p.midtone[c]);
    }
    *out = p;
    return STK_OK;
}

inline stk_status table(int kind, double param, int knots, float* t) {
    if (!t || knots < 2 || knots > MAX_KNOTS) return STK_INVALID_PARAMS;
    if (kind != STK_CURVE_ASINH && kind != STK_CURVE_GAMMA && kind != STK_CURVE_SRGB) return STK_INVALID_PARAMS;
    if (kind != STK_CURVE_SRGB && (!std::isfinite(param) || !(param > 0.0))) return STK_INVALID_PARAMS;
    const double K = (double)knots;
    const double norm = kind == STK_CURVE_ASINH ? std::asinh(param) : 0.0, inv = kind == STK_CURVE_GAMMA ? 1.0 / param : 1.0 / 2.4;
    for (int k = 1; k < knots; k++) {
        const double x = (double)k / K;
        double v;
        if (kind == STK_CURVE_ASINH) v = std::asinh(param * x) / norm;
        else if (kind == STK_CURVE_GAMMA) v = std::pow(x, inv);
        else v = x <= 0.0031308 ? 12.92 * x : 1.055 * std::pow(x, inv) - 0.055;
        const float f = (float)v;
        t[k] = f < 0.0f ? 0.0f : f > 1.0f ? 1.0f : f;
    }
    t[0] = 0.0f; t[knots] = 1.0f;
    return STK_OK;
}

// ---- the keys of the selection (the device computes the same; the host decodes what it reads back) ----------------------
// order-preserving: negative values have every bit flipped, the others the sign bit set
inline uint32_t key_of_bits(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
inline float value_of_key(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

}  // namespace stretch
}  // namespace stk
