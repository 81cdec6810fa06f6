// star_quality_harness.cpp — the host half of star measurement (libstacker_rs_amd/csrc/star_shape_host.h: the derived values,
// a frame's quality, the scores and the quality weights) over random and degenerate shapes: sums of either sign and of the
// largest magnitude the device can return, S = 0, npix = 0, every flag, frames with no star, with no measured star and
// filled to max_stars, every power, and each refusal. Every buffer is a heap block of exactly the documented size, so that a
// read or write one element outside it is an ASan report. A stand-alone program: built with ASan + UBSan by
// tests/test_cpu_star_measure.py and run as it is. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../../libstacker_rs_amd/csrc/star_shape_host.h"

using namespace stk::shape;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

template <typename T>
static T* block(size_t n) { return (T*)std::calloc(n ? n : 1, sizeof(T)); }

int main() {
    std::mt19937_64 rng(12345);
    auto uni = [&](int64_t lo, int64_t hi) { return (int64_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
    const int64_t BIG = 65535ll * 144 * 441;                               // the largest Sxx of a 12-pixel aperture

    // ---- derive: random, extreme and degenerate integers; it never reads or writes outside `count` shapes
    for (int count : {0, 1, 2, 37, 1024}) {
        stk_star_shape* s = block<stk_star_shape>((size_t)count);
        for (int i = 0; i < count; i++) {
            stk_star_shape& o = s[i];
            const int kind = i % 8;
            o.S = kind == 0 ? 0 : kind == 1 ? BIG : kind == 2 ? -uni(1, BIG) : uni(1, 65535 * 441);
            o.Sx = uni(-BIG, BIG); o.Sy = uni(-BIG, BIG); o.Sxx = uni(kind == 3 ? -BIG : 0, BIG); o.Syy = uni(0, BIG); o.Sxy = uni(-BIG, BIG);
            o.px = (int32_t)uni(-5, 70000); o.py = (int32_t)uni(-5, 70000); o.bg = (int32_t)uni(0, 65535); o.mad = (int32_t)uni(0, 65535);
            o.npix = kind == 4 ? 0 : (int32_t)uni(1, 441);
            o.flags = kind == 5 ? (int32_t)uni(1, 15) : kind == 6 ? 8 : 0;
            o.x = o.fwhm = std::nan("");                                      // stale doubles are overwritten
        }
        CHECK(derive(count ? s : nullptr, count) == STK_OK);
        for (int i = 0; i < count; i++) {
            const stk_star_shape& o = s[i];
            CHECK(!std::isnan(o.x) && !std::isnan(o.fwhm));
            if (o.flags != 0) CHECK(o.fwhm == 0.0 && o.ecc == 0.0 && o.snr == 0.0);
            else if (o.S != 0) CHECK(o.fwhm > 0.0 && o.ecc >= 0.0 && o.ecc <= 1.0);
        }
        CHECK(derive(s, count) == STK_OK);                                    // in place, a second time: the same values
        std::free(s);
    }
    CHECK(derive(nullptr, 1) == STK_INVALID_PARAMS);
    CHECK(derive(nullptr, -1) == STK_INVALID_PARAMS);
    {   // a round Gaussian-like blob by hand: cxx = cyy = 2, cxy = 0
        stk_star_shape* s = block<stk_star_shape>(1);
        s->S = 100; s->Sx = 50; s->Sy = -25; s->Sxx = 225; s->Syy = 206; s->Sxy = -12; s->px = 10; s->py = 20; s->mad = 10; s->npix = 25;
        CHECK(derive(s, 1) == STK_OK);
        CHECK(s->x == 10.5 && s->y == 19.75 && s->cxx == 2.0 && s->cyy == 2.06 - 0.0625 && s->flags == 0);
        CHECK(std::fabs(s->fwhm - FWHM_PER_SIGMA * std::sqrt((2.0 + 1.9975) / 2.0)) < 1e-12 && s->snr == 100.0 / ((1.4826 * 10.0) * 5.0));
        std::free(s);
    }

    // ---- frame_quality, quality_scores, quality_weights
    for (int n : {1, 2, 9}) {
        for (int cap : {1, 4, 33}) {
            stk_star_shape* s = block<stk_star_shape>((size_t)n * cap);
            int32_t* ns = block<int32_t>((size_t)n);
            stk_star_quality* q = block<stk_star_quality>((size_t)n);
            double* sc = block<double>((size_t)n * 4);
            float* w = block<float>((size_t)n);
            float* u = block<float>((size_t)n);
            int32_t* inc = block<int32_t>((size_t)n);
            int32_t* inc_out = block<int32_t>((size_t)n);
            for (int i = 0; i < n; i++) {
                ns[i] = i == 1 ? 0 : i == 2 ? cap : (int32_t)uni(0, cap);      // no star, a full list, anything between
                if (i == 0) ns[i] = cap;
                for (int k = 0; k < cap; k++) {
                    stk_star_shape& o = s[(size_t)i * cap + k];
                    o.S = uni(100, 100000); o.Sxx = o.S * uni(1, 9); o.Syy = o.S * uni(1, 9); o.Sxy = 0; o.npix = (int32_t)uni(5, 200);
                    o.mad = (int32_t)uni(0, 60); o.bg = (int32_t)uni(0, 65535);
                    o.flags = (i == 3 || (k % 5 == 4)) ? 4 : 0;                 // frame 3: stars, none measured
                }
                inc[i] = 1; u[i] = 1.0f + 0.25f * (float)i;
            }
            CHECK(derive(s, n * cap) == STK_OK);
            CHECK(frame_quality(s, ns, n, cap, q) == STK_OK);
            for (int i = 0; i < n; i++) {
                CHECK(q[i].n_stars == ns[i] && q[i].n_measured <= ns[i]);
                if (i == 1 || i == 3) CHECK(q[i].n_measured == 0 && q[i].fwhm == 0.0 && q[i].noise == 0.0);
                if (q[i].n_measured) CHECK(q[i].fwhm > 0.0 && q[i].snr > 0.0);
            }
            CHECK(quality_scores(q, n, sc) == STK_OK);
            for (int i = 0; i < n; i++) CHECK(sc[4 * i + 3] == (double)q[i].n_measured && (q[i].n_measured || sc[4 * i] == 0.0));
            for (int pw = 0; pw <= 4; pw++) {
                stk_star_quality_params p{0.0, 0.0, 1, pw, (pw + 1) % 5, (pw + 2) % 5, 0};
                int32_t rej = -1;
                CHECK(quality_weights(q, n, &p, 0, inc, u, w, inc_out, &rej) == STK_OK);
                CHECK(inc_out[0] == 1 && rej >= 0 && rej < n);
                for (int i = 0; i < n; i++) CHECK(std::isfinite(w[i]) && w[i] >= 0.0f && (inc_out[i] || w[i] == 0.0f) && w[i] <= u[i]);
                CHECK(quality_weights(q, n, &p, -1, nullptr, nullptr, w, nullptr, nullptr) == STK_OK);
            }
            stk_star_quality_params p{0.0, 0.0, 1, 2, 0, 0, 0};
            if (n > 1) {
                CHECK(quality_weights(q, n, &p, 1, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);   // a reference without a measured star
                inc[0] = 0;
                CHECK(quality_weights(q, n, &p, 0, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);   // a reference that is not included
                inc[0] = 1;
            }
            p.fwhm_max = 1e-9;                                                 // nothing passes ... but the reference
            CHECK(quality_weights(q, n, &p, -1, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);
            CHECK(quality_weights(q, n, &p, 0, inc, u, w, inc_out, nullptr) == STK_OK && w[0] == u[0]);
            p.fwhm_max = 0.0;
            CHECK(quality_weights(q, n, &p, n, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);
            CHECK(quality_weights(q, n, &p, -2, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);
            CHECK(quality_weights(q, 0, &p, -1, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);
            CHECK(quality_weights(nullptr, n, &p, -1, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);
            CHECK(quality_weights(q, n, nullptr, -1, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);
            CHECK(quality_weights(q, n, &p, -1, inc, u, nullptr, inc_out, nullptr) == STK_INVALID_PARAMS);
            for (int bad = 0; bad < 7; bad++) {
                stk_star_quality_params b = p;
                if (bad == 0) b.fwhm_power = 5; else if (bad == 1) b.ecc_power = -1; else if (bad == 2) b.snr_power = 5;
                else if (bad == 3) b.min_measured = 0; else if (bad == 4) b.reserved = 1; else if (bad == 5) b.fwhm_max = std::nan("");
                else b.ecc_max = -0.5;
                CHECK(quality_weights(q, n, &b, -1, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);
            }
            u[n - 1] = -1.0f;
            CHECK(quality_weights(q, n, &p, -1, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);
            u[n - 1] = std::numeric_limits<float>::infinity();
            CHECK(quality_weights(q, n, &p, -1, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);
            u[n - 1] = 1.0f;
            const double keep = q[n - 1].snr;
            q[n - 1].snr = std::numeric_limits<double>::infinity();
            CHECK(quality_weights(q, n, &p, -1, inc, u, w, inc_out, nullptr) == STK_INVALID_PARAMS);
            q[n - 1].snr = keep;
            ns[0] = cap + 1;
            CHECK(frame_quality(s, ns, n, cap, q) == STK_INVALID_PARAMS);
            ns[0] = -1;
            CHECK(frame_quality(s, ns, n, cap, q) == STK_INVALID_PARAMS);
            ns[0] = cap;
            CHECK(frame_quality(s, ns, 0, cap, q) == STK_INVALID_PARAMS);
            CHECK(frame_quality(s, ns, n, 0, q) == STK_INVALID_PARAMS);
            CHECK(frame_quality(nullptr, ns, n, cap, q) == STK_INVALID_PARAMS);
            CHECK(frame_quality(s, nullptr, n, cap, q) == STK_INVALID_PARAMS);
            CHECK(frame_quality(s, ns, n, cap, nullptr) == STK_INVALID_PARAMS);
            CHECK(quality_scores(nullptr, n, sc) == STK_INVALID_PARAMS);
            CHECK(quality_scores(q, n, nullptr) == STK_INVALID_PARAMS);
            CHECK(quality_scores(q, 0, sc) == STK_INVALID_PARAMS);
            std::free(s); std::free(ns); std::free(q); std::free(sc); std::free(w); std::free(u); std::free(inc); std::free(inc_out);
        }
    }

    // ---- the measure parameters' checks
    {
        const stk_star_measure_params ok{7, 10, 14, 3.0f, 1, 5, 0, 0};
        CHECK(validate(&ok) == nullptr);
        CHECK(validate((const stk_star_measure_params*)nullptr) != nullptr);
        stk_star_measure_params b = ok;
        b.radius = 1; CHECK(validate(&b)); b.radius = 13; CHECK(validate(&b)); b = ok;
        b.ring_inner = 7; CHECK(validate(&b)); b.ring_inner = 16; b.ring_outer = 16; CHECK(validate(&b)); b = ok;
        b.ring_outer = 9; CHECK(validate(&b)); b.ring_outer = 17; CHECK(validate(&b)); b = ok;
        b.kappa = -1.0f; CHECK(validate(&b)); b.kappa = std::nanf(""); CHECK(validate(&b)); b = ok;
        b.min_contrast = 0; CHECK(validate(&b)); b.min_contrast = 65536; CHECK(validate(&b)); b = ok;
        b.min_pixels = 0; CHECK(validate(&b)); b = ok;
        b.saturation = -1; CHECK(validate(&b)); b.saturation = 65536; CHECK(validate(&b)); b = ok;
        b.reserved = 1; CHECK(validate(&b));
        const stk_star_measure_params lo{2, 3, 3, 0.0f, 65535, 1, 65535, 0}, hi{12, 13, 16, 100.0f, 1, 1000, 1, 0};
        CHECK(validate(&lo) == nullptr && validate(&hi) == nullptr);
    }
    std::printf("ok\n");
    return 0;
}
