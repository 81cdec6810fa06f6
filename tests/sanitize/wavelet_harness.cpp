// wavelet_harness.cpp — the host half of the wavelet layers (libstacker_rs_amd/csrc/wavelet_host.h: the parameter checks,
// the noise table, sigma and the thresholds) over its edges: every level count, the smallest image of each, every refusal
// with bad, NaN and infinite arguments. Every buffer is a heap block of exactly the documented size, so that a read or write
// one element outside it is an ASan report. A stand-alone program: built with ASan + UBSan by tests/test_cpu_wavelet.py
// and run as it is. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../../libstacker_rs_amd/csrc/wavelet_host.h"

using namespace stk::wavelet;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

template <typename T>
static T* block(size_t n) { return (T*)std::calloc(n ? n : 1, sizeof(T)); }

static stk_wavelet_params* params() {
    stk_wavelet_params* p = block<stk_wavelet_params>(1);
    p->levels = 4; p->mode = STK_WAVELET_HARD;
    for (int j = 0; j < 8; j++) { p->gain[j] = 1.0f; p->threshold[j] = 0.0f; p->layer_amount[j] = 1.0f; }
    p->residual_gain = 1.0f; p->amount = 1.0f;
    return p;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    static const double E[8] = {0.8907963103, 0.2006638510, 0.0855075048, 0.0412174444, 0.0204249666, 0.0101897592, 0.0050920467, 0.0025456695};
    // ---- the table: every level count into a block of exactly that many doubles
    for (int levels = 1; levels <= 8; levels++) {
        double* e = block<double>((size_t)levels);
        CHECK(noise_table(levels, e) == STK_OK);
        for (int j = 0; j < levels; j++) CHECK(std::fabs(e[j] - E[j]) < 1e-9);
        for (int j = 1; j < levels; j++) CHECK(e[j] < e[j - 1] && e[j] > 0.0);
        std::free(e);
    }
    {
        double* e = block<double>(8);
        for (int levels : {0, -1, 9, 1 << 30, -(1 << 30)}) CHECK(noise_table(levels, e) == STK_INVALID_PARAMS);
        CHECK(noise_table(4, nullptr) == STK_INVALID_PARAMS);
        std::free(e);
    }
    // ---- validation: the defaults, the smallest image of every level count, one below it
    {
        stk_wavelet_params* p = params();
        CHECK(validate(nullptr, 100, 100) != nullptr);
        CHECK(validate(p, 17, 17) == nullptr);
        for (int levels = 1; levels <= 8; levels++) {
            p->levels = levels;
            const int n = (1 << levels) + 1;
            CHECK(validate(p, n, n) == nullptr && validate(p, n - 1, n) != nullptr && validate(p, n, n - 1) != nullptr);
        }
        for (int levels : {0, -1, 9, 31, 32, 1 << 30}) { p->levels = levels; CHECK(validate(p, 1 << 20, 1 << 20) != nullptr); }
        std::free(p);
    }
    // ---- validation: every field, with values out of range, NaN and infinite
    for (int j = 0; j < 8; j++) {
        for (float bad : {nan, inf, -inf}) {
            stk_wavelet_params* p = params();
            p->gain[j] = bad;
            CHECK(validate(p, 100, 100) != nullptr);
            std::free(p);
        }
        for (float bad : {nan, inf, -1e-6f, -inf}) {
            stk_wavelet_params* p = params();
            p->threshold[j] = bad;
            CHECK(validate(p, 100, 100) != nullptr);
            std::free(p);
        }
        for (float bad : {nan, inf, -1e-6f, 1.0001f}) {
            stk_wavelet_params* p = params();
            p->layer_amount[j] = bad;
            CHECK(validate(p, 100, 100) != nullptr);
            std::free(p);
        }
        stk_wavelet_params* p = params();
        p->gain[j] = -3.0f; p->threshold[j] = 1e30f; p->layer_amount[j] = 0.0f;
        CHECK(validate(p, 100, 100) == nullptr);
        std::free(p);
    }
    for (float bad : {nan, inf, -inf}) {
        stk_wavelet_params* p = params();
        p->residual_gain = bad;
        CHECK(validate(p, 100, 100) != nullptr);
        std::free(p);
    }
    for (float bad : {nan, inf, -0.1f, 1.1f}) {
        stk_wavelet_params* p = params();
        p->amount = bad;
        CHECK(validate(p, 100, 100) != nullptr);
        std::free(p);
    }
    for (int c = 0; c < 4; c++)
        for (float bad : {nan, inf, -1.0f}) {
            stk_wavelet_params* p = params();
            p->sigma[c] = bad;
            CHECK(validate(p, 100, 100) == nullptr);                       // not read while sigma_given is 0
            p->sigma_given = 1;
            CHECK(validate(p, 100, 100) != nullptr);
            std::free(p);
        }
    for (int mode : {-1, 2, 1 << 30}) {
        stk_wavelet_params* p = params();
        p->mode = mode;
        CHECK(validate(p, 100, 100) != nullptr);
        p->mode = STK_WAVELET_SOFT;
        CHECK(validate(p, 100, 100) == nullptr);
        p->reserved = mode;
        CHECK(validate(p, 100, 100) != nullptr);
        std::free(p);
    }
    // ---- when the estimate is needed, sigma and the thresholds
    {
        stk_wavelet_params* p = params();
        double* e = block<double>(8);
        float* t = block<float>(8);
        CHECK(noise_table(8, e) == STK_OK);
        CHECK(!needs_estimate(p));
        p->threshold[5] = 3.0f;                                            // beyond the 4 levels in use
        CHECK(!needs_estimate(p));
        p->threshold[3] = 3.0f;
        CHECK(needs_estimate(p));
        p->sigma_given = 1;
        CHECK(!needs_estimate(p));
        thresholds(p, 8.0f, e, t);
        CHECK(t[0] == 0.0f && t[3] == (float)(3.0 * 8.0 * e[3]) && t[4] == 0.0f && t[5] == 0.0f && t[7] == 0.0f);
        thresholds(p, 0.0f, e, t);
        for (int j = 0; j < 8; j++) CHECK(t[j] == 0.0f);
        p->levels = 8;
        for (int j = 0; j < 8; j++) p->threshold[j] = 3.0e38f;
        thresholds(p, 3.0e38f, e, t);                                      // beyond f32: the cast gives infinity, no trap
        for (int j = 0; j < 8; j++) CHECK(std::isinf(t[j]));
        CHECK(sigma_from_median(0.0f, e[0]) == 0.0f);
        CHECK(std::fabs(sigma_from_median(0.6745f * (float)e[0], e[0]) - 1.0f) < 1e-4f);
        CHECK(std::isfinite(sigma_from_median(1e30f, e[0])));
        std::free(t); std::free(e); std::free(p);
    }
    std::printf("ok\n");
    return 0;
}
