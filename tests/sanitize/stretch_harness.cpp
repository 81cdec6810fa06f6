// stretch_harness.cpp — the host half of the display stretch (libstacker_rs_amd/csrc/stretch_host.h: the parameter checks,
// the quantile ranks, the auto rule, the table builder and the keys) over its edges: every refusal with bad, NaN and infinite
// arguments, the smallest and the largest table, records of every kind. Every buffer is a heap block of exactly the
// documented size, so that a read or write one element outside it is an ASan report. A stand-alone program: built with
// ASan + UBSan by tests/test_cpu_stretch.py and run as it is. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "../../libstacker_rs_amd/csrc/stretch_host.h"

using namespace stk::stretch;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

template <typename T>
static T* block(size_t n) { return (T*)std::calloc(n ? n : 1, sizeof(T)); }

static stk_stretch_params* params() {
    stk_stretch_params* p = block<stk_stretch_params>(1);
    p->curve = STK_STRETCH_MTF; p->out_depth = STK_DEPTH_F32; p->out_scale = 1.0f;
    for (int c = 0; c < 4; c++) { p->black[c] = 0.0f; p->white[c] = 1.0f; p->midtone[c] = 0.5f; }
    return p;
}

static stk_image_stat* records() {
    stk_image_stat* s = block<stk_image_stat>(4);
    for (int c = 0; c < 3; c++) { s[c].count = 1000; s[c].min = 0.01f; s[c].max = 0.9f; s[c].median = 0.02f + 0.01f * c; s[c].mad = 0.002f; s[c].q[0] = 0.5f; }
    return s;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    const double dinf = std::numeric_limits<double>::infinity(), dnan = std::nan("");
    // ---- the tables: every kind into a block of exactly knots + 1 floats
    for (int kind : {STK_CURVE_ASINH, STK_CURVE_GAMMA, STK_CURVE_SRGB})
        for (int knots : {2, 3, 255, 4096, 65536}) {
            float* t = block<float>((size_t)knots + 1);
            CHECK(table(kind, 2.5, knots, t) == STK_OK);
            CHECK(t[0] == 0.0f && t[knots] == 1.0f);
            for (int k = 1; k <= knots; k++) CHECK(t[k] >= t[k - 1] && t[k] <= 1.0f);
            stk_stretch_params* p = params();
            p->curve = STK_STRETCH_TABLE;
            CHECK(validate(p, 3, t, knots) == nullptr);
            t[knots / 2] = nan; CHECK(validate(p, 3, t, knots) != nullptr);
            t[knots / 2] = 1.5f; CHECK(validate(p, 3, t, knots) != nullptr);
            t[knots / 2] = -0.5f; CHECK(validate(p, 3, t, knots) != nullptr);
            t[knots / 2] = 0.5f; t[knots] = inf; CHECK(validate(p, 3, t, knots) != nullptr);
            std::free(p);
            std::free(t);
        }
    {
        float* t = block<float>(9);
        for (int knots : {1, 0, -1, 65537, 1 << 30, -(1 << 30)}) CHECK(table(STK_CURVE_ASINH, 10.0, knots, t) == STK_INVALID_PARAMS);
        for (int kind : {-1, 3, 1 << 30}) CHECK(table(kind, 10.0, 8, t) == STK_INVALID_PARAMS);
        for (double bad : {0.0, -1.0, dnan, dinf, -dinf}) {
            CHECK(table(STK_CURVE_ASINH, bad, 8, t) == STK_INVALID_PARAMS);
            CHECK(table(STK_CURVE_GAMMA, bad, 8, t) == STK_INVALID_PARAMS);
            CHECK(table(STK_CURVE_SRGB, bad, 8, t) == STK_OK);
        }
        CHECK(table(STK_CURVE_ASINH, 10.0, 8, nullptr) == STK_INVALID_PARAMS);
        CHECK(table(STK_CURVE_ASINH, 1e300, 8, t) == STK_OK && table(STK_CURVE_ASINH, 1e-300, 8, t) == STK_OK);
        CHECK(table(STK_CURVE_GAMMA, 1e300, 8, t) == STK_OK && table(STK_CURVE_GAMMA, 1e-300, 8, t) == STK_OK);
        std::free(t);
    }
    // ---- the stretch parameters: every field, out of range, NaN and infinite
    {
        stk_stretch_params* p = params();
        CHECK(validate(nullptr, 3, nullptr, 0) != nullptr);
        for (int cn : {1, 3, 4}) CHECK(validate(p, cn, nullptr, 0) == nullptr);
        for (int cn : {0, 2, 5, -1}) CHECK(validate(p, cn, nullptr, 0) != nullptr);
        for (int v : {-1, 3, 1 << 30}) { p->curve = v; CHECK(validate(p, 3, nullptr, 0) != nullptr); }
        p->curve = STK_STRETCH_LINEAR;
        for (int v : {-1, 2}) { p->colour = v; CHECK(validate(p, 3, nullptr, 0) != nullptr); }
        p->colour = 1; CHECK(validate(p, 3, nullptr, 0) == nullptr && validate(p, 1, nullptr, 0) == nullptr);
        for (int v : {0, 7, 24, 64, -8}) { p->out_depth = v; CHECK(validate(p, 3, nullptr, 0) != nullptr); }
        for (int v : {STK_DEPTH_U8, STK_DEPTH_U16, STK_DEPTH_F32}) { p->out_depth = v; CHECK(validate(p, 3, nullptr, 0) == nullptr); }
        p->reserved = 1; CHECK(validate(p, 3, nullptr, 0) != nullptr); p->reserved = 0;
        for (float bad : {nan, inf, -inf}) { p->out_scale = bad; CHECK(validate(p, 3, nullptr, 0) != nullptr); }
        p->out_scale = -2.0f; CHECK(validate(p, 3, nullptr, 0) == nullptr);
        for (int c = 0; c < 3; c++) {
            for (float bad : {nan, inf, -inf}) {
                p->black[c] = bad; CHECK(validate(p, 3, nullptr, 0) != nullptr); p->black[c] = 0.0f;
                p->white[c] = bad; CHECK(validate(p, 3, nullptr, 0) != nullptr); p->white[c] = 1.0f;
            }
            p->white[c] = 0.0f; CHECK(validate(p, 3, nullptr, 0) != nullptr);                    // white == black
            p->white[c] = -1.0f; CHECK(validate(p, 3, nullptr, 0) != nullptr); p->white[c] = 1.0f;
            p->curve = STK_STRETCH_MTF;
            for (float bad : {nan, inf, -inf, 0.0f, 1.0f, -0.5f, 1.5f}) { p->midtone[c] = bad; CHECK(validate(p, 3, nullptr, 0) != nullptr); }
            p->curve = STK_STRETCH_LINEAR; CHECK(validate(p, 3, nullptr, 0) == nullptr);        // the midtone is read under MTF alone
            p->midtone[c] = 0.5f;
            CHECK((validate(p, 1, nullptr, 0) == nullptr));
        }
        p->black[3] = nan; p->white[3] = -inf; p->midtone[3] = 7.0f; p->curve = STK_STRETCH_MTF;
        CHECK(validate(p, 4, nullptr, 0) == nullptr);                                             // the entry of alpha is not read
        p->black[1] = nan; CHECK(validate(p, 1, nullptr, 0) == nullptr && validate(p, 3, nullptr, 0) != nullptr);
        p->black[1] = 0.0f; p->curve = STK_STRETCH_TABLE;
        float* t = block<float>(3);
        t[2] = 1.0f;
        CHECK(validate(p, 3, nullptr, 2) != nullptr && validate(p, 3, t, 2) == nullptr);
        for (int knots : {1, 0, -1, 65537, 1 << 30}) CHECK(validate(p, 3, t, knots) != nullptr);
        std::free(t);
        std::free(p);
    }
    // ---- the quantiles and their ranks
    {
        double* q = block<double>(4);
        CHECK(validate_quantiles(nullptr, 0) == nullptr && validate_quantiles(q, 4) == nullptr);
        CHECK(validate_quantiles(nullptr, 1) != nullptr && validate_quantiles(q, 5) != nullptr && validate_quantiles(q, -1) != nullptr);
        for (double bad : {dnan, dinf, -dinf, -1e-9, 1.0 + 1e-9}) { q[3] = bad; CHECK(validate_quantiles(q, 4) != nullptr && validate_quantiles(q, 3) == nullptr); }
        std::free(q);
        CHECK(quantile_rank(0.0, 1) == 1 && quantile_rank(1.0, 1) == 1 && quantile_rank(0.0, 10) == 1 && quantile_rank(1.0, 10) == 10);
        CHECK(quantile_rank(0.1, 10) == 1 && quantile_rank(0.11, 10) == 2 && quantile_rank(0.5, 5) == 3);
        const int64_t big = ((int64_t)1 << 31) - 1;
        CHECK(quantile_rank(1.0, big) == big && quantile_rank(0.5, big) == (big + 1) / 2);
    }
    // ---- the rule: the defaults, every mode, bad parameters, bad records
    {
        stk_image_stat* s = records();
        stk_stretch_params* out = block<stk_stretch_params>(1);
        stk_stretch_auto_params* a = block<stk_stretch_auto_params>(1);
        for (int cn : {1, 3, 4}) CHECK(auto_params(s, cn, nullptr, out) == STK_OK && out->curve == STK_STRETCH_MTF && validate(out, cn, nullptr, 0) == nullptr);
        for (int cn : {0, 2, 5, -3}) CHECK(auto_params(s, cn, nullptr, out) == STK_INVALID_PARAMS);
        CHECK(auto_params(nullptr, 3, nullptr, out) == STK_INVALID_PARAMS && auto_params(s, 3, nullptr, nullptr) == STK_INVALID_PARAMS);
        CHECK(out->black[3] == 0.0f && out->white[3] == 1.0f && out->midtone[3] == 0.5f);
        *a = auto_defaults();
        for (int linked : {0, 1})
            for (int mode : {0, 1, 2}) {
                a->linked = linked; a->white_mode = mode;
                CHECK(auto_params(s, 3, a, out) == STK_OK && validate(out, 3, nullptr, 0) == nullptr);
                for (int c = 0; c < 3; c++) CHECK(out->midtone[c] >= 1e-6f && out->midtone[c] <= 1.0f - 1e-6f && out->black[c] >= s[c].min);
            }
        *a = auto_defaults();
        for (double bad : {dnan, dinf, -dinf, 1e-9}) { a->shadows_clip = bad; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS); }
        a->shadows_clip = 0.0; CHECK(auto_params(s, 3, a, out) == STK_OK);
        for (double bad : {dnan, dinf, 0.0, 1.0, -0.25}) { a->target_background = bad; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS); }
        a->target_background = 0.25;
        for (double bad : {dnan, dinf, -dinf}) { a->white = bad; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS); }
        a->white = 1.0;
        for (double bad : {dnan, dinf, -0.1, 1.1}) { a->white_quantile = bad; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS); }
        a->white_quantile = 0.999;
        for (int bad : {-1, 2, 1 << 30}) { a->linked = bad; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS); }
        a->linked = 0;
        for (int bad : {-1, 3, 1 << 30}) { a->white_mode = bad; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS); }
        a->white_mode = 0;
        for (float bad : {nan, inf, -inf}) {
            s[2].median = bad; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS && auto_params(s, 1, a, out) == STK_OK); s[2].median = 0.03f;
            s[0].mad = bad; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS); s[0].mad = 0.002f;
            s[1].min = bad; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS); s[1].min = 0.01f;
            s[1].max = bad; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS); s[1].max = 0.9f;
            s[3].median = bad; CHECK(auto_params(s, 4, a, out) == STK_OK); s[3].median = 0.0f;    // alpha's record is not read
        }
        s[0].count = -1; CHECK(auto_params(s, 3, a, out) == STK_INVALID_PARAMS); s[0].count = 1000;
        // a constant image, MAD 0, x0 = 0, an empty channel, the largest magnitudes
        s[0].min = s[0].max = s[0].median = 0.25f; s[0].mad = 0.0f;
        a->white_mode = 1;
        CHECK(auto_params(s, 3, a, out) == STK_OK && out->black[0] == 0.25f && out->white[0] == 1.25f && out->midtone[0] == 0.5f);
        s[1] = stk_image_stat{};
        CHECK(auto_params(s, 3, a, out) == STK_OK && out->black[1] == 0.0f && out->white[1] == 1.0f && out->midtone[1] == 0.5f);
        s[2].min = -3.4e38f; s[2].max = 3.4e38f; s[2].median = 3.0e38f; s[2].mad = 3.4e38f;
        for (int linked : {0, 1}) { a->linked = linked; CHECK(auto_params(s, 3, a, out) == STK_OK && std::isfinite(out->midtone[2])); }
        std::free(a);
        std::free(out);
        std::free(s);
    }
    // ---- the keys: order and the way back
    {
        const float v[] = {-inf, -3.4e38f, -1.0f, -1e-45f, 0.0f, 1e-45f, 1.0f, 3.4e38f, inf};
        uint32_t prev = 0;
        for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) {
            uint32_t b;
            std::memcpy(&b, &v[i], 4);
            const uint32_t k = key_of_bits(b);
            CHECK(i == 0 || k > prev);
            CHECK(value_of_key(k) == v[i]);
            prev = k;
        }
        CHECK(value_of_key(0xFFFFFFFFu) != value_of_key(0xFFFFFFFFu));                            // the largest key is a NaN's: no sample has it
    }
    std::printf("ok\n");
    return 0;
}
