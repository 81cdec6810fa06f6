// psf_harness.cpp — the host half of deconvolution (libstacker_rs_amd/csrc/psf_host.h: the parameter and tap checks, the PSF
// model, the covariance of a frame's shapes) over its edges: radius 1 and 16, near-singular and singular covariances, both
// kinds, zero shapes, every shape flagged, shapes below min_snr, one shape, and each refusal. Every buffer is a heap block of
// exactly the documented size, so that a read or write one element outside it is an ASan report. A stand-alone program:
// built with ASan + UBSan by tests/test_cpu_deconvolve.py and run as it is. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../../libstacker_rs_amd/csrc/psf_host.h"

using namespace stk::psf;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

template <typename T>
static T* block(size_t n) { return (T*)std::calloc(n ? n : 1, sizeof(T)); }

static stk_deconv_params params() {
    stk_deconv_params p{};
    p.iterations = 30; p.radius = 8; p.floor = 1e-6f; p.pedestal = 0.0f; p.lambda = 0.0f; p.tv_eps = 1e-3f; p.amount = 1.0f;
    return p;
}

static int model_case(int kind, double beta, int radius, double cxx, double cyy, double cxy) {
    const int side = 2 * radius + 1;
    float* taps = block<float>((size_t)side * side);
    CHECK(model(kind, beta, radius, cxx, cyy, cxy, taps) == STK_OK);
    double sum = 0.0;
    for (int k = 0; k < side * side; k++) {
        CHECK(std::isfinite(taps[k]) && taps[k] >= 0.0f);
        CHECK(taps[k] == taps[side * side - 1 - k]);                      // point symmetry
        sum += taps[k];
    }
    CHECK(std::fabs(sum - 1.0) < 1e-5);
    CHECK(validate_taps(taps, radius) == nullptr);
    for (int k = 0; k < side * side; k++) CHECK(taps[k] <= taps[(side * side) / 2]);
    std::free(taps);
    return 0;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    // ---- the model: radius 1 and 16, round, elongated and near-singular covariances, both kinds
    for (int radius : {1, 2, 16})
        for (int kind : {STK_PSF_GAUSSIAN, STK_PSF_MOFFAT}) {
            if (model_case(kind, 2.5, radius, 2.0, 2.0, 0.0)) return 1;
            if (model_case(kind, 1.0 + 1e-9, radius, 4.0, 1.96, 0.8)) return 1;
            if (model_case(kind, 100.0, radius, 1e-3, 1e-3, 0.0)) return 1;             // a delta at this sampling
            if (model_case(kind, 4.0, radius, 1.0, 1.0, 1.0 - 1e-12)) return 1;          // det ~ 2e-12: a line
            if (model_case(kind, 3.0, radius, 1e6, 1e6, 0.0)) return 1;                 // flat
        }
    {
        float* taps = block<float>(9);
        CHECK(model(STK_PSF_GAUSSIAN, 0.0, 1, 1.0, 1.0, 1.0, taps) == STK_INVALID_PARAMS);       // singular
        CHECK(model(STK_PSF_GAUSSIAN, 0.0, 1, 1.0, 1.0, 1.5, taps) == STK_INVALID_PARAMS);       // indefinite
        CHECK(model(STK_PSF_GAUSSIAN, 0.0, 1, 0.0, 1.0, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(STK_PSF_GAUSSIAN, 0.0, 1, 1.0, -1.0, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(STK_PSF_GAUSSIAN, 0.0, 1, nan, 1.0, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(STK_PSF_GAUSSIAN, 0.0, 1, 1.0, inf, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(STK_PSF_GAUSSIAN, 0.0, 1, 1e200, 1e200, 0.0, taps) == STK_INVALID_PARAMS);   // the determinant overflows
        CHECK(model(STK_PSF_MOFFAT, 1.0, 1, 1.0, 1.0, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(STK_PSF_MOFFAT, nan, 1, 1.0, 1.0, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(STK_PSF_MOFFAT, inf, 1, 1.0, 1.0, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(2, 2.5, 1, 1.0, 1.0, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(-1, 2.5, 1, 1.0, 1.0, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(STK_PSF_GAUSSIAN, 0.0, 0, 1.0, 1.0, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(STK_PSF_GAUSSIAN, 0.0, 17, 1.0, 1.0, 0.0, taps) == STK_INVALID_PARAMS);
        CHECK(model(STK_PSF_GAUSSIAN, 0.0, 1, 1.0, 1.0, 0.0, nullptr) == STK_INVALID_PARAMS);
        for (int k = 0; k < 9; k++) CHECK(taps[k] == 0.0f);                                     // a refusal writes nothing
        std::free(taps);
    }

    // ---- the shapes
    double cxx = -1, cyy = -1, cxy = -1;
    int32_t used = -1;
    CHECK(from_shapes(nullptr, 0, 0.0, 1.0, &cxx, &cyy, &cxy, &used) == STK_INVALID_PARAMS && used == 0);     // zero shapes
    CHECK(from_shapes(nullptr, 3, 0.0, 1.0, &cxx, &cyy, &cxy, &used) == STK_INVALID_PARAMS);
    CHECK(from_shapes(nullptr, -1, 0.0, 1.0, &cxx, &cyy, &cxy, &used) == STK_INVALID_PARAMS);
    for (int n : {1, 2, 5, 8}) {
        stk_star_shape* s = block<stk_star_shape>((size_t)n);
        for (int k = 0; k < n; k++) { s[k].cxx = 2.0 + k; s[k].cyy = 3.0 + (n - k); s[k].cxy = 0.1 * k; s[k].snr = 10.0 * (k + 1); }
        CHECK(from_shapes(s, n, 0.0, 1.0, &cxx, &cyy, &cxy, &used) == STK_OK && used == n);
        const int kth = (n + 1) / 2 - 1;
        CHECK(cxx == 2.0 + kth && cyy == 3.0 + 1 + kth && cxy == 0.1 * kth);
        CHECK(from_shapes(s, n, 0.0, 2.0, &cxx, &cyy, &cxy, nullptr) == STK_OK && cxx == 4.0 * (2.0 + kth));
        CHECK(from_shapes(s, n, 10.0 * n, 1.0, &cxx, &cyy, &cxy, &used) == STK_OK && used == 1 && cxx == 2.0 + (n - 1));   // the last one alone
        CHECK(from_shapes(s, n, 10.0 * n + 1.0, 1.0, &cxx, &cyy, &cxy, &used) == STK_INVALID_PARAMS && used == 0);          // none bright enough
        for (int k = 0; k < n; k++) s[k].flags = 1 << (k % 4);
        CHECK(from_shapes(s, n, 0.0, 1.0, &cxx, &cyy, &cxy, &used) == STK_INVALID_PARAMS && used == 0);                     // every shape flagged
        s[0].flags = 0; s[0].cxx = 1.0; s[0].cyy = 1.0; s[0].cxy = 1.0;
        CHECK(from_shapes(s, n, 0.0, 1.0, &cxx, &cyy, &cxy, &used) == STK_INVALID_PARAMS && used == 1);                     // not positive definite
        s[0].cxy = nan;
        CHECK(from_shapes(s, n, 0.0, 1.0, &cxx, &cyy, &cxy, &used) == STK_INVALID_PARAMS);
        s[0].cxy = 0.0;
        CHECK(from_shapes(s, n, 0.0, 0.0, &cxx, &cyy, &cxy, &used) == STK_INVALID_PARAMS);
        CHECK(from_shapes(s, n, 0.0, nan, &cxx, &cyy, &cxy, &used) == STK_INVALID_PARAMS);
        CHECK(from_shapes(s, n, nan, 1.0, &cxx, &cyy, &cxy, &used) == STK_INVALID_PARAMS);
        CHECK(from_shapes(s, n, 0.0, 1.0, nullptr, &cyy, &cxy, &used) == STK_INVALID_PARAMS);
        CHECK(from_shapes(s, n, 0.0, 1.0, &cxx, &cyy, &cxy, &used) == STK_OK && used == 1 && cxx == 1.0 && cxy == 0.0);
        std::free(s);
    }

    // ---- the parameter and tap checks
    stk_deconv_params p = params();
    CHECK(validate(&p, 9, 9) == nullptr && validate(&p, 8, 9) != nullptr && validate(&p, 9, 8) != nullptr && validate(nullptr, 9, 9) != nullptr);
#define REFUSED(field, value) do { stk_deconv_params q = params(); q.field = value; CHECK(validate(&q, 64, 64) != nullptr); } while (0)
#define ADMITTED(field, value) do { stk_deconv_params q = params(); q.field = value; CHECK(validate(&q, 64, 64) == nullptr); } while (0)
    REFUSED(iterations, 0); REFUSED(iterations, 1001); ADMITTED(iterations, 1); ADMITTED(iterations, 1000);
    REFUSED(radius, 0); REFUSED(radius, 17); ADMITTED(radius, 1); ADMITTED(radius, 16);
    REFUSED(floor, 0.0f); REFUSED(floor, -1.0f); REFUSED(floor, (float)nan); REFUSED(floor, (float)inf);
    REFUSED(pedestal, (float)nan); REFUSED(pedestal, (float)inf); ADMITTED(pedestal, -5.0f);
    REFUSED(lambda, -1e-3f); REFUSED(lambda, (float)nan); REFUSED(lambda, (float)inf); ADMITTED(lambda, 0.5f);
    REFUSED(tv_eps, 0.0f); REFUSED(tv_eps, (float)nan); REFUSED(tv_eps, (float)inf);
    REFUSED(amount, -0.1f); REFUSED(amount, 1.1f); REFUSED(amount, (float)nan); ADMITTED(amount, 0.0f);
    REFUSED(reserved, 1);
    for (int radius : {1, 16}) {
        const int n = (2 * radius + 1) * (2 * radius + 1);
        float* taps = block<float>((size_t)n);
        CHECK(validate_taps(taps, radius) != nullptr && validate_taps(nullptr, radius) != nullptr);        // sums to 0
        taps[n / 2] = 1.0f;
        CHECK(validate_taps(taps, radius) == nullptr);
        taps[n - 1] = 1.5e-3f;
        CHECK(validate_taps(taps, radius) != nullptr);
        taps[n - 1] = 0.5e-3f;
        CHECK(validate_taps(taps, radius) == nullptr);
        taps[0] = -0.0f;
        CHECK(validate_taps(taps, radius) == nullptr);
        taps[0] = -1e-6f;
        CHECK(validate_taps(taps, radius) != nullptr);
        taps[0] = (float)nan;
        CHECK(validate_taps(taps, radius) != nullptr);
        taps[0] = (float)inf;
        CHECK(validate_taps(taps, radius) != nullptr);
        std::free(taps);
    }
    std::printf("ok\n");
    return 0;
}
