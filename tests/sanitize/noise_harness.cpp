// noise_harness.cpp — the host half of noise estimation (libstacker_rs_amd/csrc/noise_host.h: the reduction of the two
// histograms and the frame weights) on the inputs that stress its indexing: counts in the first and the last bin of either
// histogram, the cut at `top` with and without an overflow bin, empty histograms, the smallest bin counts, n = 1, every
// frame but one excluded, and each refusal. Every buffer is a heap block of exactly the documented size, so that a read or
// write one element outside it is an ASan report. A stand-alone program: built with ASan + UBSan by
// tests/test_cpu_noise.py and run as it is. Prints "ok" and the statistics of the regular cases.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../libstacker_rs_amd/csrc/noise_host.h"

using namespace stk::noise;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct Hist {
    uint32_t *hv, *hr;
    int bv, br;
    Hist(int bv_, int br_) : bv(bv_), br(br_) {
        hv = (uint32_t*)std::calloc((size_t)bv, sizeof(uint32_t));
        hr = (uint32_t*)std::calloc((size_t)br, sizeof(uint32_t));
    }
    ~Hist() { std::free(hv); std::free(hr); }
};

static int run(const Hist& h, int overflow, stk_noise_stat* out) {
    stk_noise_stat* o = (stk_noise_stat*)std::malloc(sizeof(stk_noise_stat));
    const stk_status st = from_hist(h.hv, h.bv, h.hr, h.br, overflow, o);
    *out = *o;
    std::free(o);
    return (int)st;
}

int main() {
    stk_noise_stat s;
    for (int depth : {8, 16}) {
        const int bv = depth == 8 ? 256 : 65536, br = depth == 8 ? 2041 : 65536, ov = depth == 16;
        {   // empty histograms
            Hist h(bv, br);
            CHECK(run(h, ov, &s) == 0);
            CHECK(s.median == 0 && s.mad == 0 && s.res_median == 0 && s.sigma == 0.0 && s.kept == 0 && (s.flags & 1));
        }
        {   // everything in the first bins: a constant frame of zeros
            Hist h(bv, br);
            h.hv[0] = 1000; h.hr[0] = 900;
            CHECK(run(h, ov, &s) == 0);
            CHECK(s.median == 0 && s.mad == 0 && s.res_median == 0 && s.sigma == 0.0 && s.kept == 900 && s.flags == 1);
        }
        {   // everything in the last bins: the 0 / max checkerboard's residuals, all-max values
            Hist h(bv, br);
            h.hv[bv - 1] = 1000; h.hr[br - 1] = 900;
            CHECK(run(h, ov, &s) == 0);
            CHECK(s.median == bv - 1 && s.mad == 0 && s.res_median == br - 1);
            if (ov) CHECK(s.flags == 3 && s.sigma == 0.0 && s.kept == 0);      // the cut stops below the overflow bin
            else CHECK(s.flags == 0 && s.kept == 900 && std::fabs(s.sigma - (br - 1) * 1.0136 / 6.0) < 1e-9);
        }
        {   // both ends of the values and of the residuals
            Hist h(bv, br);
            h.hv[0] = 5; h.hv[bv - 1] = 5; h.hr[1] = 3; h.hr[br - 2] = 4;
            CHECK(run(h, ov, &s) == 0);
            CHECK(s.median == 0 && s.mad == 0 && s.res_median == br - 2);
            h.hv[0] = 4; h.hv[bv / 2] = 3; h.hv[bv - 1] = 4;                   // the median in the middle, the MAD out to both ends
            CHECK(run(h, ov, &s) == 0);
            CHECK(s.median == bv / 2 && s.mad == bv / 2 - 1);
            CHECK(s.kept == 7);                                                // cut == top == br - 2 keeps both bins
            CHECK(((s.flags >> 1) & 1) == ov);
        }
        {   // a Gaussian-like residual histogram: the rounds converge
            Hist h(bv, br);
            for (int b = 0; b < 200 && b < br; b++) h.hr[b] = (uint32_t)(100000.0 * std::exp(-0.5 * (b / 30.0) * (b / 30.0)));
            for (int v = 90; v < 110; v++) h.hv[v] = 1000;
            CHECK(run(h, ov, &s) == 0);
            CHECK(s.flags == 0 && std::fabs(s.sigma - 5.0) < 0.1 && s.median == 99 && s.mad == 5);
            std::printf("depth %d: sigma %.6f kept %lld res_median %d\n", depth, s.sigma, (long long)s.kept, s.res_median);
        }
    }
    {   // the smallest histograms the call takes, and the refusals
        Hist h(1, 2);
        h.hv[0] = 1; h.hr[1] = 1;
        CHECK(run(h, 0, &s) == 0 && s.median == 0 && s.res_median == 1 && s.kept == 1);
        CHECK(run(h, 1, &s) == 0 && s.flags == 3);                             // top = 0: only bin 0 under the cut
        CHECK(from_hist(nullptr, 1, h.hr, 2, 0, &s) == STK_INVALID_PARAMS);
        CHECK(from_hist(h.hv, 1, nullptr, 2, 0, &s) == STK_INVALID_PARAMS);
        CHECK(from_hist(h.hv, 1, h.hr, 2, 0, nullptr) == STK_INVALID_PARAMS);
        CHECK(from_hist(h.hv, 0, h.hr, 2, 0, &s) == STK_INVALID_PARAMS);
        CHECK(from_hist(h.hv, 1, h.hr, 1, 0, &s) == STK_INVALID_PARAMS);
        CHECK(from_hist(h.hv, 65537, h.hr, 2, 0, &s) == STK_INVALID_PARAMS);
        CHECK(from_hist(h.hv, 1, h.hr, 65537, 0, &s) == STK_INVALID_PARAMS);
        CHECK(from_hist(h.hv, 1, h.hr, 2, 2, &s) == STK_INVALID_PARAMS);
    }
    // the largest counts: 2^27 pixels in the last regular bin of a 16-bit histogram stay inside int64
    {
        Hist h(65536, 65536);
        h.hv[65535] = 1u << 27; h.hr[65534] = 1u << 27;
        CHECK(run(h, 1, &s) == 0);
        CHECK(s.kept == (1ll << 27) && s.flags == 2 && std::fabs(s.sigma - 65534.0 * 1.0136 / 6.0) < 1e-6);
    }

    // ---- weights
    for (int n : {1, 2, 7}) {
        for (int cn : {1, 3, 4}) {
            stk_noise_stat* st = (stk_noise_stat*)std::calloc((size_t)n * 4, sizeof(stk_noise_stat));
            stk_frame_weight* rec = (stk_frame_weight*)std::calloc((size_t)n, sizeof(stk_frame_weight));
            int32_t* inc = (int32_t*)std::calloc((size_t)n, sizeof(int32_t));
            float* u = (float*)std::calloc((size_t)n, sizeof(float));
            float* w = (float*)std::calloc((size_t)n, sizeof(float));
            for (int i = 0; i < n; i++) {
                for (int c = 0; c < 4; c++) { st[i * 4 + c].sigma = c < cn ? 1.0 + i : 0.0; rec[i].gain[c] = 1.0f + 0.1f * c; }
                inc[i] = 1; u[i] = 1.0f;
            }
            CHECK(weights(st, n, cn, nullptr, nullptr, nullptr, 0.25, w) == STK_OK);
            for (int i = 0; i < n; i++) CHECK(w[i] == (float)(1.0 / ((1.0 + i) * (1.0 + i))));
            CHECK(weights(st, n, cn, rec, inc, u, 0.25, w) == STK_OK);
            CHECK(w[0] == 1.0f);
            inc[0] = 0;                                                        // the reference moves to frame 1
            if (n == 1) CHECK(weights(st, n, cn, rec, inc, u, 0.25, w) == STK_INVALID_PARAMS);
            else { CHECK(weights(st, n, cn, rec, inc, u, 0.25, w) == STK_OK); CHECK(w[0] == 0.0f && w[1] == 1.0f); }
            inc[0] = 1;
            CHECK(weights(st, n, cn, rec, inc, u, 100.0, w) == STK_OK);       // everything under the floor: equal weights
            for (int i = 0; i < n; i++) CHECK(w[i] == 1.0f);
            // refusals
            CHECK(weights(st, n, cn, rec, inc, u, 0.0, w) == STK_INVALID_PARAMS);
            CHECK(weights(st, n, cn, rec, inc, u, -1.0, w) == STK_INVALID_PARAMS);
            CHECK(weights(st, n, cn, rec, inc, u, std::numeric_limits<double>::infinity(), w) == STK_INVALID_PARAMS);
            CHECK(weights(st, n, cn, rec, inc, u, std::nan(""), w) == STK_INVALID_PARAMS);
            u[n - 1] = -1.0f;
            CHECK(weights(st, n, cn, rec, inc, u, 0.25, w) == STK_INVALID_PARAMS);
            u[n - 1] = std::numeric_limits<float>::infinity();
            CHECK(weights(st, n, cn, rec, inc, u, 0.25, w) == STK_INVALID_PARAMS);
            u[n - 1] = 1.0f;
            st[(n - 1) * 4].sigma = std::nan("");
            CHECK(weights(st, n, cn, rec, inc, u, 0.25, w) == STK_INVALID_PARAMS);
            st[(n - 1) * 4].sigma = 1.0;
            for (int c = 0; c < 4; c++) rec[n - 1].gain[c] = 0.0f;
            CHECK(weights(st, n, cn, rec, inc, u, 0.25, w) == STK_INVALID_PARAMS);
            CHECK(weights(st, 0, cn, rec, inc, u, 0.25, w) == STK_INVALID_PARAMS);
            CHECK(weights(st, n, 2, rec, inc, u, 0.25, w) == STK_INVALID_PARAMS);
            CHECK(weights(nullptr, n, cn, rec, inc, u, 0.25, w) == STK_INVALID_PARAMS);
            CHECK(weights(st, n, cn, rec, inc, u, 0.25, nullptr) == STK_INVALID_PARAMS);
            std::free(st); std::free(rec); std::free(inc); std::free(u); std::free(w);
        }
    }
    std::printf("ok\n");
    return 0;
}
