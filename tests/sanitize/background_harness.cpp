// background_harness.cpp — the host half of the background model (libstacker_rs_amd/csrc/background_host.h: the
// estimator) over degenerate grids and records: 1 x 1 and 2 x 2 grids (no 3 x 3 neighbourhood, no edge extrapolation), all
// nodes invalid, records with n = 0, records with kept = 1, random records on grids whose last row and column lie beyond
// the frame, every estimator and switch, and each refusal. Every buffer is a heap block of exactly the documented size, so
// that a read or write one element outside it is an ASan report. A stand-alone program: built with ASan + UBSan by
// tests/test_cpu_background.py and run as it is. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../libstacker_rs_amd/csrc/background_host.h"

using namespace stk::bg;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

template <typename T>
static T* block(size_t n) { return (T*)std::calloc(n ? n : 1, sizeof(T)); }

static stk_background_params params(int step) {
    stk_background_params p{};
    p.step = step; p.clip_iters = 3; p.kappa = 3.0f; p.f32_scale = 1.0f; p.estimator = STK_BG_MODE; p.min_count = 0;
    p.max_reject = 0.5f; p.recentre = 1; p.filter = 1; p.fill = 4;
    return p;
}

// a record as the device writes it for a window of n keys around `level`
static stk_bg_cell record(int n, int kept, int level, int mad) {
    stk_bg_cell r{};
    r.n = n; r.kept = kept; r.med = level; r.mad = mad; r.lo = std::max(level - 3 * mad, 0); r.hi = std::min(level + 3 * mad, 65535);
    r.sum = (int64_t)kept * level; r.sum2 = (uint64_t)kept * (uint64_t)level * (uint64_t)level + (uint64_t)kept * (uint64_t)mad * (uint64_t)mad;
    return r;
}

struct Planes {
    float *level, *rms; int32_t* valid; int32_t flags;
    Planes(size_t nodes, int C) : level(block<float>(nodes * C)), rms(block<float>(nodes * C)), valid(block<int32_t>(nodes)), flags(-1) {}
    ~Planes() { std::free(level); std::free(rms); std::free(valid); }
};

int main() {
    std::mt19937_64 rng(4321);
    auto uni = [&](int lo, int hi) { return (int)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };

    // ---- 1 x 1 grid (a 1 x 1 frame) and 2 x 2 grids, every channel count and depth
    for (int cn : {1, 3, 4})
        for (int depth : {8, 16, 32})
            for (int size : {1, 2, 17}) {                                    // 17 px at step 16: nodes at 0 and 16
                const int C = std::min(cn, 3), g = grid_nodes(size, 16);
                CHECK(g == (size == 1 ? 1 : 2));
                const size_t nodes = (size_t)g * g;
                stk_bg_cell* cells = block<stk_bg_cell>(nodes * C);
                for (size_t i = 0; i < nodes * C; i++) cells[i] = record(100, 90, 1000 + (int)i, 5);
                Planes o(nodes, C);
                stk_background_params p = params(16);
                for (int est = 0; est < 3; est++) {
                    p.estimator = est;
                    CHECK(estimate(size, size, cn, depth, &p, cells, o.level, o.rms, o.valid, &o.flags) == STK_OK);
                    CHECK(o.flags == 0);
                    for (size_t i = 0; i < nodes; i++) CHECK(o.valid[i] == (1 << C) - 1);
                    for (size_t i = 0; i < nodes * C; i++) CHECK(std::isfinite(o.level[i]) && o.rms[i] == 5.0f);
                }
                CHECK(estimate(size, size, cn, depth, &p, cells, o.level, nullptr, nullptr, nullptr) == STK_OK);     // the optional outputs
                std::free(cells);
            }

    // ---- all nodes invalid: zeros and the flag bits; n = 0 records; kept = 1
    {
        const int w = 150, h = 100, step = 32, gw = grid_nodes(w, step), gh = grid_nodes(h, step), C = 3;
        const size_t nodes = (size_t)gw * gh;
        stk_bg_cell* cells = block<stk_bg_cell>(nodes * C);                 // calloc: n = 0 records
        Planes o(nodes, C);
        stk_background_params p = params(step);
        CHECK(estimate(w, h, 3, 16, &p, cells, o.level, o.rms, o.valid, &o.flags) == STK_OK);
        CHECK(o.flags == 7);
        for (size_t i = 0; i < nodes * C; i++) CHECK(o.level[i] == 0.0f && o.rms[i] == 0.0f);
        for (size_t i = 0; i < nodes; i++) CHECK(o.valid[i] == 0);
        for (size_t i = 0; i < nodes * C; i++) cells[i] = record(1, 1, 777, 0);                     // kept = 1: below min_count
        CHECK(estimate(w, h, 3, 16, &p, cells, o.level, o.rms, o.valid, &o.flags) == STK_OK);
        CHECK(o.flags == 7 && o.level[0] == 0.0f);
        p.min_count = 1;                                                    // ... and valid once one key is enough
        CHECK(estimate(w, h, 3, 16, &p, cells, o.level, o.rms, o.valid, &o.flags) == STK_OK);
        CHECK(o.flags == 0);
        for (size_t i = 0; i < nodes * C; i++) CHECK(o.level[i] == 777.0f && o.rms[i] == 0.0f);
        // one valid node in channel 1 alone: the fill spreads it, the fallback takes the rest
        for (size_t i = 0; i < nodes * C; i++) cells[i] = stk_bg_cell{};
        cells[(size_t)(1 * gw + 1) * C + 1] = record(1000, 900, 1234, 7);
        p.min_count = 0; p.fill = 1;
        CHECK(estimate(w, h, 3, 16, &p, cells, o.level, o.rms, o.valid, &o.flags) == STK_OK);
        CHECK(o.flags == 5);
        for (size_t i = 0; i < nodes; i++) CHECK(o.level[i * C + 1] == 1234.0f && o.level[i * C] == 0.0f && o.valid[i] == (i == (size_t)gw + 1 ? 2 : 0));
        std::free(cells);
    }

    // ---- random records, scattered invalid nodes, grids whose last node lies beyond the frame
    for (int round = 0; round < 60; round++) {
        const int steps[4] = {16, 32, 64, 128};
        const int step = steps[round % 4], w = uni(1, 400), h = uni(1, 300), cn = round % 3 == 0 ? 1 : round % 3 == 1 ? 3 : 4;
        const int C = std::min(cn, 3), gw = grid_nodes(w, step), gh = grid_nodes(h, step);
        const size_t nodes = (size_t)gw * gh;
        stk_bg_cell* cells = block<stk_bg_cell>(nodes * C);
        for (size_t i = 0; i < nodes * C; i++) {
            const int kind = uni(0, 9), n = uni(1, (step + 1) * (step + 1));
            cells[i] = kind == 0 ? stk_bg_cell{} : kind == 1 ? record(n, 1, uni(0, 65535), 0) : record(n, uni(1, n), uni(0, 65535), uni(0, 300));
        }
        Planes o(nodes, C);
        stk_background_params p = params(step);
        p.estimator = round % 3; p.recentre = round & 1; p.filter = (round >> 1) & 1; p.fill = round % 17; p.min_count = round % 5 == 0 ? 1 : 0;
        p.max_reject = (float)(round % 11) / 10.0f; p.f32_scale = 16.0f;
        const int depth = round % 2 ? 32 : 16;
        CHECK(estimate(w, h, cn, depth, &p, cells, o.level, o.rms, o.valid, &o.flags) == STK_OK);
        for (size_t i = 0; i < nodes * C; i++) CHECK(std::isfinite(o.level[i]) && std::isfinite(o.rms[i]) && o.rms[i] >= 0.0f);
        CHECK(o.flags >= 0 && o.flags < (1 << C));
        std::free(cells);
    }

    // ---- refusals
    {
        stk_bg_cell* cells = block<stk_bg_cell>(4);
        Planes o(4, 1);
        stk_background_params p = params(16);
        CHECK(estimate(17, 17, 1, 16, &p, cells, o.level, o.rms, o.valid, &o.flags) == STK_OK);
        CHECK(estimate(0, 17, 1, 16, &p, cells, o.level, o.rms, o.valid, &o.flags) == STK_INVALID_PARAMS);
        CHECK(estimate(17, 17, 2, 16, &p, cells, o.level, o.rms, o.valid, &o.flags) == STK_INVALID_PARAMS);
        CHECK(estimate(17, 17, 1, 12, &p, cells, o.level, o.rms, o.valid, &o.flags) == STK_INVALID_PARAMS);
        CHECK(estimate(17, 17, 1, 16, nullptr, cells, o.level, o.rms, o.valid, &o.flags) == STK_INVALID_PARAMS);
        CHECK(estimate(17, 17, 1, 16, &p, nullptr, o.level, o.rms, o.valid, &o.flags) == STK_INVALID_PARAMS);
        CHECK(estimate(17, 17, 1, 16, &p, cells, nullptr, o.rms, o.valid, &o.flags) == STK_INVALID_PARAMS);
        stk_background_params q = p; q.step = 8;
        CHECK(validate(&q, false) != nullptr);
        q = p; q.clip_iters = 6; CHECK(validate(&q, false) != nullptr);
        q = p; q.kappa = 0.0f; CHECK(validate(&q, false) != nullptr);
        q = p; q.f32_scale = std::nanf(""); CHECK(validate(&q, false) == nullptr && validate(&q, true) != nullptr);
        q = p; q.reserved[2] = 1; CHECK(validate(&q, false) != nullptr);
        std::free(cells);
    }
    std::printf("ok\n");
    return 0;
}
