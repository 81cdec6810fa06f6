// entries_harness.cpp — the two rules that say which frames of a stack are samples of a combine and under which matrix
// (combine.h: entries_from_include for the caller-held-warps forms, entries_from_stats for the whole-stack forms), against
// frame lists and matrix pointers written out by hand. Every combine's result depends on them, and they are pure host
// code, so they run here under ASan + UBSan (tests/test_cpu_sanitize.py).
#include <cstdio>
#include <vector>

#include "../../libstacker_rs_amd/csrc/combine.h"

static int failures = 0;

static void expect(const char* what, const EntryTable& t, const std::vector<int>& frame, const std::vector<const double*>& M) {
    if (t.frame == frame && t.M == M && t.size() == (int)frame.size()) return;
    std::printf("%s: got frames", what);
    for (int f : t.frame) std::printf(" %d", f);
    std::printf(" (%zu matrices), want", t.M.size());
    for (int f : frame) std::printf(" %d", f);
    std::printf("%s\n", t.frame == frame ? "; the matrix pointers differ" : "");
    failures++;
}

int main() {
    static const double* const I = IDENTITY3;
    for (int k = 0; k < 9; k++)
        if (IDENTITY3[k] != (k % 4 == 0 ? 1.0 : 0.0)) { std::printf("IDENTITY3[%d] = %g\n", k, IDENTITY3[k]); failures++; }

    // ---- the caller-held-warps forms ----
    std::vector<double> M(4 * 9, 0.5);                      // never read: only addresses are taken
    const double* m = M.data();
    EntryTable t;
    t.frame = {7, 7, 7}; t.M = {nullptr};                    // a used table is overwritten, not appended to
    entries_from_include(1, m, nullptr, t);
    expect("include: n = 1, null", t, {0}, {m});             // frame 0 under M + 0, not the identity
    entries_from_include(4, m, nullptr, t);
    expect("include: n = 4, null", t, {0, 1, 2, 3}, {m, m + 9, m + 18, m + 27});
    const int32_t all[4] = {1, 1, 1, 1};
    entries_from_include(4, m, all, t);
    expect("include: n = 4, all", t, {0, 1, 2, 3}, {m, m + 9, m + 18, m + 27});
    const int32_t middle[4] = {1, 1, 0, 1};
    entries_from_include(4, m, middle, t);
    expect("include: frame 2 dropped", t, {0, 1, 3}, {m, m + 9, m + 27});
    const int32_t first[4] = {0, 5, -1, 1};                  // any non-zero value includes
    entries_from_include(4, m, first, t);
    expect("include: frame 0 dropped", t, {1, 2, 3}, {m + 9, m + 18, m + 27});
    const int32_t none[4] = {0, 0, 0, 0};
    entries_from_include(4, m, none, t);
    expect("include: all zero", t, {}, {});
    const int32_t one0 = 0;
    entries_from_include(1, m, &one0, t);
    expect("include: n = 1, dropped", t, {}, {});

    // ---- the whole-stack forms ----
    std::vector<stk_frame_stats> s(4);
    for (int i = 0; i < 4; i++) { s[i] = stk_frame_stats{}; for (int k = 0; k < 9; k++) s[i].warp[k] = i * 10 + k; }
    const double *w1 = s[1].warp, *w2 = s[2].warp, *w3 = s[3].warp;
    entries_from_stats(1, s.data(), false, t);
    expect("stats: ECC, n = 1", t, {0}, {I});                // frame 0 under the shared identity, not stats[0].warp
    entries_from_stats(1, s.data(), true, t);
    expect("stats: keypoint, n = 1", t, {0}, {I});
    entries_from_stats(4, s.data(), false, t);
    expect("stats: ECC, n = 4", t, {0, 1, 2, 3}, {I, w1, w2, w3});
    s[2].status = 2;
    entries_from_stats(4, s.data(), false, t);
    expect("stats: ECC keeps a non-zero status", t, {0, 1, 2, 3}, {I, w1, w2, w3});
    entries_from_stats(4, s.data(), true, t);
    expect("stats: keypoint drops frame 2", t, {0, 1, 3}, {I, w1, w3});
    s[2].status = 0; s[0].status = 1;
    entries_from_stats(4, s.data(), true, t);
    expect("stats: keypoint keeps frame 0 whatever its status", t, {0, 1, 2, 3}, {I, w1, w2, w3});
    s[1].status = 1; s[2].status = 1; s[3].status = 2;
    entries_from_stats(4, s.data(), true, t);
    expect("stats: keypoint, every moving frame dropped", t, {0}, {I});

    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
