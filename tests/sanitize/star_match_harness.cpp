// star_match_harness.cpp — the host half of star registration (libstacker_rs_amd/csrc/star_match.h) on the lists that
// stress its indexing: 0 .. 3 stars, coincident stars, collinear stars, more stars than match_stars, lists of unequal
// length, a singular and a zero homography, non-finite coordinates. A stand-alone program: built with ASan + UBSan by
// tests/test_cpu_star.py and run as it is. Prints "ok" and the pair counts of the regular cases.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../libstacker_rs_amd/csrc/star_match.cpp"

using namespace stk::star;

static stk_star_params defaults() {
    stk_star_params p{};
    p.radius = 4; p.kappa = 4.f; p.min_contrast = 8; p.min_pixels = 3; p.max_stars = 200; p.match_stars = 50; p.neighbours = 5;
    p.tri_tolerance = 0.01; p.min_votes = 2; p.refine = 1; p.min_stars = 6; p.min_inliers = 4; p.method = STK_METHOD_RANSAC;
    p.ransac_reproj_threshold = 2.0; p.border_mode = STK_BORDER_CONSTANT;
    return p;
}

static std::vector<stk_star> field(int n, unsigned seed, double ang, double scale, double tx, double ty) {
    std::vector<stk_star> s(n);
    unsigned st = seed * 2654435761u + 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (double)(st >> 8) / (double)(1u << 24); };
    const double c = std::cos(ang) * scale, sn = std::sin(ang) * scale;
    for (int i = 0; i < n; i++) {
        const double x = rnd() * 480.0, y = rnd() * 360.0;
        s[i] = stk_star{(float)(c * x - sn * y + tx), (float)(sn * x + c * y + ty), (float)(1000 - i), 0, 0, 0, 0, 0};
    }
    return s;
}

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// the call as a C caller makes it: heap blocks of exactly the documented size
static int run_lists(const std::vector<stk_star>& mv, const std::vector<stk_star>& rf, const stk_star_params& p, stk_status want, int* n_out) {
    stk_star* m = (stk_star*)std::malloc(sizeof(stk_star) * mv.size() + 1);
    stk_star* r = (stk_star*)std::malloc(sizeof(stk_star) * rf.size() + 1);
    for (size_t i = 0; i < mv.size(); i++) m[i] = mv[i];
    for (size_t i = 0; i < rf.size(); i++) r[i] = rf[i];
    int32_t* pairs = (int32_t*)std::malloc(sizeof(int32_t) * 2 * (size_t)std::max(p.match_stars, 1));
    int32_t n = -1;
    const stk_status st = stk_star_match_lists(mv.empty() ? nullptr : m, (int32_t)mv.size(), rf.empty() ? nullptr : r, (int32_t)rf.size(), &p, pairs, &n);
    int bad = st != want;
    if (st == STK_OK) {
        bad |= n < 0 || n > p.match_stars;
        for (int k = 0; k < n && !bad; k++)
            bad |= pairs[2 * k] < 0 || pairs[2 * k] >= (int)mv.size() || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= (int)rf.size() ||
                   (k > 0 && pairs[2 * k] <= pairs[2 * k - 2]);
    }
    if (n_out) *n_out = n;
    std::free(m); std::free(r); std::free(pairs);
    return bad;
}

int main() {
    const stk_star_params p = defaults();
    int n = 0;
    // 0 .. 3 stars on either side, and against a full field
    const std::vector<stk_star> full = field(120, 1, 0.0, 1.0, 0.0, 0.0);
    for (int a = 0; a <= 3; a++)
        for (int b = 0; b <= 3; b++) {
            CHECK(!run_lists(field(a, 2, 0.3, 1.0, 5, 5), field(b, 2, 0.0, 1.0, 0, 0), p, STK_OK, &n));
            CHECK(n == 0 || (a == 3 && b == 3));
        }
    for (int a = 0; a <= 3; a++) {
        CHECK(!run_lists(field(a, 3, 0.0, 1.0, 0, 0), full, p, STK_OK, &n));
        CHECK(!run_lists(full, field(a, 3, 0.0, 1.0, 0, 0), p, STK_OK, &n));
    }
    // coincident stars: all at one point, and pairs of duplicates inside a field
    std::vector<stk_star> same(40, stk_star{10.f, 20.f, 1.f, 0, 0, 0, 0, 0});
    CHECK(!run_lists(same, same, p, STK_OK, &n) && n == 0);
    std::vector<stk_star> dup = field(60, 4, 0.0, 1.0, 0, 0);
    for (int i = 0; i + 1 < 60; i += 2) dup[i + 1] = dup[i];
    CHECK(!run_lists(dup, full, p, STK_OK, &n));
    CHECK(!run_lists(dup, dup, p, STK_OK, &n));
    // collinear stars: every triangle has c / a small or a zero area; evenly and unevenly spaced
    std::vector<stk_star> line(50), line2(50);
    for (int i = 0; i < 50; i++) { line[i] = stk_star{(float)(3 * i), (float)(2 * i), 1.f, 0, 0, 0, 0, 0}; line2[i] = stk_star{(float)(i * i), 7.f, 1.f, 0, 0, 0, 0, 0}; }
    CHECK(!run_lists(line, line, p, STK_OK, &n));
    CHECK(!run_lists(line2, line, p, STK_OK, &n));
    // regular cases: a rotated, scaled, shifted copy pairs almost every star of the first match_stars
    int n_rot = 0, n_flip = 0;
    CHECK(!run_lists(field(120, 1, 2.0, 1.03, 30, -20), full, p, STK_OK, &n_rot));
    CHECK(n_rot >= 40);
    CHECK(!run_lists(field(200, 1, 3.14159265358979, 1.0, 479, 359), field(200, 1, 0.0, 1.0, 0, 0), p, STK_OK, &n_flip));
    CHECK(n_flip >= 40);
    // the smallest and largest parameter values
    stk_star_params q = p;
    q.match_stars = 4; q.neighbours = 2; q.min_votes = 1;
    CHECK(!run_lists(field(9, 5, 1.0, 1.0, 0, 0), field(7, 5, 0.0, 1.0, 0, 0), q, STK_OK, &n));
    q.match_stars = 200; q.neighbours = 8;
    CHECK(!run_lists(field(200, 6, 1.0, 1.0, 0, 0), field(150, 6, 0.0, 1.0, 0, 0), q, STK_OK, &n));
    // refusals: parameters out of range, the methods that are not implemented, coordinates that are not finite
    q = p; q.match_stars = 201; CHECK(!run_lists(full, full, q, STK_INVALID_PARAMS, &n));
    q = p; q.neighbours = 1; CHECK(!run_lists(full, full, q, STK_INVALID_PARAMS, &n));
    q = p; q.tri_tolerance = NAN; CHECK(!run_lists(full, full, q, STK_INVALID_PARAMS, &n));
    q = p; q.method = STK_METHOD_RHO; CHECK(!run_lists(full, full, q, STK_NOT_IMPLEMENTED, &n));
    std::vector<stk_star> nanlist = full;
    nanlist[17].x = NAN;
    CHECK(!run_lists(nanlist, full, p, STK_INVALID_PARAMS, &n));
    nanlist[17].x = INFINITY;
    CHECK(!run_lists(full, nanlist, p, STK_INVALID_PARAMS, &n));
    // the guided re-match: identity, a singular matrix, the zero matrix, empty lists
    std::vector<int32_t> g;
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Sg[9] = {1, 2, 3, 2, 4, 6, 0, 0, 0};
    guided_pairs(full.data(), 120, full.data(), 120, I, 2.0, g);
    CHECK(g.size() == 240);
    for (int k = 0; k < 120; k++) CHECK(g[2 * k] == k && g[2 * k + 1] == k);
    guided_pairs(full.data(), 120, full.data(), 120, Z, 2.0, g);
    CHECK(g.empty());
    guided_pairs(full.data(), 120, full.data(), 120, Sg, 2.0, g);
    CHECK(g.empty());
    guided_pairs(full.data(), 0, full.data(), 120, I, 2.0, g);
    CHECK(g.empty());
    guided_pairs(full.data(), 120, full.data(), 0, I, 2.0, g);
    CHECK(g.empty());
    guided_pairs(same.data(), 40, same.data(), 40, I, 2.0, g);           // all coincident: star 0 pairs with star 0 only
    CHECK(g.size() == 2 && g[0] == 0 && g[1] == 0);
    // triangles of fewer than three stars, and votes against an empty triangle list
    std::vector<Triangle> t0, t1;
    triangles(full.data(), 2, 50, 5, t0);
    CHECK(t0.empty());
    triangles(full.data(), 120, 50, 5, t1);
    CHECK(!t1.empty());
    std::vector<int32_t> pr;
    vote_pairs(t1, 50, t0, 2, 0.01, 2, pr);
    CHECK(pr.empty());
    vote_pairs(t0, 2, t1, 50, 0.01, 2, pr);
    CHECK(pr.empty());
    std::printf("ok %d %d\n", n_rot, n_flip);
    return 0;
}
