// star_match.cpp — the host half of star registration: declarations and contracts in star_match.h, definition in
// include/stacker.h (stk_star_params, "Matching"). No HIP call, no stk_ctx.
#include "star_match.h"

#include <algorithm>
#include <array>
#include <cmath>

namespace stk {
namespace star {

namespace {

inline double dist(const stk_star& p, const stk_star& q) {
    const double dx = (double)q.x - (double)p.x, dy = (double)q.y - (double)p.y;
    return std::sqrt(dx * dx + dy * dy);
}

}  // namespace

void triangles(const stk_star* s, int count, int match_stars, int neighbours, std::vector<Triangle>& out) {
    out.clear();
    const int p = std::max(0, std::min(match_stars, count));
    if (p < 3) return;
    const int nn = std::min(neighbours, p - 1);
    std::vector<std::array<int, 3>> triples;
    std::vector<std::pair<double, int>> near(p - 1);
    for (int i = 0; i < p; i++) {
        int k = 0;
        for (int j = 0; j < p; j++) if (j != i) near[k++] = {dist(s[i], s[j]), j};
        std::sort(near.begin(), near.end());                 // by distance, ties to the lower index
        for (int a = 0; a < nn; a++)
            for (int b = a + 1; b < nn; b++) {
                std::array<int, 3> t{i, near[a].second, near[b].second};
                std::sort(t.begin(), t.end());
                triples.push_back(t);
            }
    }
    std::sort(triples.begin(), triples.end());
    triples.erase(std::unique(triples.begin(), triples.end()), triples.end());
    for (const auto& t : triples) {
        // a side is named by its opposite vertex
        std::pair<double, int> side[3] = {{dist(s[t[1]], s[t[2]]), t[0]}, {dist(s[t[0]], s[t[2]]), t[1]}, {dist(s[t[0]], s[t[1]]), t[2]}};
        std::sort(side, side + 3, [](const std::pair<double, int>& x, const std::pair<double, int>& y) {
            return x.first != y.first ? x.first > y.first : x.second < y.second;
        });
        const double a = side[0].first, b = side[1].first, c = side[2].first;
        if (!(a > 0.0) || c / a < 0.1) continue;
        out.push_back(Triangle{{side[0].second, side[1].second, side[2].second}, b / a, c / a});
    }
}

void vote_pairs(const std::vector<Triangle>& moving, int nm, const std::vector<Triangle>& ref, int nr, double tri_tolerance,
                int min_votes, std::vector<int32_t>& pairs, std::vector<int32_t>* votes_or_null) {
    pairs.clear();
    std::vector<int32_t> own;
    std::vector<int32_t>& V = votes_or_null ? *votes_or_null : own;
    V.assign((size_t)std::max(nm, 0) * (size_t)std::max(nr, 0), 0);
    if (nm <= 0 || nr <= 0) return;
    const double tol2 = tri_tolerance * tri_tolerance;
    for (const Triangle& t : moving) {
        int best = -1;
        double bd = 0.0;
        for (size_t k = 0; k < ref.size(); k++) {
            const double d0 = t.ba - ref[k].ba, d1 = t.ca - ref[k].ca;
            const double d = d0 * d0 + d1 * d1;
            if (best < 0 || d < bd) { best = (int)k; bd = d; }
        }
        if (best < 0 || !(bd <= tol2)) continue;
        for (int q = 0; q < 3; q++) V[(size_t)t.v[q] * nr + ref[best].v[q]] += 1;
    }
    std::vector<int> col_best(nr, 0);                         // argmax of every column, lowest i on ties
    for (int j = 0; j < nr; j++)
        for (int i = 1; i < nm; i++)
            if (V[(size_t)i * nr + j] > V[(size_t)col_best[j] * nr + j]) col_best[j] = i;
    for (int i = 0; i < nm; i++) {
        int j = 0;
        for (int q = 1; q < nr; q++) if (V[(size_t)i * nr + q] > V[(size_t)i * nr + j]) j = q;
        if (V[(size_t)i * nr + j] >= min_votes && col_best[j] == i) { pairs.push_back(i); pairs.push_back(j); }
    }
}

void guided_pairs(const stk_star* moving, int n_moving, const stk_star* ref, int n_ref, const double* H, double thr,
                  std::vector<int32_t>& pairs) {
    pairs.clear();
    if (n_moving <= 0 || n_ref <= 0) return;
    std::vector<double> X(n_moving), Y(n_moving);
    for (int i = 0; i < n_moving; i++) {
        const double x = moving[i].x, y = moving[i].y;
        const double den = H[6] * x + H[7] * y + H[8];
        X[i] = (H[0] * x + H[1] * y + H[2]) / den;
        Y[i] = (H[3] * x + H[4] * y + H[5]) / den;
    }
    // a distance that is not finite counts as infinite
    auto d = [&](int i, int j) {
        const double dx = (double)ref[j].x - X[i], dy = (double)ref[j].y - Y[i];
        const double v = std::sqrt(dx * dx + dy * dy);
        return std::isfinite(v) ? v : INFINITY;
    };
    std::vector<int> back(n_ref, 0);                          // nearest projected star of every reference star
    for (int j = 0; j < n_ref; j++) {
        double bd = d(0, j);
        for (int i = 1; i < n_moving; i++) { const double v = d(i, j); if (v < bd) { bd = v; back[j] = i; } }
    }
    for (int i = 0; i < n_moving; i++) {
        int j = 0;
        double bd = d(i, 0);
        for (int q = 1; q < n_ref; q++) { const double v = d(i, q); if (v < bd) { bd = v; j = q; } }
        if (bd <= thr && back[j] == i) { pairs.push_back(i); pairs.push_back(j); }
    }
}

const char* validate(const stk_star_params* p, bool* not_implemented) {
    if (not_implemented) *not_implemented = false;
    if (!p) return "null star parameters";
    if (p->radius < 2 || p->radius > 7) return "star: radius must be 2 .. 7";
    if (!std::isfinite(p->kappa) || p->kappa < 0.0f) return "star: kappa must be finite and >= 0";
    if (p->min_contrast < 1 || p->min_contrast > 255) return "star: min_contrast must be 1 .. 255";
    if (p->min_pixels < 1 || p->min_pixels > (2 * p->radius + 1) * (2 * p->radius + 1)) return "star: min_pixels must be 1 .. (2 radius + 1)^2";
    if (p->max_stars < 4 || p->max_stars > 1024) return "star: max_stars must be 4 .. 1024";
    if (p->match_stars < 4 || p->match_stars > 200) return "star: match_stars must be 4 .. 200";
    if (p->neighbours < 2 || p->neighbours > 8) return "star: neighbours must be 2 .. 8";
    if (!std::isfinite(p->tri_tolerance) || !(p->tri_tolerance > 0.0)) return "star: tri_tolerance must be finite and > 0";
    if (p->min_votes < 1) return "star: min_votes must be >= 1";
    if (p->refine != 0 && p->refine != 1) return "star: refine must be 0 or 1";
    if (p->min_stars < 4) return "star: min_stars must be >= 4";
    if (p->min_inliers < 4) return "star: min_inliers must be >= 4";
    if (p->method == STK_METHOD_RHO || (p->method >= 32 && p->method <= 38)) {
        if (not_implemented) *not_implemented = true;
        return "findHomography: RHO and the USAC methods are not implemented";
    }
    if (p->method != STK_METHOD_LEAST_SQUARES && p->method != STK_METHOD_LMEDS && p->method != STK_METHOD_RANSAC) return "star: unknown method";
    if (!std::isfinite(p->ransac_reproj_threshold) || !(p->ransac_reproj_threshold > 0.0)) return "star: ransac_reproj_threshold must be finite and > 0";
    return nullptr;
}

}  // namespace star
}  // namespace stk

extern "C" stk_status stk_star_match_lists(const stk_star* moving, int32_t n_moving, const stk_star* ref, int32_t n_ref,
                                           const stk_star_params* params, int32_t* pairs, int32_t* n_pairs) {
    using namespace stk::star;
    bool ni = false;
    if (validate(params, &ni)) return ni ? STK_NOT_IMPLEMENTED : STK_INVALID_PARAMS;
    if (n_moving < 0 || n_ref < 0 || (n_moving && !moving) || (n_ref && !ref) || !pairs || !n_pairs) return STK_INVALID_PARAMS;
    for (int i = 0; i < n_moving; i++) if (!std::isfinite(moving[i].x) || !std::isfinite(moving[i].y)) return STK_INVALID_PARAMS;
    for (int i = 0; i < n_ref; i++) if (!std::isfinite(ref[i].x) || !std::isfinite(ref[i].y)) return STK_INVALID_PARAMS;
    const int m = params->match_stars;
    std::vector<Triangle> tm, tr;
    triangles(moving, n_moving, m, params->neighbours, tm);
    triangles(ref, n_ref, m, params->neighbours, tr);
    std::vector<int32_t> pr;
    vote_pairs(tm, std::min(m, (int)n_moving), tr, std::min(m, (int)n_ref), params->tri_tolerance, params->min_votes, pr);
    for (size_t k = 0; k < pr.size(); k++) pairs[k] = pr[k];
    *n_pairs = (int32_t)(pr.size() / 2);
    return STK_OK;
}
