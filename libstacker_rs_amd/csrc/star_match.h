// star_match.h — the host half of star registration (include/stacker.h, stk_star_params, "Matching"): triangles of a
// star list, votes, pairs, the guided re-match under a homography, and the parameter checks. It includes no HIP type and
// no stk_ctx, like combine.h's selection rules, so a host-only program can call it
// (tests/sanitize/star_match_harness.cpp). All arithmetic is f64 on the stars' f32 coordinates; a distance is
// sqrt(dx*dx + dy*dy); the library is built with -ffp-contract=off.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/stacker.h"

namespace stk {
namespace star {

struct Triangle {
    int v[3];            // vertices opposite the sides a >= b >= c
    double ba, ca;       // the descriptor (b / a, c / a)
};

// step 1: the triangles of the first min(match_stars, count) stars of `s`, in the order of their sorted index triples
void triangles(const stk_star* s, int count, int match_stars, int neighbours, std::vector<Triangle>& out);
// steps 2 and 3: votes of the moving triangles for the reference triangles, then the mutual-best pairs with at least
// min_votes, as (moving index, reference index) in ascending moving index. nm, nr: the stars the triangles were built on.
// votes_or_null: the nm x nr matrix, for tests
void vote_pairs(const std::vector<Triangle>& moving, int nm, const std::vector<Triangle>& ref, int nr, double tri_tolerance,
                int min_votes, std::vector<int32_t>& pairs, std::vector<int32_t>* votes_or_null = nullptr);
// step 5: all moving stars projected by H (row-major 3 x 3) against all reference stars: mutual nearest within thr
void guided_pairs(const stk_star* moving, int n_moving, const stk_star* ref, int n_ref, const double* H, double thr,
                  std::vector<int32_t>& pairs);
// the checks of include/stacker.h; null = fine, else the message. *not_implemented: the method is RHO or a USAC one
const char* validate(const stk_star_params* p, bool* not_implemented);

}  // namespace star
}  // namespace stk
