// hg_batch_harness.cpp — the whole host driver of findHomography (homography.cpp: find_homography_batch) under ASan + UBSan,
// end to end, over random mixed batches. The two device launches are replaced by plain scalar stand-ins written for this
// harness: the model launch fits every sample by Gaussian elimination and scores it through exactly the offsets the driver
// put into HgFrame; the refinement launch reports back what it was asked (winning sample, threshold, mode), so that the
// driver's decisions can be held against the textbook sequential loop run here with the same scorer. Checked:
//   * the layout the driver hands to the launches (point ranges, the tiling of the sample / score / error regions);
//   * speculation in rounds == the sequential RANSAC / LMEDS loop (winner, mode, threshold, inlier count, models evaluated);
//   * problem i of a batch == that problem alone, on every field and on the masks.
#include "hip_stubs.h"
#include "../../libstacker_rs_amd/csrc/homography.cpp"

#include <cstdarg>
#include <cstdio>
#include <random>

using namespace stk::geom;

namespace {

[[noreturn]] void die(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\nFAILED\n");
    std::exit(1);
}

// what the call under way must hand to the launches
struct Expect {
    std::vector<int> pt_ofs, n;      // of the problems that reach the device, in order
    size_t n_points = 0;
    int lmeds = 0;
    float thr2 = 0;
    int model_launches = 0, refine_launches = 0;
} g_exp;

// ---- the scorer: the homography through four correspondences, h8 = 1, by Gaussian elimination with partial pivoting ----
bool fit_four(const HgPoint s[4], double H[9]) {
    double A[8][9];
    for (int k = 0; k < 4; k++) {
        const double X = s[k].Mx, Y = s[k].My, x = s[k].mx, y = s[k].my;
        const double r0[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, x}, r1[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, y};
        for (int c = 0; c < 9; c++) { A[2 * k][c] = r0[c]; A[2 * k + 1][c] = r1[c]; }
    }
    for (int col = 0; col < 8; col++) {
        int piv = col;
        for (int r = col + 1; r < 8; r++) if (std::fabs(A[r][col]) > std::fabs(A[piv][col])) piv = r;
        if (!(std::fabs(A[piv][col]) > 1e-12)) return false;
        if (piv != col) for (int c = 0; c < 9; c++) std::swap(A[piv][c], A[col][c]);
        for (int r = col + 1; r < 8; r++) {
            const double f = A[r][col] / A[col][col];
            for (int c = col; c < 9; c++) A[r][c] -= f * A[col][c];
        }
    }
    for (int r = 7; r >= 0; r--) {
        double v = A[r][8];
        for (int c = r + 1; c < 8; c++) v -= A[r][c] * H[c];
        H[r] = v / A[r][r];
    }
    H[8] = 1;
    for (int k = 0; k < 8; k++) if (!std::isfinite(H[k])) return false;
    return true;
}

float point_error(const double H[9], const HgPoint& p) {
    float h[8];
    for (int k = 0; k < 8; k++) h[k] = (float)H[k];
    const float w = h[6] * p.Mx + h[7] * p.My + 1.f;
    const float px = (h[0] * p.Mx + h[1] * p.My + h[2]) / w, py = (h[3] * p.Mx + h[4] * p.My + h[5]) / w;
    const float dx = px - p.mx, dy = py - p.my;
    return dx * dx + dy * dy;
}

unsigned bits_of(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

// score of one sample over P[0 .. n): the inlier count, or (LMEDS) the bits of the (n / 2)-th smallest error; -1 when the
// system is singular. err: n floats of scratch, written for LMEDS.
int score_sample(const HgPoint* P, int n, const HgSample& q, int lmeds, float thr2, float* err) {
    HgPoint s[4];
    for (int k = 0; k < 4; k++) {
        if (q.idx[k] < 0 || q.idx[k] >= n) die("sample index %d outside 0 .. %d", q.idx[k], n);
        s[k] = P[q.idx[k]];
    }
    double H[9];
    if (!fit_four(s, H)) return -1;
    if (!lmeds) {
        int count = 0;
        for (int i = 0; i < n; i++) count += point_error(H, P[i]) <= thr2;
        return count;
    }
    std::vector<unsigned> b((size_t)n);
    for (int i = 0; i < n; i++) { err[i] = point_error(H, P[i]); b[i] = bits_of(err[i]); }
    std::nth_element(b.begin(), b.begin() + n / 2, b.end());      // errors are >= +0: bit order is value order
    return (int)b[n / 2];
}

}  // namespace

namespace stk {
namespace geom {

hipError_t launch_hg_models(const HgPoint* pts, const HgFrame* frames, int n_frames, int max_hyp, const HgSample* samples,
                            int lmeds, float* err_scratch, int* scores, hipStream_t) {
    g_exp.model_launches++;
    if (lmeds != g_exp.lmeds) die("models: lmeds %d", lmeds);
    if (n_frames <= 0 || n_frames > (int)g_exp.n.size()) die("models: %d frames of %zu live problems", n_frames, g_exp.n.size());
    size_t live = 0;
    int hyp = 0, seen_max = 0;
    size_t err = 0;
    for (int f = 0; f < n_frames; f++) {
        const HgFrame& fr = frames[f];
        // the rows are the unfinished problems in their order: each one's point range is a live problem's, further on
        while (live < g_exp.n.size() && g_exp.pt_ofs[live] != fr.pt_ofs) live++;
        if (live == g_exp.n.size() || g_exp.n[live] != fr.n) die("models: row %d has points %d + %d, no live problem's", f, fr.pt_ofs, fr.n);
        live++;
        if (fr.n <= 4) die("models: row %d is a problem of %d points", f, fr.n);
        if (fr.n_hyp <= 0 || fr.n_hyp > max_hyp) die("models: row %d has %d samples, max_hyp %d", f, fr.n_hyp, max_hyp);
        if (fr.hyp_ofs != hyp) die("models: row %d samples at %d, expected %d", f, fr.hyp_ofs, hyp);
        if (lmeds && (size_t)fr.err_ofs != err) die("models: row %d errors at %d, expected %zu", f, fr.err_ofs, err);
        if (!lmeds && fr.thr2 != g_exp.thr2) die("models: row %d threshold %g, expected %g", f, (double)fr.thr2, (double)g_exp.thr2);
        hyp += fr.n_hyp;
        err += (size_t)fr.n_hyp * fr.n;
        seen_max = std::max(seen_max, fr.n_hyp);
    }
    if (seen_max != max_hyp) die("models: max_hyp %d, largest row %d", max_hyp, seen_max);
    for (int f = 0; f < n_frames; f++) {
        const HgFrame& fr = frames[f];
        for (int h = 0; h < fr.n_hyp; h++)
            scores[fr.hyp_ofs + h] = score_sample(pts + fr.pt_ofs, fr.n, samples[fr.hyp_ofs + h], lmeds, fr.thr2,
                                                  lmeds ? err_scratch + fr.err_ofs + (size_t)h * fr.n : nullptr);
    }
    return hipSuccess;
}

hipError_t launch_hg_refine(const HgPoint* pts, const HgJob* jobs, int n_frames, HgResult* results, uint8_t* masks, hipStream_t) {
    g_exp.refine_launches++;
    if (n_frames != (int)g_exp.n.size()) die("refine: %d jobs of %zu live problems", n_frames, g_exp.n.size());
    for (int k = 0; k < n_frames; k++) {
        const HgJob& j = jobs[k];
        if (j.pt_ofs != g_exp.pt_ofs[k] || j.n != g_exp.n[k]) die("refine: job %d has points %d + %d", k, j.pt_ofs, j.n);
        if (j.mode < -1 || j.mode > 1) die("refine: job %d mode %d", k, j.mode);
        HgResult r{};
        r.found = j.mode >= 0;
        for (int q = 0; q < 4; q++) r.H[q] = j.idx[q];
        r.H[4] = j.thr2;
        r.H[5] = j.mode;
        uint8_t* m = masks + j.pt_ofs;
        const HgPoint* P = pts + j.pt_ofs;
        if (j.mode == 1) {
            HgPoint s[4];
            for (int q = 0; q < 4; q++) {
                if (j.idx[q] < 0 || j.idx[q] >= j.n) die("refine: job %d sample index %d", k, j.idx[q]);
                s[q] = P[j.idx[q]];
            }
            double H[9];
            if (!fit_four(s, H)) die("refine: job %d: the winning sample has no model", k);
            for (int i = 0; i < j.n; i++) { m[i] = point_error(H, P[i]) <= j.thr2; r.n_inliers += m[i]; }
        } else {
            for (int i = 0; i < j.n; i++) m[i] = j.mode == 0;
            r.n_inliers = j.mode == 0 ? j.n : 0;
        }
        results[k] = r;
    }
    return hipSuccess;
}

}  // namespace geom
}  // namespace stk

namespace {

struct Member {
    std::vector<float> src, dst;     // exactly 2 n floats each: a read past the end is ASan's
    int n = 0;
};

Member random_member(std::mt19937& gen, int n, double frac) {
    std::uniform_real_distribution<double> U(0, 1);
    std::normal_distribution<double> N(0, 0.5);
    const double H[9] = {1 + 0.02 * (U(gen) - 0.5), 0.02 * (U(gen) - 0.5), 40 * (U(gen) - 0.5), 0.02 * (U(gen) - 0.5), 1 + 0.02 * (U(gen) - 0.5),
                         40 * (U(gen) - 0.5), 2e-5 * (U(gen) - 0.5), 2e-5 * (U(gen) - 0.5), 1};
    Member m;
    m.n = n;
    m.src.resize(2 * (size_t)n); m.dst.resize(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const double X = 1920 * U(gen), Y = 1080 * U(gen), w = H[6] * X + H[7] * Y + 1;
        m.src[2 * i] = (float)X; m.src[2 * i + 1] = (float)Y;
        m.dst[2 * i] = (float)((H[0] * X + H[1] * Y + H[2]) / w + N(gen));
        m.dst[2 * i + 1] = (float)((H[3] * X + H[4] * Y + H[5]) / w + N(gen));
    }
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::shuffle(order.begin(), order.end(), gen);
    const int k = (int)(frac * n);
    for (int q = 0; q < k; q++) {
        m.dst[2 * order[q]] += (float)(400 * (U(gen) - 0.5));
        m.dst[2 * order[q] + 1] += (float)(400 * (U(gen) - 0.5));
    }
    return m;
}

Member draw_member(std::mt19937& gen) {
    static const int sizes[] = {5, 6, 7, 5, 6, 7, 63, 64, 65, 63, 64, 65, 129, 129, 300, 300, 17, 33, 40, 1000, 4096};
    static const double fracs[] = {0, 0.3, 0.5, 0.7};
    const unsigned kind = gen() % 20;
    Member m;
    if (kind == 0) return random_member(gen, (int)(gen() % 4), 0);                  // n = 0 .. 3: never reaches the device
    if (kind == 1) return random_member(gen, 4, 0);                                 // n == 4: finished before round 0
    if (kind == 2) {                                                                // 20 collinear points: no admissible sample
        m.n = 20;
        for (int i = 0; i < 20; i++) { m.src.push_back((float)i); m.src.push_back(2.f * i); }
        m.dst = m.src;
        return m;
    }
    if (kind == 3) {                                                                // ten equal points
        m.n = 10;
        for (int i = 0; i < 10; i++) { m.src.push_back(3.f); m.src.push_back(4.f); }
        m.dst = m.src;
        return m;
    }
    unsigned pick = gen() % (sizeof(sizes) / sizeof(sizes[0]));
    if (sizes[pick] >= 1000 && gen() % 3) pick = gen() % 12;                        // the large ones cost the most: fewer of them
    return random_member(gen, sizes[pick], fracs[gen() % 4]);
}

void expect_layout(const std::vector<const Member*>& batch, int method, double thr) {
    g_exp = Expect{};
    const bool known = method == 0 || method == 4 || method == 8;
    for (const Member* m : batch) {
        if (m->n < 4 || !known) continue;
        g_exp.pt_ofs.push_back((int)g_exp.n_points);
        g_exp.n.push_back(m->n);
        g_exp.n_points += (size_t)m->n;
    }
    g_exp.lmeds = method == 4;
    const double t = thr <= 0 ? 3 : thr;
    g_exp.thr2 = (float)(t * t);
}

struct Run {
    std::vector<HgOutcome> out;
    std::vector<std::vector<uint8_t>> masks;     // exactly n bytes each
};

Run run_driver(HgWorkspace* ws, const std::vector<const Member*>& batch, int method, double thr) {
    Run r;
    std::vector<HgProblem> probs;
    r.masks.resize(batch.size());
    for (size_t i = 0; i < batch.size(); i++) {
        r.masks[i].assign((size_t)batch[i]->n, 0xAB);
        probs.push_back(HgProblem{batch[i]->src.data(), batch[i]->dst.data(), batch[i]->n, batch[i]->n ? r.masks[i].data() : nullptr});
    }
    r.out.resize(batch.size());
    for (HgOutcome& o : r.out) { o.rc = -77; o.models_evaluated = -77; }             // every outcome must be written
    expect_layout(batch, method, thr);
    const int st = find_homography_batch(nullptr, nullptr, ws, probs.data(), (int)probs.size(), method, thr, r.out.data());
    if (st != 0) die("find_homography_batch returned %d", st);
    if (g_exp.n.empty() ? (g_exp.model_launches || g_exp.refine_launches) : g_exp.refine_launches != 1)
        die("%d model and %d refinement launches for %zu live problems", g_exp.model_launches, g_exp.refine_launches, g_exp.n.size());
    return r;
}

// the sequential algorithm, as RANSACPointSetRegistrator::run / LMeDSPointSetRegistrator::run state it
struct Loop { int mode = -1; HgSample best{}; int best_count = 0; double best_median = DBL_MAX; int iterations = 0; };

Loop textbook_loop(const Member& m, int method, float thr2) {
    Loop L;
    if (method == 0 || m.n == 4) { L.mode = 0; return L; }
    const bool lmeds = method == 4;
    std::vector<HgPoint> P((size_t)m.n);
    for (int i = 0; i < m.n; i++) P[i] = HgPoint{m.src[2 * i], m.src[2 * i + 1], m.dst[2 * i], m.dst[2 * i + 1]};
    std::vector<float> err((size_t)m.n);
    HgProblem pr{m.src.data(), m.dst.data(), m.n, nullptr};
    Track t;
    t.n = m.n;
    int niters = lmeds ? iterations_needed(0.995, 0.45, 2000) : 2000, iter = 0;
    for (; iter < niters; iter++) {
        HgSample s{};
        if (!draw_sample(t, pr, s)) break;                                          // the sample stream ends
        const int sc = score_sample(P.data(), m.n, s, lmeds, thr2, err.data());
        if (sc == -1) continue;
        if (lmeds) {
            float med; std::memcpy(&med, &sc, 4);
            if ((double)med < L.best_median) { L.best_median = med; L.best = s; L.mode = 1; }
        } else if (sc > std::max(L.best_count, 3)) {
            L.best_count = sc; L.best = s; L.mode = 1;
            niters = iterations_needed(0.995, (double)(m.n - sc) / m.n, niters);
        }
    }
    L.iterations = iter;
    return L;
}

int round_end(int iterations, bool lmeds) {
    if (lmeds) return iterations_needed(0.995, 0.45, 2000);
    return iterations <= 32 ? 32 : iterations <= 288 ? 288 : 2000;
}

bool same_outcome(const HgOutcome& a, const HgOutcome& b) {
    return a.rc == b.rc && a.found == b.found && a.n_inliers == b.n_inliers && a.models_evaluated == b.models_evaluated &&
           std::memcmp(a.H, b.H, sizeof(a.H)) == 0;
}

}  // namespace

int main() {
    std::mt19937 gen(17);
    static const int methods[] = {8, 4, 0};
    static const double thrs[] = {3.0, 0.5, 12.0, 0.0, -1.0};
    HgWorkspace* shared = hg_workspace_create();             // reused by every batch: buffers larger than the call needs
    long n_problems = 0, n_robust = 0, by_round[3] = {0, 0, 0};
    for (int trial = 0; trial < 60; trial++) {
        const int method = methods[trial % 3];
        const double thr = thrs[(trial / 3) % 5];
        const int count = trial == 0 ? 1 : 1 + (int)(gen() % 40);
        std::vector<Member> members;
        for (int i = 0; i < count; i++) members.push_back(draw_member(gen));
        if (trial == 7) for (Member& m : members) m = random_member(gen, (int)(gen() % 4), 0);   // a batch that never reaches the device
        std::vector<const Member*> batch;
        for (const Member& m : members) batch.push_back(&m);
        const Run got = run_driver(shared, batch, method, thr);
        const float thr2 = g_exp.thr2;
        for (int i = 0; i < count; i++) {
            const Member& m = members[i];
            const HgOutcome& o = got.out[i];
            n_problems++;
            // ---- alone, on a workspace of its own
            HgWorkspace* own = hg_workspace_create();
            const Run one = run_driver(own, {&m}, method, thr);
            hg_workspace_destroy(own);
            if (!same_outcome(o, one.out[0]) || got.masks[i] != one.masks[0])
                die("trial %d problem %d (n %d, method %d): the batch and the single call differ", trial, i, m.n, method);
            if (m.n < 4) {
                if (o.rc != 3 || o.found || o.models_evaluated != 0) die("trial %d problem %d: n %d gives rc %d", trial, i, m.n, o.rc);
                for (uint8_t b : got.masks[i]) if (b) die("trial %d problem %d: mask of a refused problem", trial, i);
                continue;
            }
            if (o.rc != 0) die("trial %d problem %d: rc %d", trial, i, o.rc);
            // ---- against the sequential loop
            const Loop L = textbook_loop(m, method, thr2);
            if ((int)o.H[5] != L.mode || o.found != (L.mode >= 0)) die("trial %d problem %d (n %d): mode %d, the loop's %d", trial, i, m.n, (int)o.H[5], L.mode);
            if (L.mode == 0) {
                if (o.models_evaluated != 0 || o.n_inliers != m.n) die("trial %d problem %d: a plain fit evaluated %d models", trial, i, o.models_evaluated);
                for (uint8_t b : got.masks[i]) if (b != 1) die("trial %d problem %d: mask of a plain fit", trial, i);
                continue;
            }
            n_robust++;
            const bool lmeds = method == 4;
            if (o.models_evaluated < L.iterations || o.models_evaluated > round_end(L.iterations, lmeds))
                die("trial %d problem %d (n %d): %d models evaluated, the loop ran %d iterations", trial, i, m.n, o.models_evaluated, L.iterations);
            by_round[o.models_evaluated <= 32 ? 0 : o.models_evaluated <= 288 ? 1 : 2]++;
            if (L.mode < 0) {
                if (o.n_inliers != 0) die("trial %d problem %d: inliers without a model", trial, i);
                for (uint8_t b : got.masks[i]) if (b) die("trial %d problem %d: mask without a model", trial, i);
                continue;
            }
            for (int q = 0; q < 4; q++)
                if ((int)o.H[q] != L.best.idx[q]) die("trial %d problem %d (n %d): winning sample differs from the loop's", trial, i, m.n);
            float want_thr2 = thr2;
            if (lmeds) {                                     // homography.cpp: sigma = 2.5 * 1.4826 * (1 + 5 / (n - 4)) * sqrt(median)
                double sigma = 2.5 * 1.4826 * (1 + 5. / (m.n - 4)) * std::sqrt(L.best_median);
                sigma = std::max(sigma, 0.001);
                want_thr2 = (float)(sigma * sigma);
            }
            if (o.H[4] != (double)want_thr2) die("trial %d problem %d: threshold %g, the loop's %g", trial, i, o.H[4], (double)want_thr2);
            int ones = 0;
            for (uint8_t b : got.masks[i]) { if (b > 1) die("trial %d problem %d: mask byte %d", trial, i, b); ones += b; }
            if (ones != o.n_inliers || (!lmeds && ones != L.best_count))
                die("trial %d problem %d: %d mask bytes set, %d inliers, the loop's best %d", trial, i, ones, o.n_inliers, L.best_count);
        }
    }
    hg_workspace_destroy(shared);
    if (by_round[0] < 20 || by_round[1] < 20 || by_round[2] < 20) die("rounds not exercised: %ld %ld %ld", by_round[0], by_round[1], by_round[2]);
    std::printf("ok problems %ld robust %ld ending in round 0 / 1 / 2: %ld %ld %ld\n", n_problems, n_robust, by_round[0], by_round[1], by_round[2]);
    return 0;
}
