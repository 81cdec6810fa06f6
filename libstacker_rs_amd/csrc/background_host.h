// background_host.h — the host half of the background model (include/stacker.h, stk_background_params): the parameter
// checks, the node grid with its windows, and the estimator that turns one frame's window records into its level and rms
// planes. Inline, no HIP type and no stk_ctx, so that a host-only program can call them
// (tests/sanitize/background_harness.cpp); background.cpp exports the estimator as stk_background_estimate. f64 and f32 as
// the definition says, each operation rounded on its own (-ffp-contract=off): only + - x / and sqrt, so that a numpy
// restatement (tests/background_restate.py) matches bit for bit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/stacker.h"

namespace stk {
namespace bg {

inline bool step_ok(int step) { return step == 16 || step == 32 || step == 64 || step == 128; }

// null when the parameters are in range, else what is wrong with them; f32: the frames are f32 (f32_scale is read)
inline const char* validate(const stk_background_params* p, bool f32) {
    if (!p) return "null background parameters";
    if (!step_ok(p->step)) return "background: step must be 16, 32, 64 or 128";
    if (p->clip_iters < 0 || p->clip_iters > 5) return "background: clip_iters must be 0 .. 5";
    if (!std::isfinite(p->kappa) || !(p->kappa > 0.0f)) return "background: kappa must be finite and > 0";
    if (f32 && (!std::isfinite(p->f32_scale) || !(p->f32_scale > 0.0f))) return "background: f32_scale must be finite and > 0";
    if (p->estimator < STK_BG_MEDIAN || p->estimator > STK_BG_MODE) return "background: estimator must be 0 (median), 1 (mean) or 2 (mode)";
    if (p->min_count < 0) return "background: min_count must be >= 0";
    if (!(p->max_reject >= 0.0f && p->max_reject <= 1.0f)) return "background: max_reject must be 0 .. 1";
    if (p->recentre != 0 && p->recentre != 1) return "background: recentre must be 0 or 1";
    if (p->filter != 0 && p->filter != 1) return "background: filter must be 0 or 1";
    if (p->fill < 0 || p->fill > 16) return "background: fill must be 0 .. 16";
    for (int c = 0; c < 4; c++)
        if (!std::isfinite(p->target[c])) return "background: target must be finite";
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return "background parameters: reserved must be 0";
    return nullptr;
}

// nodes of stk_mesh_grid along one axis
inline int grid_nodes(int size, int step) { return (size - 1 + step - 1) / step + 1; }
// the window of node k along one axis: [a, b], empty when a > b
inline void window(int k, int step, int size, int& a, int& b) {
    const int q = k * step;
    a = std::max(q - step / 2, 0);
    b = std::min(q + step / 2, size - 1);
}

// `passes` Jacobi passes of the mesh section's Fill on one channel's values (nn = gw gh) with validity m
inline void fill(std::vector<float>& A, std::vector<uint8_t>& m, int gw, int gh, int passes) {
    const int nn = gw * gh;
    std::vector<float> B(A.size());
    std::vector<uint8_t> mb(m.size());
    for (int pass = 0; pass < passes; pass++) {
        for (int i = 0; i < nn; i++) {
            const int j = i / gw, k = i - j * gw;
            float d = A[i];
            uint8_t ok = m[i];
            if (!ok) {
                float den = 0.0f, num = 0.0f;
                for (int dj = -1; dj <= 1; dj++)
                    for (int dk = -1; dk <= 1; dk++) {
                        const int jj = j + dj, kk = k + dk;
                        if ((unsigned)jj >= (unsigned)gh || (unsigned)kk >= (unsigned)gw) continue;
                        const int q = jj * gw + kk;
                        if (!m[q]) continue;
                        const float wgt = (float)((2 - (dj < 0 ? -dj : dj)) * (2 - (dk < 0 ? -dk : dk)));
                        den = den + wgt;
                        num = num + wgt * A[q];
                    }
                if (den > 0.0f) { d = num / den; ok = 1; }
            }
            B[i] = d; mb[i] = ok;
        }
        A.swap(B); m.swap(mb);
    }
}

// the lower median of the values whose validity is set; false when there is none
inline bool lower_median(const std::vector<float>& A, const std::vector<uint8_t>& m, float* out) {
    std::vector<float> v;
    for (size_t i = 0; i < A.size(); i++)
        if (m[i]) v.push_back(A[i]);
    if (v.empty()) return false;
    std::sort(v.begin(), v.end());
    *out = v[(v.size() + 1) / 2 - 1];
    return true;
}

// stk_background_estimate
inline stk_status estimate(int width, int height, int channels, int depth, const stk_background_params* p, const stk_bg_cell* cells,
                           float* level, float* rms_out, int32_t* valid_out, int32_t* flags_out) {
    if (width <= 0 || height <= 0 || (channels != 1 && channels != 3 && channels != 4) || (depth != 8 && depth != 16 && depth != 32) ||
        validate(p, depth == 32) || !cells || !level)
        return STK_INVALID_PARAMS;
    const int C = std::min(channels, 3), step = p->step;
    const int gw = grid_nodes(width, step), gh = grid_nodes(height, step), nn = gw * gh;
    const double min_count = (double)(p->min_count ? p->min_count : 64);
    // window centres p and node positions q along both axes; an empty window's centre is never read (its nodes are invalid)
    std::vector<double> px(gw), py(gh);
    for (int k = 0; k < gw; k++) { int a, b; window(k, step, width, a, b); px[k] = ((double)a + (double)b) / 2.0; }
    for (int j = 0; j < gh; j++) { int a, b; window(j, step, height, a, b); py[j] = ((double)a + (double)b) / 2.0; }
    int flags = 0;
    if (valid_out) std::fill(valid_out, valid_out + nn, 0);
    std::vector<double> L(nn), L1(nn), R(nn);
    std::vector<float> A(nn), F(nn), RA(nn);
    std::vector<uint8_t> ok(nn), okr(nn);
    for (int c = 0; c < C; c++) {
        for (int i = 0; i < nn; i++) {
            const stk_bg_cell& r = cells[(size_t)i * C + c];
            double lev = 0.0, rms = 0.0;
            if (r.kept > 0) {
                const double kept = (double)r.kept, med = (double)r.med;
                const double mean = (double)r.sum / kept;
                lev = med;
                if (p->estimator == STK_BG_MEAN) lev = mean;
                else if (p->estimator == STK_BG_MODE) {
                    const double s = 1.4826 * (double)std::max(r.mad, 1);
                    if (std::fabs(mean - med) <= 0.3 * s) lev = 2.5 * med - 1.5 * mean;
                }
                rms = std::sqrt(std::max((double)r.sum2 / kept - mean * mean, 0.0));
            }
            L[i] = lev; R[i] = rms;
            ok[i] = (double)r.kept >= min_count && (double)(r.n - r.kept) <= (double)p->max_reject * (double)r.n;
            if (valid_out && ok[i]) valid_out[i] |= 1 << c;
        }
        // 1. recentre: x on the input values, then y on the x pass's output
        if (p->recentre) {
            L1 = L;
            for (int j = 0; j < gh; j++)
                for (int k = 0; k < gw; k++) {
                    const int i = j * gw + k;
                    const double q = (double)(k * step);
                    if (!ok[i] || px[k] == q) continue;
                    const int kn = px[k] > q ? k + 1 : k - 1;
                    if (kn < 0 || kn >= gw || !ok[j * gw + kn] || px[kn] == px[k]) continue;
                    L1[i] = L[i] + ((L[i] - L[j * gw + kn]) * (q - px[k])) / (px[k] - px[kn]);
                }
            L = L1;
            for (int j = 0; j < gh; j++)
                for (int k = 0; k < gw; k++) {
                    const int i = j * gw + k;
                    const double q = (double)(j * step);
                    if (!ok[i] || py[j] == q) continue;
                    const int jn = py[j] > q ? j + 1 : j - 1;
                    if (jn < 0 || jn >= gh || !ok[jn * gw + k] || py[jn] == py[j]) continue;
                    L[i] = L1[i] + ((L1[i] - L1[jn * gw + k]) * (q - py[j])) / (py[j] - py[jn]);
                }
        }
        // 2. sample units, f32
        for (int i = 0; i < nn; i++) {
            double lev = L[i], rms = R[i];
            if (depth == 32) { lev = lev / (double)p->f32_scale; rms = rms / (double)p->f32_scale; }
            A[i] = (float)lev; RA[i] = (float)rms;
        }
        okr = ok;
        // 3. the 3 x 3 median of wholly valid neighbourhoods, on the input values
        if (p->filter) {
            F = A;
            for (int j = 1; j + 1 < gh; j++)
                for (int k = 1; k + 1 < gw; k++) {
                    float v[9];
                    bool all = true;
                    for (int dj = -1; dj <= 1; dj++)
                        for (int dk = -1; dk <= 1; dk++) {
                            const int q = (j + dj) * gw + k + dk;
                            all = all && ok[q];
                            v[(dj + 1) * 3 + dk + 1] = A[q];
                        }
                    if (!all) continue;
                    std::sort(v, v + 9);
                    F[j * gw + k] = v[4];
                }
            A = F;
        }
        // 4. the last column, then the last row
        if (gw >= 3)
            for (int j = 0; j < gh; j++) {
                const int i = j * gw + gw - 1;
                if (ok[i] || !ok[i - 1] || !ok[i - 2]) continue;
                A[i] = (A[i - 1] + A[i - 1]) - A[i - 2];
                ok[i] = 1;
            }
        if (gh >= 3)
            for (int k = 0; k < gw; k++) {
                const int i = (gh - 1) * gw + k;
                if (ok[i] || !ok[i - gw] || !ok[i - 2 * gw]) continue;
                A[i] = (A[i - gw] + A[i - gw]) - A[i - 2 * gw];
                ok[i] = 1;
            }
        // 5. and 6. fill, then the fallback from the values before the fill
        float fall = 0.0f, rfall = 0.0f;
        if (!lower_median(A, ok, &fall)) flags |= 1 << c;
        lower_median(RA, okr, &rfall);
        fill(A, ok, gw, gh, p->fill);
        for (int i = 0; i < nn; i++) level[(size_t)i * C + c] = ok[i] ? A[i] : fall;
        if (rms_out) {
            fill(RA, okr, gw, gh, p->fill);
            for (int i = 0; i < nn; i++) rms_out[(size_t)i * C + c] = okr[i] ? RA[i] : rfall;
        }
    }
    if (flags_out) *flags_out = flags;
    return STK_OK;
}

}  // namespace bg
}  // namespace stk
