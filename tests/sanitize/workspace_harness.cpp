// workspace_harness.cpp — the host back end of the combines (libstacker_rs_amd/csrc/workspace.h) under ASan + UBSan
// (tests/test_cpu_sanitize.py): the carver, every layout built through it, and the one way to finish a combine. A region
// one element short shows up on a GPU only as a wrong pixel or a fault; a copy-back one byte long is a heap overrun in the
// caller's array that no comparison of results can see. Here every region is checked against the bytes its users need,
// stated from the element counts, and the host outputs are heap blocks of exactly the size the C ABI documents.
#include "hip_stubs.h"

#include <cstdio>
#include <string>
#include <vector>

static int g_stamp = 0;
extern "C" {
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { *reinterpret_cast<int*>(e) = ++g_stamp; return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    *ms = 0.5f * (float)(*reinterpret_cast<int*>(b) - *reinterpret_cast<int*>(a));
    return hipSuccess;
}
}

#include "../../libstacker_rs_amd/csrc/context.h"

float ev_ms(hipEvent_t a, hipEvent_t b) { float ms = 0; (void)hipEventElapsedTime(&ms, a, b); return ms; }      // (stacker.cpp's)

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("  [%s]\n", #cond); failures++; } } while (0)

// the sizes the hand-written offsets below are computed with
static_assert(sizeof(stk_frame_weight) == 40 && sizeof(stk::WarpFrame) == 120 && sizeof(stk::RejectEntry) == 168 && sizeof(void*) == 8, "sizes");

struct Region { const char* name; size_t at, need; size_t align = 256; };

// aligned, inside [0, total), pairwise disjoint over the bytes the users need
static void check_regions(const std::string& what, size_t total, const std::vector<Region>& r) {
    for (size_t i = 0; i < r.size(); i++) {
        CHECK(r[i].at % r[i].align == 0, "%s: %s at %zu is not aligned", what.c_str(), r[i].name, r[i].at);
        CHECK(r[i].at + r[i].need <= total, "%s: %s [%zu, +%zu) ends behind the total %zu", what.c_str(), r[i].name, r[i].at, r[i].need, total);
        for (size_t j = 0; j < i; j++) {
            if (!r[i].need || !r[j].need) continue;
            CHECK(r[i].at + r[i].need <= r[j].at || r[j].at + r[j].need <= r[i].at, "%s: %s [%zu, +%zu) overlaps %s [%zu, +%zu)", what.c_str(),
                  r[i].name, r[i].at, r[i].need, r[j].name, r[j].at, r[j].need);
        }
    }
}
static void add_planes(std::vector<Region>& r, const char* name, size_t at, size_t stride, size_t n, size_t need) {
    for (size_t k = 0; k < n; k++) r.push_back({name, at + k * stride, need});
}
static std::string tag(const char* name, std::initializer_list<long long> v) {
    std::string s = name;
    for (long long x : v) s += " " + std::to_string(x);
    return s;
}

static void test_carver() {
    Carver c(1000);                                      // a start that is no multiple of 256
    CHECK(c.total == 1024, "carver: start 1000 -> %zu", c.total);
    const size_t sizes[] = {0, 1, 256, 257, 0, 5};
    const size_t want[] = {1024, 1024, 1280, 1536, 2048, 2048};
    for (int k = 0; k < 6; k++) {
        const size_t at = c.take(sizes[k]);
        CHECK(at == want[k], "carver: take(%zu) -> %zu, want %zu", sizes[k], at, want[k]);
    }
    CHECK(c.total == 2304, "carver: total %zu", c.total);
    CHECK(c.spans.size() == 6, "carver: %zu spans", c.spans.size());
    for (size_t k = 0; k < c.spans.size(); k++) {
        CHECK(c.spans[k].first == want[k] && c.spans[k].second == sizes[k], "carver: span %zu = (%zu, %zu)", k, c.spans[k].first, c.spans[k].second);
        CHECK(c.spans[k].first % 256 == 0, "carver: span %zu not aligned", k);
        if (k) CHECK(c.spans[k].first >= c.spans[k - 1].first + c.spans[k - 1].second, "carver: span %zu overlaps the one before", k);
    }
    CHECK(c.total == c.spans.back().first + up256(c.spans.back().second), "carver: total is not the end of the last span");
    CHECK(Carver().total == 0 && Carver(256).total == 256 && Carver(257).total == 512, "carver: start rounding");
    CHECK(up256(0) == 0 && up256(1) == 256 && up256(256) == 256 && up256(257) == 512, "up256");
}

static void test_layouts() {
    const int ns[] = {0, 1, 2, 5}, whs[][2] = {{1, 1}, {17, 9}, {64, 64}}, cns[] = {1, 3, 4}, steps[] = {8, 16};
    const size_t FW = sizeof(stk_frame_weight), P8 = sizeof(void*);
    for (int n : ns) for (auto& wh : whs) {
        const int w = wh[0], h = wh[1];
        const size_t un = (size_t)n, px = (size_t)w * h;
        for (int cn : {0, 1, 3, 4}) for (size_t np : {(size_t)0, (size_t)3}) {
            const LocalLayout L = local_layout(un, n, w, h, cn, np);
            std::vector<Region> r = {{"fptrs", L.fptrs, un * P8}, {"mptrs", L.mptrs, un * P8}, {"coef", L.coef, cn ? un * FW : 0},
                                     {"image", L.image, px * cn * 4}, {"den", L.den, cn ? px * 4 : 0}};
            add_planes(r, "plane", L.planes, L.plane, np, px * 4);
            check_regions(tag("local", {n, w, h, cn, (long long)np}), L.total, r);
        }
        for (int cn : cns) {
            const size_t nel = px * cn;
            const ClipLayout C = clip_layout(nel);
            check_regions(tag("clip", {w, h, cn}), C.total, {{"c", C.c, nel * 4, 4}, {"L", C.L, nel * 4, 4}, {"U", C.U, nel * 4, 4}});
            for (size_t R : {(size_t)1, (size_t)h}) for (int counts = 0; counts < 2; counts++) {
                const QuantileLayout Q = quantile_layout(n, R, w, h, cn, counts != 0);
                check_regions(tag("quantile", {n, (long long)R, w, h, cn, counts}), Q.total,
                              {{"image", Q.image, nel * 4}, {"band", Q.band, R * un * w * cn * 4}, {"counts", Q.counts, counts ? px * 4 : 0}});
            }
            for (int step : {0, 4}) {
                const WeightedLayout L = weighted_layout(n, w, h, cn, step);
                const size_t moving = n > 1 ? un - 1 : 0;
                const size_t parts = step > 0 ? stk::moments_plan(w, h, step).parts() * moving * (1 + 5 * cn) * 8 : 0;
                check_regions(tag("weighted", {n, w, h, cn, step}), L.total,
                              {{"image", L.image, nel * 4}, {"den", L.den, px * 4}, {"coef", L.coef, un * FW},
                               {"moments", L.moments, moving * cn * 6 * 8}, {"partials", L.partials, parts}});
            }
            for (int clean = 0; clean < 2; clean++) for (int counts = 0; counts < 2; counts++) for (size_t np : {(size_t)0, (size_t)3}) {
                const RejectLayout L = reject_layout(n, w, h, cn, clean != 0, counts != 0, np);
                std::vector<Region> r = {{"entries", L.entries, un * sizeof(stk::RejectEntry)}, {"tallies", L.tallies, un * 2 * 8},
                                         {"clean", L.clean, clean ? nel * 4 : 0}, {"counts", L.counts, counts ? px * 4 : 0}};
                add_planes(r, "plane", L.planes, L.plane, np, px * 4);
                check_regions(tag("reject", {n, w, h, cn, clean, counts, (long long)np}), L.total, r);
            }
            for (size_t pre : {(size_t)0, nel * 4}) for (int host = 0; host < 2; host++) for (size_t np : {(size_t)0, (size_t)3}) {
                const int ow = 2 * w, oh = 2 * h;
                const DrizzleLayout L = drizzle_layout(pre, n, w, h, ow, oh, cn, host != 0, np);
                std::vector<Region> r = {{"mean", 0, pre}, {"foot", L.foot, un * 2 * 4}, {"coef", L.coef, un * FW}, {"mptrs", L.mptrs, un * P8},
                                         {"image", L.image, host ? (size_t)ow * oh * cn * 4 : 0}, {"den", L.den, host ? (size_t)ow * oh * 4 : 0}};
                add_planes(r, "plane", L.planes, L.plane, np, px * 4);
                check_regions(tag("drizzle", {(long long)pre, n, w, h, cn, host, (long long)np}), L.total, r);
            }
            for (int step : steps) {
                const NodeGrid g = node_grid(w, h, step);
                for (int cells = 0; cells < 2; cells++) for (int planes = 0; planes < 2; planes++) {
                    const NormLayout L = norm_layout(n, w, h, cn, g, cells != 0, planes != 0);
                    std::vector<Region> r = {{"ptrs", L.ptrs, un * P8}, {"coef", L.coef, un * FW}, {"image", L.image, nel * 4}, {"den", L.den, px * 4},
                                             {"cells", L.cells, cells && n > 1 ? (un - 1) * g.cells() * cn * 6 * 8 : 0}};
                    add_planes(r, "plane", L.planes, L.plane, planes ? un : 0, g.nodes() * 2 * cn * 4);
                    check_regions(tag("norm", {n, w, h, cn, step, cells, planes}), L.total, r);
                }
                const size_t nn = g.nodes();
                for (int mask = 0; mask < 16; mask++) {          // fields, status, scratch, image: each both ways
                    const size_t nf = mask & 1 ? un : 0, nst = mask & 2 ? un : 0, nsc = mask & 4 ? un : 0, img = mask & 8 ? nel : 0;
                    const MeshLayout L = mesh_layout(un, nf, nst, nsc, g.gw, g.gh, img);
                    std::vector<Region> r = {{"tptrs", L.tptrs, un * P8}, {"fptrs", L.fptrs, un * P8}, {"sptrs", L.sptrs, un * P8}, {"image", L.image, img * 4}};
                    add_planes(r, "field", L.fields, L.fplane, nf, nn * 2 * 4);
                    add_planes(r, "status", L.status, L.splane, nst, nn * 4);
                    add_planes(r, "scratch", L.scratch, L.cplane, nsc, nn * (2 * 4 + 2));   // a copy of the field and two validity bytes per node
                    check_regions(tag("mesh", {n, w, h, cn, step, mask}), L.total, r);
                    for (int levels : {1, 3}) {
                        if ((step >> (levels - 1)) < 4 || (std::min(w, h) >> (levels - 1)) < 16) continue;     // pyr_validate refuses
                        const PyrLayout P = pyr_layout(L.total, un, g.gw, g.gh, w, h, levels);
                        std::vector<Region> q = r;
                        q.push_back({"vptrs", P.vptrs, un * P8});
                        add_planes(q, "valid", P.valid, P.vplane, un, nn);
                        add_planes(q, "pyramid", P.planes, P.pstride, un, stk::mesh_pyr_offset(w, h, levels));
                        add_planes(q, "table", P.tables, P.tbytes, (size_t)(levels - 1), un * sizeof(stk::WarpFrame));
                        check_regions(tag("pyramid", {n, w, h, cn, step, mask, levels}), P.total, q);
                    }
                }
            }
        }
    }
}

// One grid point per layout against offsets written out by hand from the formulas of commit 54dc8f0 ("Fold Y into the
// Jacobian before the ECC homography moment sums"), the last one that carved each layout with its own chain of
// L.x = L.y + up(...). 5 entries of 17 x 9 x 3: an image is 1836 -> 2048 bytes, a w x h plane 612 -> 768.
#define SAME(expr, want) CHECK((expr) == (size_t)(want), #expr " = %zu, want %zu", (size_t)(expr), (size_t)(want))
static void test_parent_offsets() {
    const WeightedLayout W = weighted_layout(5, 17, 9, 3, 4);        // plan: 5 x 3 stepped grid, 1 x 1 workgroups, 4 partials
    SAME(W.image, 0); SAME(W.den, 2048); SAME(W.coef, 2816); SAME(W.moments, 3072); SAME(W.partials, 3840); SAME(W.total, 5888);
    SAME(weighted_layout(5, 17, 9, 3, 0).total, 3840);
    const LocalLayout L = local_layout(5, 5, 17, 9, 3, 5);
    SAME(L.fptrs, 0); SAME(L.mptrs, 256); SAME(L.coef, 512); SAME(L.image, 768); SAME(L.den, 2816); SAME(L.planes, 3584); SAME(L.plane, 768);
    SAME(L.total, 7424);
    const LocalLayout L0 = local_layout(5, 0, 17, 9, 0, 5);           // the map pass alone
    SAME(L0.coef, 512); SAME(L0.image, 512); SAME(L0.den, 512); SAME(L0.planes, 512); SAME(L0.total, 4352);
    const NodeGrid g = node_grid(17, 9, 8);
    SAME(g.gw, 3); SAME(g.gh, 2); SAME(g.cw, 3); SAME(g.ch, 2); SAME(g.shift, 3);
    const NormLayout N = norm_layout(5, 17, 9, 3, g, true, true);     // cells: 4 x 6 x 3 x 6 doubles = 3456 -> 3584; a plane: 144 -> 256
    SAME(N.ptrs, 0); SAME(N.coef, 256); SAME(N.image, 512); SAME(N.den, 2560); SAME(N.cells, 3328); SAME(N.planes, 6912); SAME(N.plane, 256);
    SAME(N.total, 8192);
    const DrizzleLayout D = drizzle_layout(1836, 5, 17, 9, 34, 18, 3, true, 2);   // image 7344 -> 7424, den 2448 -> 2560
    SAME(D.foot, 2048); SAME(D.coef, 2304); SAME(D.mptrs, 2560); SAME(D.image, 2816); SAME(D.den, 10240); SAME(D.planes, 12800); SAME(D.plane, 768);
    SAME(D.total, 14336);
    const MeshLayout M = mesh_layout(5, 4, 4, 4, 3, 2, 459);          // 6 nodes: every plane rounds to 256
    SAME(M.tptrs, 0); SAME(M.fptrs, 256); SAME(M.sptrs, 512); SAME(M.fields, 768); SAME(M.status, 1792); SAME(M.scratch, 2816); SAME(M.image, 3840);
    SAME(M.fplane, 256); SAME(M.splane, 256); SAME(M.cplane, 256); SAME(M.total, 5888);
    const PyrLayout P = pyr_layout(1000, 5, 9, 9, 64, 64, 3);         // 81 nodes; levels 1, 2: 1024 + 256 bytes; a table: 600 -> 768
    SAME(P.vptrs, 1024); SAME(P.valid, 1280); SAME(P.vplane, 256); SAME(P.planes, 2560); SAME(P.pstride, 1280); SAME(P.tables, 8960); SAME(P.tbytes, 768);
    SAME(P.total, 10496);
    const RejectLayout R = reject_layout(5, 17, 9, 3, true, true, 5);  // entries 840 -> 1024
    SAME(R.entries, 0); SAME(R.tallies, 1024); SAME(R.clean, 1280); SAME(R.counts, 3328); SAME(R.planes, 4096); SAME(R.plane, 768); SAME(R.total, 7936);
    const QuantileLayout Q = quantile_layout(5, 9, 17, 9, 3, true);    // 512 image floats, 2295 -> 2304 band floats, counts behind them
    SAME(Q.image, 0); SAME(Q.band, 2048); SAME(Q.counts, 11264); SAME(Q.total, 12032);
    const ClipLayout C = clip_layout(459);
    SAME(C.c, 0); SAME(C.L, 1836); SAME(C.U, 3672); SAME(C.total, 5508);
}

// ---------------------------------------------------------------------------------------------
struct Events {
    int slot[8] = {};
    stk_ctx ctx;
    Events() { for (int k = 0; k < 8; k++) ctx.ev[k] = reinterpret_cast<hipEvent_t>(&slot[k]); }
    // begin recorded ev[4], end ev[5] right after it, nothing else
    void check_pair(const char* what) {
        CHECK(slot[4] > 0 && slot[5] == slot[4] + 1, "%s: ev[4] at %d, ev[5] at %d", what, slot[4], slot[5]);
        for (int k = 0; k < 8; k++) if (k != 4 && k != 5) CHECK(slot[k] == 0, "%s: ev[%d] recorded", what, k);
    }
};
template <typename T> static T* block(size_t n, T fill) { T* p = new T[n]; for (size_t i = 0; i < n; i++) p[i] = fill; return p; }

static void test_outputs(int w, int h, int cn) {
    const size_t px = (size_t)w * h, nel = px * cn;
    const std::string what = tag("outputs", {w, h, cn});
    for (int location : {(int)STK_HOST, (int)STK_DEVICE}) for (int with_sides = 0; with_sides < 2; with_sides++) {
        const bool host = location != STK_DEVICE;
        // the clip forms: the staging copies are the clip planes themselves (c, L, U); counts and kept have nel elements
        {
            Events e;
            const ClipLayout C = clip_layout(nel);
            char* planes = new char[C.total];
            float *c = (float*)(planes + C.c), *U = (float*)(planes + C.U);
            int32_t* Lc = (int32_t*)(planes + C.L);
            float* image = block<float>(nel, -1.0f);
            int32_t* counts = with_sides ? block<int32_t>(nel, -1) : nullptr;
            float* kept = with_sides ? block<float>(nel, -1.0f) : nullptr;
            stk_image_f32 out{image, w, h, cn, location, 0};
            const CombineOutputs o(&out, c, nel, {counts, planes + C.L, nel}, {kept, planes + C.U, nel});
            CHECK(o.image() == (host ? c : image), "%s: image dst", what.c_str());
            CHECK(o.side<int32_t>(0) == (!with_sides ? nullptr : host ? Lc : counts), "%s: counts dst", what.c_str());
            CHECK(o.side<float>(1) == (!with_sides ? nullptr : host ? U : kept), "%s: kept dst", what.c_str());
            for (size_t i = 0; i < nel; i++) { c[i] = (float)i; Lc[i] = (int32_t)(7 * i); U[i] = 0.5f * (float)i; }   // "the kernel" wrote the planes
            double ms = 2.0;
            CHECK(combine_begin(&e.ctx) == STK_OK && combine_end(&e.ctx, &ms, &o) == STK_OK, "%s: begin / end failed", what.c_str());
            e.check_pair(what.c_str());
            CHECK(ms == 2.5, "%s: ms = %g, want 2 + 0.5", what.c_str(), ms);
            for (size_t i = 0; i < nel; i++) {
                CHECK(image[i] == (host ? (float)i : -1.0f), "%s: image[%zu] = %g (location %d)", what.c_str(), i, image[i], location);
                if (with_sides) CHECK(counts[i] == (host ? (int32_t)(7 * i) : -1) && kept[i] == (host ? 0.5f * (float)i : -1.0f), "%s: side planes at %zu", what.c_str(), i);
            }
            delete[] planes; delete[] image; delete[] counts; delete[] kept;
        }
        // the folds and the quantile: staging regions of a layout; the side planes have w x h elements (den f32, counts int32)
        {
            Events e;
            const QuantileLayout Q = quantile_layout(2, 1, w, h, cn, host && with_sides);
            const WeightedLayout W = weighted_layout(2, w, h, cn, 0);
            char* qs = new char[Q.total];
            char* ws = new char[W.total];
            float* image = block<float>(nel, -1.0f);
            int32_t* counts = with_sides ? block<int32_t>(px, -1) : nullptr;
            float* den = with_sides ? block<float>(px, -1.0f) : nullptr;
            stk_image_f32 out{image, w, h, cn, location, 0};
            const CombineOutputs oq(&out, (float*)(qs + Q.image), nel, {counts, qs + Q.counts, px});
            const CombineOutputs ow(&out, (float*)(ws + W.image), nel, {den, ws + W.den, px});
            CHECK(oq.side<int32_t>(0) == (!with_sides ? nullptr : host ? (int32_t*)(qs + Q.counts) : counts), "%s: quantile counts dst", what.c_str());
            CHECK(ow.side<float>(0) == (!with_sides ? nullptr : host ? (float*)(ws + W.den) : den), "%s: den dst", what.c_str());
            CHECK(oq.side<float>(1) == nullptr && ow.side<float>(1) == nullptr, "%s: an absent side plane has a destination", what.c_str());
            for (size_t i = 0; i < nel; i++) { oq.image()[i] = host ? 3.0f : -1.0f; }
            if (with_sides) for (size_t i = 0; i < px; i++) oq.side<int32_t>(0)[i] = host ? 9 : -1;
            CHECK(combine_begin(&e.ctx) == STK_OK && combine_end(&e.ctx, nullptr, &oq) == STK_OK, "%s: quantile begin / end failed", what.c_str());
            for (size_t i = 0; i < nel; i++) CHECK(image[i] == (host ? 3.0f : -1.0f), "%s: quantile image[%zu]", what.c_str(), i);
            if (with_sides) for (size_t i = 0; i < px; i++) CHECK(counts[i] == (host ? 9 : -1), "%s: quantile counts[%zu]", what.c_str(), i);
            for (size_t i = 0; i < nel; i++) ow.image()[i] = host ? 4.0f : -1.0f;
            if (with_sides) for (size_t i = 0; i < px; i++) ow.side<float>(0)[i] = host ? 5.0f : -1.0f;
            CHECK(combine_begin(&e.ctx) == STK_OK && combine_end(&e.ctx, nullptr, &ow) == STK_OK, "%s: fold begin / end failed", what.c_str());
            for (size_t i = 0; i < nel; i++) CHECK(image[i] == (host ? 4.0f : -1.0f), "%s: fold image[%zu]", what.c_str(), i);
            if (with_sides) for (size_t i = 0; i < px; i++) CHECK(den[i] == (host ? 5.0f : -1.0f), "%s: den[%zu]", what.c_str(), i);
            delete[] qs; delete[] ws; delete[] image; delete[] counts; delete[] den;
        }
    }
    // a table the host reads back (moments: doubles), and the pair alone (the field pass has no output)
    Events e;
    const size_t n = nel * 6;
    double* dev = block<double>(n, 1.25);
    double* host = block<double>(n, 0.0);
    const CombineOutputs t(host, dev, n, sizeof(double));
    double ms = 0.0;
    CHECK(combine_begin(&e.ctx) == STK_OK && combine_end(&e.ctx, &ms, &t) == STK_OK, "%s: table begin / end failed", what.c_str());
    for (size_t i = 0; i < n; i++) CHECK(host[i] == 1.25, "%s: table[%zu]", what.c_str(), i);
    CHECK(combine_begin(&e.ctx) == STK_OK && combine_end(&e.ctx, &ms) == STK_OK && ms == 1.0, "%s: the pair alone, ms = %g", what.c_str(), ms);
    delete[] dev; delete[] host;
}

int main() {
    test_carver();
    test_layouts();
    test_parent_offsets();
    test_outputs(17, 9, 3);
    test_outputs(1, 1, 4);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
