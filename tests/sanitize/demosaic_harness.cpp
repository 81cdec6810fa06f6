// demosaic_harness.cpp — the host half of the colour-filter mosaic calls (libstacker_rs_amd/csrc/demosaic_check.h, spans.h,
// workspace.h: DemosaicLayout) under ASan + UBSan (tests/test_cpu_demosaic.py): every refusal include/stacker.h names for
// stk_demosaic and stk_cfa_mask, the sizes the call works with, the overlap test that calibration shares, and the workspace
// layout. The pointers handed in are heap blocks of exactly the documented spans; the checks must not read through them.
#include "hip_stubs.h"

#include <cstdio>
#include <string>
#include <vector>

#include "../../libstacker_rs_amd/csrc/context.h"
#include "../../libstacker_rs_amd/csrc/demosaic_check.h"

using namespace stk;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("  [%s]\n", #cond); failures++; } } while (0)

struct Case {
    int n = 2, w = 7, h = 5, depth = 8, location = STK_HOST, pattern = STK_CFA_GRBG, method = STK_DEMOSAIC_MHC, out_depth = 8;
    size_t in_stride = 0, out_stride = 0;
    std::vector<std::vector<char>> planes, outs;
    std::vector<const void*> data;
    std::vector<void*> out;
    stk_mosaic m{};
    void build() {
        const size_t el = depth / 8, oel = out_depth / 8;
        const int ow = method == STK_DEMOSAIC_SUPERPIXEL ? w / 2 : w, oh = method == STK_DEMOSAIC_SUPERPIXEL ? h / 2 : h;
        const size_t is = in_stride ? in_stride : w * el, os = out_stride ? out_stride : ow * 3 * oel;
        planes.assign(n, std::vector<char>(is * (h - 1) + w * el));
        outs.assign(n, std::vector<char>(os * (oh - 1) + ow * 3 * oel));
        data.clear(); out.clear();
        for (int i = 0; i < n; i++) { data.push_back(planes[i].data()); out.push_back(outs[i].data()); }
        m = stk_mosaic{data.data(), n, w, h, depth, location, pattern, in_stride};
    }
    stk_status run(DemosaicPlan* P, std::string* why) { return demosaic_check(&m, method, out_depth, out.data(), out_stride, P, why); }
};

static void expect(const char* what, Case& c, stk_status want) {
    DemosaicPlan P{};
    std::string why;
    const stk_status got = c.run(&P, &why);
    CHECK(got == want, "%s: status %d, want %d (%s)", what, (int)got, (int)want, why.c_str());
    CHECK((got == STK_OK) == why.empty(), "%s: message '%s' with status %d", what, why.c_str(), (int)got);
}

static void test_accepts_and_sizes() {
    for (int depth : {8, 16, 32}) for (int od : {depth, 32}) for (int method = 0; method < 4; method++) for (int pad = 0; pad < 2; pad++) {
        Case c;
        c.depth = depth; c.out_depth = od; c.method = method;
        const size_t el = depth / 8, oel = od / 8;
        const int ow = method == 3 ? 3 : 7, oh = method == 3 ? 2 : 5;
        if (pad) { c.in_stride = 7 * el + 3 * el; c.out_stride = ow * 3 * oel + 5 * oel; }
        c.build();
        DemosaicPlan P{};
        std::string why;
        CHECK(c.run(&P, &why) == STK_OK, "accept %d %d %d %d: %s", depth, od, method, pad, why.c_str());
        CHECK(P.ow == ow && P.oh == oh, "plan size %d x %d", P.ow, P.oh);
        CHECK(P.in_stride == (pad ? 10 * el : 7 * el) && P.in_span == c.planes[0].size(), "plan in: stride %zu span %zu", P.in_stride, P.in_span);
        CHECK(P.out_row == ow * 3 * oel && P.out_stride == (pad ? (ow * 3 + 5) * oel : ow * 3 * oel) && P.out_span == c.outs[0].size(),
              "plan out: row %zu stride %zu span %zu", P.out_row, P.out_stride, P.out_span);
    }
    Case s; s.w = 2; s.h = 2; s.method = STK_DEMOSAIC_SUPERPIXEL; s.build(); expect("superpixel 2 x 2", s, STK_OK);
    Case t; t.w = 3; t.h = 3; t.method = STK_DEMOSAIC_HA; t.build(); expect("HA 3 x 3", t, STK_OK);
}

static void test_refusals() {
    { Case c; c.build(); DemosaicPlan P{}; std::string why;
      CHECK(demosaic_check(nullptr, 1, 8, c.out.data(), 0, &P, &why) == STK_INVALID_PARAMS && !why.empty(), "null mosaic");
      CHECK(demosaic_check(&c.m, 1, 8, nullptr, 0, &P, &why) == STK_INVALID_PARAMS, "null outputs");
      c.m.data = nullptr; expect("null table", c, STK_INVALID_PARAMS); }
    { Case c; c.build(); c.data[1] = nullptr; expect("null plane", c, STK_INVALID_PARAMS); }
    { Case c; c.build(); c.out[0] = nullptr; expect("null output", c, STK_INVALID_PARAMS); }
    { Case c; c.build(); c.m.n = 0; expect("n = 0", c, STK_INVALID_PARAMS); }
    for (int p : {-1, 4}) { Case c; c.build(); c.m.pattern = p; expect("pattern", c, STK_INVALID_PARAMS); }
    for (int me : {-1, 4}) { Case c; c.build(); c.method = me; expect("method", c, STK_INVALID_PARAMS); }
    for (int d : {0, 12, 64}) { Case c; c.build(); c.m.depth = d; expect("depth", c, STK_INVALID_PARAMS); }
    for (int l : {-1, 2}) { Case c; c.build(); c.m.location = l; expect("location", c, STK_INVALID_PARAMS); }
    { Case c; c.build(); c.out_depth = 16; expect("out_depth 16 of u8", c, STK_INVALID_PARAMS); }
    { Case c; c.depth = 32; c.out_depth = 32; c.build(); c.out_depth = 8; expect("f32 to u8", c, STK_INVALID_PARAMS); }
    { Case c; c.depth = 16; c.out_depth = 16; c.build(); c.out_depth = 8; expect("u16 to u8", c, STK_INVALID_PARAMS); }
    for (int me = 0; me < 3; me++) {
        { Case c; c.method = me; c.build(); c.m.width = 2; expect("width 2", c, STK_INVALID_PARAMS); }
        { Case c; c.method = me; c.build(); c.m.height = 2; expect("height 2", c, STK_INVALID_PARAMS); }
    }
    { Case c; c.method = 3; c.build(); c.m.width = 1; expect("superpixel width 1", c, STK_INVALID_PARAMS); }
    { Case c; c.build(); c.m.width = 1 << 16; c.m.height = 1 << 15; expect("2^31 pixels", c, STK_INVALID_PARAMS); }
    { Case c; c.build(); c.m.row_stride_bytes = 6; expect("stride below a row", c, STK_INVALID_PARAMS); }
    { Case c; c.depth = 16; c.out_depth = 16; c.build(); c.m.row_stride_bytes = 17; expect("odd stride of u16", c, STK_INVALID_PARAMS); }
    { Case c; c.build(); c.out_stride = 20; expect("output stride below a row", c, STK_INVALID_PARAMS); }
    { Case c; c.out_depth = 32; c.build(); c.out_stride = 7 * 12 + 2; expect("output stride off the element size", c, STK_INVALID_PARAMS); }
    // the limits: the checks read no plane, so a table of one repeated pointer stands for 65536 planes
    { Case c; c.build();
      std::vector<const void*> many(65536, c.data[0]);
      std::vector<void*> outs(65536, c.out[0]);
      c.m.data = many.data(); c.m.n = 65536;
      DemosaicPlan P{}; std::string why;
      CHECK(demosaic_check(&c.m, c.method, c.out_depth, outs.data(), 0, &P, &why) == STK_NOT_IMPLEMENTED && !why.empty(), "65536 planes");
      c.m.n = 65535;
      CHECK(demosaic_check(&c.m, c.method, c.out_depth, outs.data(), 0, &P, &why) == STK_OK, "65535 planes: %s", why.c_str()); }
    CHECK(demosaic_grid_rows(65535 * 16, 0, 1) == 65535 && demosaic_grid_rows(65535 * 16, 2, 1) == 65536, "grid rows at the limit");
    CHECK(demosaic_grid_rows(3, 0, 0) == 1 && demosaic_grid_rows(16, 2, 2) == 2 && demosaic_grid_rows(17, 0, 1) == 2, "grid rows, small");
    CHECK(demosaic_grid_rows(9, 3, 3) == 1 && demosaic_grid_rows(10, 0, 3) == 2 && demosaic_grid_rows(65535 * 8 + 2, 0, 3) == 65536, "grid rows, superpixel");
    { Case c; c.build(); c.m.width = 3; c.m.height = 65535 * 16 + 1; c.m.row_stride_bytes = 0; expect("too many tile rows", c, STK_NOT_IMPLEMENTED); }

    std::string why;
    float plane[1];
    CHECK(cfa_mask_check(4, 4, 0, 0, plane, STK_HOST, &why) == STK_OK && why.empty(), "mask ok");
    CHECK(cfa_mask_check(4, 4, 0, 0, nullptr, STK_HOST, &why) == STK_INVALID_PARAMS && !why.empty(), "mask null plane");
    CHECK(cfa_mask_check(0, 4, 0, 0, plane, STK_HOST, &why) == STK_INVALID_PARAMS, "mask width 0");
    CHECK(cfa_mask_check(4, -1, 0, 0, plane, STK_HOST, &why) == STK_INVALID_PARAMS, "mask height -1");
    CHECK(cfa_mask_check(1 << 16, 1 << 15, 0, 0, plane, STK_HOST, &why) == STK_INVALID_PARAMS, "mask too large");
    CHECK(cfa_mask_check(4, 4, 4, 0, plane, STK_HOST, &why) == STK_INVALID_PARAMS, "mask pattern");
    CHECK(cfa_mask_check(4, 4, 0, 3, plane, STK_HOST, &why) == STK_INVALID_PARAMS, "mask channel 3");
    CHECK(cfa_mask_check(4, 4, 0, -1, plane, STK_HOST, &why) == STK_INVALID_PARAMS, "mask channel -1");
    CHECK(cfa_mask_check(4, 4, 0, 0, plane, 2, &why) == STK_INVALID_PARAMS, "mask location");
}

static void test_overlap() {
    std::vector<char> block(1000);
    char* b = block.data();
    SpanSet s;
    s.add(b + 100, 50);            // [100, 150)
    s.add(b + 400, 10);            // [400, 410)
    s.add(b + 90, 200);            // [90, 290): covers the first
    s.seal();
    const struct { size_t lo, n; bool hit; } q[] = {{0, 90, false}, {0, 91, true}, {289, 1, true}, {290, 110, false}, {290, 111, true},
                                                    {405, 1, true}, {410, 5, false}, {160, 10, true}, {399, 1, false}, {0, 1000, true}};
    for (const auto& e : q) CHECK(s.overlaps(b + e.lo, e.n) == e.hit, "span [%zu, +%zu): want %d", e.lo, e.n, (int)e.hit);
    SpanSet none;
    none.seal();
    CHECK(!none.overlaps(b, 1000), "an empty set overlaps nothing");

    // through the call's check: an output inside a plane's span, in its row padding, right behind its last sample
    Case c; c.n = 2; c.in_stride = 16; c.build();                // 7-byte rows 16 apart: span 4 * 16 + 7 = 71
    std::vector<char> big(71 + 7 * 3 * 5);
    c.data[0] = big.data();
    c.out[1] = big.data() + 71;
    expect("an output right behind a plane", c, STK_OK);
    c.out[1] = big.data() + 70;
    expect("an output on a plane's last sample", c, STK_INVALID_PARAMS);
    c.out[1] = big.data() + 8;
    expect("an output that starts in a plane's row padding", c, STK_INVALID_PARAMS);
    c.out[1] = c.outs[1].data();
    c.out[0] = (void*)c.data[1];
    expect("an output that is another frame's plane", c, STK_INVALID_PARAMS);
}

static void test_layout() {
    static_assert(sizeof(DemFrame) == 16, "record size");
    for (size_t n : {(size_t)1, (size_t)17, (size_t)65535}) for (size_t ob : {(size_t)0, (size_t)1, (size_t)7 * 5 * 3 * 4 * 3}) {
        const DemosaicLayout L = demosaic_layout(n, ob);
        CHECK(L.records == 0 && L.out % 256 == 0 && L.out >= n * sizeof(DemFrame), "layout %zu %zu: records %zu out %zu", n, ob, L.records, L.out);
        CHECK(L.total >= L.out + ob && L.total % 256 == 0, "layout %zu %zu: total %zu", n, ob, L.total);
    }
    const DemosaicLayout M = demosaic_layout(0, 4 * 12);
    CHECK(M.out == 0 && M.total == 256, "mask layout: out %zu total %zu", M.out, M.total);
}

int main() {
    test_accepts_and_sizes();
    test_refusals();
    test_overlap();
    test_layout();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
