// workspace.h — the host back end every combine shares: the carver that lays regions into a grow-only DevBuf, every
// combine's layout built through it, the one reserve-or-fail, the upload of the record table, and the one way to finish a
// combine (CombineOutputs, combine_begin / combine_end). Included from context.h, behind stk_ctx and HIP_TRY. The carver,
// the grids and the layouts are inline and touch no stk_ctx, so a host-only program checks their arithmetic
// (tests/sanitize/workspace_harness.cpp).
#pragma once
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "common.h"
#include "reject.h"

// ---------------------------------------------------------------------------------------------
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Hands out 256-byte-aligned byte offsets in order, from `start` rounded up; total: the end of the last region, rounded.
struct Carver {
    size_t total;
    std::vector<std::pair<size_t, size_t>> spans;       // (offset, bytes asked) of every region handed out
    explicit Carver(size_t start = 0) : total(up256(start)) {}
    size_t take(size_t bytes) {
        const size_t at = total;
        spans.emplace_back(at, bytes);
        total += up256(bytes);
        return at;
    }
};

// the node grid of a step (stk_mesh_grid): nodes gw x gh at multiples of step up to the last pixel; cells cw x ch between them
inline bool grid_step_ok(int step) { return step >= 8 && step <= 256 && (step & (step - 1)) == 0; }
struct NodeGrid { int step, shift, gw, gh, cw, ch; size_t cells() const { return (size_t)cw * ch; } size_t nodes() const { return (size_t)gw * gh; } };
inline NodeGrid node_grid(int w, int h, int step) {
    NodeGrid g{};
    g.step = step;
    while ((1 << g.shift) < step) g.shift++;
    g.gw = (w - 1 + step - 1) / step + 1; g.gh = (h - 1 + step - 1) / step + 1;
    g.cw = (w + step - 1) / step; g.ch = (h + step - 1) / step;
    return g;
}

// ---- the layouts: byte offsets into the buffer named; plane / *plane / pstride / tbytes: bytes of one of several ----------
// ctx->clip: the c, L and U planes of nel floats each, packed (the kernels take three pointers; nothing follows them)
struct ClipLayout { size_t c, L, U, total; };
inline ClipLayout clip_layout(size_t nel) { return ClipLayout{0, nel * sizeof(float), 2 * nel * sizeof(float), 3 * nel * sizeof(float)}; }

// ctx->quantile: a w x h x cn f32 image (the plain call's mean, then a host output's staging copy), the band of band_rows
// rows of n samples (n = 0: none yet), the staging copy of a host caller's counts
struct QuantileLayout { size_t image, band, counts, total; };
inline QuantileLayout quantile_layout(int n, size_t band_rows, int w, int h, int cn, bool counts) {
    Carver c;
    QuantileLayout L{};
    L.image = c.take((size_t)w * h * cn * sizeof(float));
    L.band = c.take(band_rows * n * w * cn * sizeof(float));
    L.counts = c.take(counts ? (size_t)w * h * sizeof(int32_t) : 0);
    L.total = c.total;
    return L;
}

// ctx->weighted; step > 0: with the moments pass's per-wave partials
struct WeightedLayout { size_t image, den, coef, moments, partials, total; };
inline WeightedLayout weighted_layout(int n_entries, int w, int h, int cn, int step) {
    const size_t ne = (size_t)std::max(n_entries, 1);
    Carver c;
    WeightedLayout L{};
    L.image = c.take((size_t)w * h * cn * sizeof(float));
    L.den = c.take((size_t)w * h * sizeof(float));
    L.coef = c.take(ne * sizeof(stk_frame_weight));
    L.moments = c.take(ne * cn * 6 * sizeof(double));
    const bool parts = step > 0 && n_entries > 1;
    L.partials = c.take(parts ? stk::moments_plan(w, h, step).parts() * (size_t)(n_entries - 1) * (1 + 5 * cn) * sizeof(double) : 0);
    L.total = c.total;
    return L;
}

// ctx->local, the local-weighted combine (local.cpp; mesh.cpp's local folds); cn == 0: the map pass alone (no per-entry
// table, image or den plane)
struct LocalLayout { size_t fptrs, mptrs, coef, image, den, planes, plane, total; };
inline LocalLayout local_layout(size_t n_ptrs, int n_entries, int w, int h, int cn, size_t n_planes) {
    Carver c;
    LocalLayout L{};
    L.fptrs = c.take(std::max<size_t>(n_ptrs, 1) * sizeof(void*));
    L.mptrs = c.take(std::max<size_t>(n_ptrs, 1) * sizeof(void*));
    L.coef = c.take(cn ? (size_t)std::max(n_entries, 1) * sizeof(stk_frame_weight) : 0);
    L.image = c.take((size_t)w * h * cn * sizeof(float));
    L.den = c.take(cn ? (size_t)w * h * sizeof(float) : 0);
    L.plane = up256((size_t)w * h * sizeof(float));
    L.planes = c.take(n_planes * L.plane);
    L.total = c.total;
    return L;
}

// ctx->local, local normalisation (local_norm.cpp); cells: the moments pass's records of n_entries - 1 entries; planes:
// one per entry
struct NormLayout { size_t ptrs, coef, image, den, cells, planes, plane, total; };
inline NormLayout norm_layout(int n_entries, int w, int h, int cn, const NodeGrid& g, bool cells, bool planes) {
    const size_t ne = (size_t)std::max(n_entries, 1);
    Carver c;
    NormLayout L{};
    L.ptrs = c.take(ne * sizeof(void*));
    L.coef = c.take(ne * sizeof(stk_frame_weight));
    L.image = c.take((size_t)w * h * cn * sizeof(float));
    L.den = c.take((size_t)w * h * sizeof(float));
    L.cells = c.take(cells ? (ne - 1) * g.cells() * cn * 6 * sizeof(double) : 0);
    L.plane = up256(g.nodes() * 2 * cn * sizeof(float));
    L.planes = c.take(planes ? ne * L.plane : 0);
    L.total = c.total;
    return L;
}

// ctx->local, drizzle (drizzle.cpp); pre: bytes in front (the plain call's mean); the image and den only where they are
// staged for the host; planes: host maps' copies
struct DrizzleLayout { size_t foot, coef, mptrs, image, den, planes, plane, total; };
inline DrizzleLayout drizzle_layout(size_t pre, int n_entries, int sw, int sh, int ow, int oh, int cn, bool host_out, size_t n_planes) {
    const size_t ne = (size_t)std::max(n_entries, 1);
    Carver c(pre);
    DrizzleLayout L{};
    L.foot = c.take(ne * 2 * sizeof(float));
    L.coef = c.take(ne * sizeof(stk_frame_weight));
    L.mptrs = c.take(ne * sizeof(void*));
    L.image = c.take(host_out ? (size_t)ow * oh * cn * sizeof(float) : 0);
    L.den = c.take(host_out ? (size_t)ow * oh * sizeof(float) : 0);
    L.plane = up256((size_t)sw * sh * sizeof(float));
    L.planes = c.take(n_planes * L.plane);
    L.total = c.total;
    return L;
}

// ctx->mesh: three pointer tables indexed like the frame table (the fold's fields, the field pass's fields and status
// planes), the field and status planes, the fill pass's scratch, a w x h x cn f32 image
struct MeshLayout { size_t tptrs, fptrs, sptrs, fields, status, scratch, image, fplane, splane, cplane, total; };
inline MeshLayout mesh_layout(size_t n_ptrs, size_t n_fields, size_t n_status, size_t n_scratch, int gw, int gh, size_t image_floats) {
    const size_t nn = (size_t)gw * gh, pt = std::max<size_t>(n_ptrs, 1) * sizeof(void*);
    Carver c;
    MeshLayout L{};
    L.fplane = up256(nn * 2 * sizeof(float));
    L.splane = up256(nn * sizeof(int32_t));
    L.cplane = stk::mesh_fill_scratch_bytes(gw, gh);
    L.tptrs = c.take(pt);
    L.fptrs = c.take(pt);
    L.sptrs = c.take(pt);
    L.fields = c.take(n_fields * L.fplane);
    L.status = c.take(n_status * L.splane);
    L.scratch = c.take(n_scratch * L.cplane);
    L.image = c.take(image_floats * sizeof(float));
    L.total = c.total;
    return L;
}

// ctx->mesh behind a MeshLayout (base: its total), the coarse-to-fine forms, per table entry (entry 0 = frame 0): the
// validity bytes' pointer table and planes, the pyramid planes (levels 1 .. levels - 1, mesh_pyr_offset) and one frame
// table per level above 0
struct PyrLayout { size_t vptrs, valid, vplane, planes, pstride, tables, tbytes, total; };
inline PyrLayout pyr_layout(size_t base, size_t n_entries, int gw, int gh, int w, int h, int levels) {
    Carver c(base);
    PyrLayout P{};
    P.vplane = up256((size_t)gw * gh);
    P.pstride = up256(stk::mesh_pyr_offset(w, h, levels));
    P.tbytes = up256(n_entries * sizeof(stk::WarpFrame));
    P.vptrs = c.take(n_entries * sizeof(void*));
    P.valid = c.take(n_entries * P.vplane);
    P.planes = c.take(n_entries * P.pstride);
    P.tables = c.take((size_t)(levels - 1) * P.tbytes);
    P.total = c.total;
    return P;
}

// ctx->reject: the entry table, the two counters per entry, then what the caller asks for: the clean image, its counts,
// map planes
struct RejectLayout { size_t entries, tallies, clean, counts, planes, plane, total; };
inline RejectLayout reject_layout(int n_entries, int sw, int sh, int cn, bool clean, bool counts, size_t n_planes) {
    const size_t ne = (size_t)std::max(n_entries, 1);
    Carver c;
    RejectLayout L{};
    L.entries = c.take(ne * sizeof(stk::RejectEntry));
    L.tallies = c.take(ne * 2 * sizeof(unsigned long long));
    L.clean = c.take(clean ? (size_t)sw * sh * cn * sizeof(float) : 0);
    L.counts = c.take(counts ? (size_t)sw * sh * sizeof(int32_t) : 0);
    L.plane = up256((size_t)sw * sh * sizeof(float));
    L.planes = c.take(n_planes * L.plane);
    L.total = c.total;
    return L;
}

// ctx->local, star detection (star.cpp): the frame pointers of the stack, then per (frame, tile) the peak count and the
// STAR_TILE_CAP record slots
struct StarLayout { size_t fptrs, counts, records, total; };
inline StarLayout star_layout(size_t n_frames, size_t tiles) {
    Carver c;
    StarLayout L{};
    L.fptrs = c.take(std::max<size_t>(n_frames, 1) * sizeof(void*));
    L.counts = c.take(n_frames * tiles * sizeof(int32_t));
    L.records = c.take(n_frames * tiles * stk::STAR_TILE_CAP * sizeof(stk::StarRecord));
    L.total = c.total;
    return L;
}

// ctx->local, star measurement (star.cpp): the frame pointers of the stack, then per frame max_stars (px, py) pairs, the number
// of them in use and max_stars record slots
struct StarMeasureLayout { size_t fptrs, stars, counts, records, total; };
inline StarMeasureLayout star_measure_layout(size_t n_frames, size_t max_stars) {
    Carver c;
    StarMeasureLayout L{};
    L.fptrs = c.take(std::max<size_t>(n_frames, 1) * sizeof(void*));
    L.stars = c.take(n_frames * max_stars * 2 * sizeof(int32_t));
    L.counts = c.take(n_frames * sizeof(int32_t));
    L.records = c.take(n_frames * max_stars * sizeof(stk::StarMeasureRecord));
    L.total = c.total;
    return L;
}

// ctx->local, frame calibration (calibrate.cpp): the per-frame records, the copies of host masters (bias, dark, flat; 0
// bytes for a device or absent one) and of a host map, the tightly packed outputs of host frames
struct CalLayout { size_t records, master[3], map, out, total; };
inline CalLayout cal_layout(size_t n_frames, const size_t master_bytes[3], size_t map_bytes, size_t out_bytes) {
    Carver c;
    CalLayout L{};
    L.records = c.take(std::max<size_t>(n_frames, 1) * sizeof(stk::CalFrame));
    for (int k = 0; k < 3; k++) L.master[k] = c.take(master_bytes[k]);
    L.map = c.take(map_bytes);
    L.out = c.take(out_bytes);
    L.total = c.total;
    return L;
}
// ctx->local, stk_defect_map and stk_image_mean: the four counters or sums, the row partials of the sums, the copy of a host
// image, the copy of a host map
struct ImageLayout { size_t counters, partials, image, map, total; };
inline ImageLayout image_layout(size_t partial_rows, size_t image_bytes, size_t map_bytes) {
    Carver c;
    ImageLayout L{};
    L.counters = c.take(4 * sizeof(double));
    L.partials = c.take(partial_rows * 4 * sizeof(double));
    L.image = c.take(image_bytes);
    L.map = c.take(map_bytes);
    L.total = c.total;
    return L;
}

// ctx->local, the background model (background.cpp): the frame pointers of the cells launch, the per-frame records of the
// apply launch, the copy of a host mask, the window records (0 bytes: the apply alone), the level planes (`plane` bytes
// apart, packed: they arrive in one copy; 0 planes: the cells alone), the tightly packed outputs of host frames
struct BgLayout { size_t fptrs, records, mask, cells, planes, plane, out, total; };
inline BgLayout bg_layout(size_t n_frames, size_t mask_bytes, size_t cell_bytes, size_t n_planes, size_t plane_floats, size_t out_bytes) {
    Carver c;
    BgLayout L{};
    L.fptrs = c.take(std::max<size_t>(n_frames, 1) * sizeof(void*));
    L.records = c.take(std::max<size_t>(n_frames, 1) * sizeof(stk::BgFrame));
    L.mask = c.take(mask_bytes);
    L.cells = c.take(cell_bytes);
    L.plane = plane_floats * sizeof(float);
    L.planes = c.take(n_planes * L.plane);
    L.out = c.take(out_bytes);
    L.total = c.total;
    return L;
}

// ctx->local, deconvolution (deconvolve.cpp): the padded tap table, then per colour channel (`channels` = min(cn, 3)) the
// planar work images, `plane` bytes apart inside each: D (which is u_0), the two u planes of the ping-pong and r; the
// copies of a host image and of a host mask (0 bytes for device ones), the staged output of a host image
struct DeconvLayout { size_t taps, D, u[2], r, plane, image, mask, out, total; };
inline DeconvLayout deconv_layout(int radius, int w, int h, int channels, size_t image_bytes, size_t mask_bytes, size_t out_bytes) {
    Carver c;
    DeconvLayout L{};
    L.taps = c.take(stk::dcv_tap_floats(radius) * sizeof(float));
    L.plane = up256((size_t)w * h * sizeof(float));
    L.D = c.take((size_t)channels * L.plane);
    L.u[0] = c.take((size_t)channels * L.plane);
    L.u[1] = c.take((size_t)channels * L.plane);
    L.r = c.take((size_t)channels * L.plane);
    L.image = c.take(image_bytes);
    L.mask = c.take(mask_bytes);
    L.out = c.take(out_bytes);
    L.total = c.total;
    return L;
}

// ctx->local, the wavelet layers (wavelet.cpp): the selection's state and histogram words, then per colour channel
// (`channels` = min(cn, 3)) the planar work images, `plane` bytes apart inside each: the two c planes of the ping-pong
// (c[0] holds c_0) and acc; the copies of a host image and of a host mask (0 bytes for device ones), the staged outputs of
// a host image (the layers form: levels + 1 of them)
struct WaveletLayout { size_t state, c[2], acc, plane, image, mask, out, total; };
inline WaveletLayout wavelet_layout(int w, int h, int channels, size_t image_bytes, size_t mask_bytes, size_t out_bytes) {
    Carver c;
    WaveletLayout L{};
    L.state = c.take(stk::wv_state_words(channels) * sizeof(uint32_t));
    L.plane = up256((size_t)w * h * sizeof(float));
    L.c[0] = c.take((size_t)channels * L.plane);
    L.c[1] = c.take((size_t)channels * L.plane);
    L.acc = c.take((size_t)channels * L.plane);
    L.image = c.take(image_bytes);
    L.mask = c.take(mask_bytes);
    L.out = c.take(out_bytes);
    L.total = c.total;
    return L;
}

// ctx->local, the display stretch (stretch.cpp): the selection's state and histogram words (`channels` = min(cn, 3); 0: none,
// the stretch alone), the copies of a host image and of a host mask (0 bytes for device ones), the table of a table curve
// and the staged output of a host image
struct StretchLayout { size_t state, image, mask, table, out, total; };
inline StretchLayout stretch_layout(int channels, size_t image_bytes, size_t mask_bytes, size_t table_bytes, size_t out_bytes) {
    Carver c;
    StretchLayout L{};
    L.state = c.take(channels ? stk::st_state_words(channels) * sizeof(uint32_t) : 0);
    L.image = c.take(image_bytes);
    L.mask = c.take(mask_bytes);
    L.table = c.take(table_bytes);
    L.out = c.take(out_bytes);
    L.total = c.total;
    return L;
}

// ctx->local, colour-filter mosaics (demosaic.cpp): the per-frame records, then the tightly packed outputs of host mosaics
// (stk_cfa_mask: no records, the plane of a host caller)
struct DemosaicLayout { size_t records, out, total; };
inline DemosaicLayout demosaic_layout(size_t n_frames, size_t out_bytes) {
    Carver c;
    DemosaicLayout L{};
    L.records = c.take(n_frames * sizeof(stk::DemFrame));
    L.out = c.take(out_bytes);
    L.total = c.total;
    return L;
}
// the workgroup rows of a demosaic launch over h mosaic rows: the cell grid starts one row early where red lies on odd rows
// (bit 1 of the pattern); the superpixel kernel (method 3) has DEM_SP_TH output rows per workgroup
inline int demosaic_grid_rows(int h, int pattern, int method) {
    return method == 3 ? (h / 2 + stk::DEM_SP_TH - 1) / stk::DEM_SP_TH : (h + (pattern >> 1) + stk::DEM_TH - 1) / stk::DEM_TH;
}

// ---------------------------------------------------------------------------------------------
// room for `bytes` in a workspace, or STK_HIP_ERROR (the allocator's sticky error is cleared: the context stays usable)
inline stk_status workspace_reserve(stk_ctx* ctx, DevBuf& buf, size_t bytes, const char* what) {
    if (buf.reserve(bytes) == hipSuccess) return STK_OK;
    (void)hipGetLastError();
    return fail(ctx, STK_HIP_ERROR, std::string(what) + ": device allocation of " + std::to_string(bytes) + " bytes failed");
}

// the record table of a fold's entries into device memory (asynchronous: `coef` must outlive the copy)
inline stk_status records_upload(stk_ctx* ctx, void* dst, const std::vector<stk_frame_weight>& coef) {
    HIP_TRY(hipMemcpyAsync(dst, coef.data(), coef.size() * sizeof(stk_frame_weight), hipMemcpyHostToDevice, ctx->stream));
    return STK_OK;
}

// The outputs of a combine: the image and up to two optional side planes (int32 counts, f32 kept / den), each the caller's
// pointer (null: not asked), its staging copy in a workspace and its element count. The kernels write where dst says: the
// caller's memory when the output is device memory, the staging copy when it is the host's; copy_back then issues exactly
// the copies of the planes that are present. The staging copies may be planes the kernel also reads (the clip planes: c
// for the image, L for counts, U for kept), where each thread reads its values before it writes there.
struct OutPlane { void* user; void* stage; size_t elems; size_t elem_bytes = 4; };
struct CombineOutputs {
    bool host;
    OutPlane plane[3];
    CombineOutputs(const stk_image_f32* out, float* stage, size_t elems, OutPlane side0 = {nullptr, nullptr, 0}, OutPlane side1 = {nullptr, nullptr, 0})
        : host(out->location != STK_DEVICE), plane{{out->data, stage, elems}, side0, side1} {}
    // a table the host reads back whatever the frames' location (moments, counters)
    CombineOutputs(void* host_table, void* dev, size_t elems, size_t elem_bytes)
        : host(true), plane{{host_table, dev, elems, elem_bytes}, {nullptr, nullptr, 0}, {nullptr, nullptr, 0}} {}
    void* dst(int k) const { return !plane[k].user ? nullptr : host ? plane[k].stage : plane[k].user; }
    float* image() const { return (float*)dst(0); }
    template <typename T> T* side(int k) const { return (T*)dst(1 + k); }
    stk_status copy_back(stk_ctx* ctx) const {
        for (const OutPlane& p : plane)
            if (host && p.user) HIP_TRY(hipMemcpyAsync(p.user, p.stage, p.elems * p.elem_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return STK_OK;
    }
};

// The bracket of a combine's launches: begin records ev[4]; end records ev[5], copies the host outputs back, synchronises
// and adds the device time between the two to *ms (null: not asked).
inline stk_status combine_begin(stk_ctx* ctx) {
    HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    return STK_OK;
}
inline stk_status combine_end(stk_ctx* ctx, double* ms, const CombineOutputs* o = nullptr) {
    HIP_TRY(hipEventRecord(ctx->ev[5], ctx->stream));
    if (o) if (stk_status st = o->copy_back(ctx)) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ms) *ms += ev_ms(ctx->ev[4], ctx->ev[5]);
    return STK_OK;
}
