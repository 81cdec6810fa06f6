/*
 * stacker.h — C ABI of the MI355X-native align-and-stack engine.
 *
 * This is the drop-in boundary for the hot path of eadf/libstacker.rs:
 * everything a Rust `libstacker`-compatible shim needs to bind (see
 * INTEGRATION.md for the `extern "C"` block a maintainer would add).
 * Plain pointers and sizes only; no C++ / torch types cross this line.
 *
 * Conventions
 *  - Images are interleaved, row-major, BGR channel order (OpenCV `Mat`
 *    layout, which is what the reference hands around: utils.rs:128-144).
 *  - `location` says whether a pointer is host (0) or device/HBM (1) memory.
 *  - Every entry point returns an `stk_status`; the message of the last
 *    failure is available from stk_last_error(). Nothing throws or aborts.
 *  - A `stk_ctx` owns one GPU, one HIP stream and the HBM workspace — or, made
 *    with stk_create_multi, several GPUs of the node (one host thread, stream
 *    and workspace per GPU, RCCL communicators for the accumulator reduce);
 *    one call at a time per context, any number of contexts per process.
 *
 * Reference citations are `file:line` under the reference checkout
 * (`src/lib.rs`, `src/utils.rs`).
 */
#ifndef STACKER_H
#define STACKER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: mirror StackerError (lib.rs:27-45) ------------------ */
typedef enum {
    STK_OK = 0,
    STK_NOT_ENOUGH_FILES = 1, /* StackerError::NotEnoughFiles  lib.rs:31,155,725 */
    STK_INVALID_PARAMS = 2,   /* StackerError::InvalidParams   lib.rs:41,324,377,876,883 */
    STK_PROCESSING_ERROR = 3, /* StackerError::ProcessingError lib.rs:43,347,841 */
    STK_BACKEND_ERROR = 4,    /* StackerError::OpenCvError     lib.rs:30 (ECC no-conv/NaN, bad types) */
    STK_IO_ERROR = 5,         /* StackerError::IoError         lib.rs:36 */
    STK_HIP_ERROR = 6,        /* no reference analogue: HIP runtime failure */
    STK_NOT_IMPLEMENTED = 7   /* StackerError::NotImplemented  lib.rs:33 */
} stk_status;

/* ---- constants the reference passes through from OpenCV ---------------- */
enum { STK_MOTION_TRANSLATION = 0, STK_MOTION_EUCLIDEAN = 1, /* MotionType lib.rs:603-609 */
       STK_MOTION_AFFINE = 2, STK_MOTION_HOMOGRAPHY = 3 };
enum { STK_METHOD_LEAST_SQUARES = 0, STK_METHOD_LMEDS = 4, /* KeyPointMatchParameters::method lib.rs:51 */
       STK_METHOD_RANSAC = 8, STK_METHOD_RHO = 16 };
/* (RHO and OpenCV's USAC numbers 32 .. 38: STK_NOT_IMPLEMENTED. Any other value: findHomography throws, stk_find_homography
 * reports STK_BACKEND_ERROR, and the whole-stack calls skip every moving frame as lib.rs:275 does.) */
enum { STK_BORDER_CONSTANT = 0, STK_BORDER_REPLICATE = 1, STK_BORDER_REFLECT = 2,
       STK_BORDER_WRAP = 3, STK_BORDER_REFLECT_101 = 4, STK_BORDER_TRANSPARENT = 5 };
enum { STK_HOST = 0, STK_DEVICE = 1 };
enum { STK_INTER_LINEAR = 1, STK_INTER_CUBIC = 2 };   /* option "warp_interpolation"; OpenCV's INTER_LINEAR / INTER_CUBIC numbers */
enum { STK_DEPTH_U8 = 8, STK_DEPTH_U16 = 16, STK_DEPTH_F32 = 32 };

/* ---- parameter mirrors -------------------------------------------------- */
/* KeyPointMatchParameters, lib.rs:48-73; defaults utils.rs:250-261. */
typedef struct {
    int32_t method;                 /* STK_METHOD_* */
    double  ransac_reproj_threshold;
    float   match_keep_ratio;
    float   match_ratio;
    int32_t border_mode;            /* STK_BORDER_* */
    double  border_value[4];        /* core::Scalar */
} stk_keypoint_params;

/* EccMatchParameters, lib.rs:611-623; Option<T> -> has_* flag + value
 * (TermCriteria mapping utils.rs:159-170). */
typedef struct {
    int32_t motion_type;            /* STK_MOTION_* */
    int32_t has_max_count;
    int32_t max_count;
    int32_t has_epsilon;
    double  epsilon;
    int32_t gauss_filt_size;        /* odd, 1 .. 63 (larger: STK_NOT_IMPLEMENTED) */
} stk_ecc_params;

/* A stack of decoded frames (what read_grey_and_f32's imread produced,
 * utils.rs:132): data[0] is the reference frame. All frames of a stk_frames share this one geometry; a stack whose
 * frames differ in size goes through stk_keypoint_match_mixed with one stk_frame_geometry per frame. */
typedef struct {
    const void* const* data;        /* n pointers */
    int32_t n;
    int32_t width, height;
    int32_t channels;               /* 3 (BGR) or 4 (BGRA, what imread(IMREAD_UNCHANGED) makes of a PNG with alpha: grey comes
                                       from B, G, R — cvtColor ignores the fourth channel, utils.rs:136-142 — and the stacked image
                                       has four channels too, the fourth being the aligned, averaged alpha / 255, exactly what the
                                       reference's convertTo / warp / add do to it); 1 is accepted by stage-level calls only */
    int32_t depth;                  /* STK_DEPTH_* */
    int32_t location;               /* STK_HOST | STK_DEVICE */
    size_t  row_stride_bytes;       /* 0 = tightly packed; else the bytes from one row to the next: at least width * channels *
                                       (depth / 8) and a multiple of depth / 8, anything else is STK_INVALID_PARAMS. This is how a
                                       Mat with padded rows, or a ROI of a larger image, is handed over; the frames need not be
                                       evenly spaced in memory, and neither data[i] nor the stride need any alignment. The results
                                       do not depend on the layout: a padded stack gives the bits of its tightly packed copy.
                                       What the engine reads of frame i, with span = row_stride_bytes * (height - 1) + width *
                                       channels * (depth / 8), the bytes from its first to its last pixel:
                                       - STK_HOST: bytes [data[i], data[i] + span) and nothing else: the padding behind the last
                                         pixel of the last row is not read (a ROI may end on the last byte of its parent buffer);
                                       - STK_DEVICE: bytes [data[i], data[i] + span) too, but ANY of them, the padding between two
                                         rows included (it must be readable memory; its values never reach a result): the warp
                                         kernels' dword-aligned windows reach up to 6 bytes past the last pixel of any row but the
                                         last (warp_accumulate_u8c3_kernel, warp_body.h: 12 bytes from (offset & ~3)
                                         for the 6 bytes of a pixel pair that starts at most at 3 * (width - 2); 4 bytes in
                                         warp_accumulate_u16c3_kernel, kernels_warp.hip; their unaligned forms 2 and 0 bytes), which
                                         for a tight frame is the next row. No kernel reads before the first pixel — a window's
                                         aligned start never precedes its row, whose offset is a multiple of 4 whenever windows
                                         are used — or behind the last one: windows are used on rows 0 .. height - 2 only (the
                                         interior test keeps a row to spare), and the 8-byte load of the last row's last pixel
                                         pair backs off by 2 bytes (warp_body.h, the rim path).
                                         Under "warp_interpolation" = STK_INTER_CUBIC the generic cubic kernel (warp_accumulate_cubic_kernel,
                                         warp_cubic_body.h) reads pixels only, element by element: the 4 x 4 taps of a footprint that lies
                                         wholly inside the frame, and the generic linear kernel's clamped taps elsewhere. The u8 BGR fast kernel
                                         (warp_accumulate_cubic_u8c3_kernel) reads a footprint row's twelve bytes as one 16-byte window from
                                         (offset & ~3) when bases and strides are dword-aligned: up to 4 bytes past the last pixel of a row, on
                                         rows 0 .. height - 2 only (its vote keeps a row to spare below the footprint), never before the row's
                                         first pixel; everywhere else it reads exactly the twelve bytes, or the linear sample's clamped taps.
                                         Nothing before the first or behind the last pixel of the span.
                                         The preparation kernels (kernels_prep.hip, kernels_quality.hip) read pixels only, and
                                         so does the calibration kernel (calibrate_kernel, kernels_calibrate.hip): element by
                                         element, a pixel's own channels and, for a defective pixel, those of its in-frame
                                         neighbours at +-defect_step. */
} stk_frames;

/* Geometry of ONE frame of a stack whose frames differ in size (stk_keypoint_match_mixed). */
typedef struct {
    int32_t width, height;
    size_t  row_stride_bytes;       /* 0 = tightly packed; else as stk_frames.row_stride_bytes (same rules, same reads) */
} stk_frame_geometry;

/* Caller-allocated f32 image (the returned CV_32FC3 Mat, lib.rs:98,656; CV_32FC4 — channels = 4 — for BGRA stacks). */
typedef struct {
    float*  data;
    int32_t width, height, channels;
    int32_t location;               /* STK_HOST | STK_DEVICE */
    size_t  row_stride_bytes;       /* 0 = tightly packed */
} stk_image_f32;

/* Optional per-frame report (additive; the reference discards these). */
typedef struct {
    int32_t status;                 /* 0 used, 1 dropped (keypoint path), 2 error */
    int32_t iterations;             /* ECC iterations executed */
    double  rho;                    /* final ECC correlation coefficient */
    int32_t n_keypoints;
    int32_t n_matches;              /* after ratio test + truncation */
    int32_t n_inliers;
    int32_t reserved;
    double  warp[9];                /* row-major 3x3 (2x3 padded with 0 0 1) */
} stk_frame_stats;

/* Device-side timing of the last whole-stack call, in milliseconds (HIP
 * events on the context's stream) plus launch counts, for roofline reports. */
typedef struct {
    double prep_ms;        /* grey + blur + gradients (ECC) or ORB (keypoint) */
    double align_ms;       /* ECC iterations or match+RANSAC */
    double warp_ms;        /* warp + accumulate */
    double finalize_ms;
    int64_t ecc_iter_launches;      /* launches of the fused ECC iteration kernel */
    int64_t ecc_slot_iterations;    /* sum over launches of active slots (frame-iterations) */
    int64_t warp_launches;
    int64_t warp_frames;
    /* option "profile" = 2 brackets every ECC iteration launch with its own HIP event pair: */
    double  ecc_iter_ms;            /* sum of those launch durations */
    int64_t ecc_iter_timed;         /* number of launches measured */
    /* host-fed stacks (frames->location == STK_HOST): the copy stream's wall time from the first copy's start to the
     * last copy's end, and the bytes moved; 0 for device-resident stacks */
    double  h2d_ms;
    int64_t h2d_bytes;
    /* keypoint path: time and launches of the dominant ORB kernel (FAST-9/16 + NMS, all pyramid levels), pixels scanned */
    double  fast_ms;
    int64_t fast_launches;
    int64_t fast_pixels;
    /* ECC iteration pass: column strips that started on the per-wave LDS ring, failed its run-time bounds check and were
     * redone by the gather loop (same bits). 0 on every BASELINE stack; non-zero only costs time. */
    int64_t ecc_ring_fallbacks;
} stk_timing;

typedef struct stk_ctx stk_ctx;

/* ---- context ------------------------------------------------------------ */
stk_status  stk_create(int32_t device_id, stk_ctx** out);
/* One context over n_devices GPUs of this node: what a single-process caller (the Rust drop-in) uses to stack on all of
 * them. stk_keypoint_match / stk_ecc_match / stk_hybrid_match (and the *_files forms) then cut the moving frames 1..n-1
 * into contiguous ranges, one per device (stk_shard_moving_frames; replaces the Rayon fold, lib.rs:188-320, 746-818),
 * run one host thread per device, sum the f32 accumulators and the {added, dropped} counters on device_ids[0] with
 * RCCL ncclReduce over xGMI (replaces try_reduce, lib.rs:321-335, 819-833) and scale there (lib.rs:339-345, 836-839).
 * Frames may be host memory or device memory on any of the devices (frames on another device are copied over once).
 * Per-frame results are bit-identical to the single-device run (a frame's summation partition depends on the frame size
 * only); the image differs by the order of the f32 adds only. n_devices == 1 returns a plain context. Stage-level and
 * *_shard entry points on such a context run on device_ids[0]. RCCL (librccl.so.1) is loaded at this call. */
stk_status  stk_create_multi(int32_t n_devices, const int32_t* device_ids, stk_ctx** out);
/* The cut itself: rank `rank` of `world_size` aligns frames [first, first + count) of an n_frames stack (frame 0 is the
 * reference and belongs to nobody's range; rank 0 folds it in). Sizes differ by at most one, earlier ranks are larger. */
stk_status  stk_shard_moving_frames(int32_t n_frames, int32_t world_size, int32_t rank, int32_t* first, int32_t* count);
/* Loads RCCL, sum-reduces `count` floats over the context's devices (a 1-rank communicator on a plain context) and
 * verifies the result on the root: the part of the multi-device path that a one-GPU machine can still execute. */
stk_status  stk_rccl_selftest(stk_ctx* ctx, int64_t count);
void        stk_destroy(stk_ctx* ctx);
const char* stk_last_error(const stk_ctx* ctx);    /* valid until the next call on ctx */
/* Run on a caller-owned hipStream_t (e.g. torch's current stream); NULL
 * restores the context's own stream. */
stk_status  stk_set_stream(stk_ctx* ctx, void* hip_stream);
stk_status  stk_get_timing(const stk_ctx* ctx, stk_timing* out);
/* Device-side event counters of the last whole-stack call, by name (stk_timing keeps its layout). Unknown name:
 * STK_INVALID_PARAMS.
 *   "ecc_first_iter_slots"  ECC iteration pass, homography: slot-iterations that took the first-iteration route (option
 *                           "ecc_first_iter"): one per frame that starts at the identity; 0 with the option off, for the
 *                           other motion types, under "ecc_variant" 0 and for f32 images.
 *   "robust_select_us"      median / MAD clip (stk_robust_clip_stack and the *_robust_clipped calls): device time of the
 *                           last such call's selection launches in microseconds, part of its stk_timing.finalize_ms.
 *   "prep_stream_frames"    test hook: ECC templates of the last call that the streaming grey + blur kernel wrote (one launch
 *                           per run of frames, option "prep_stream"); the others took the per-frame kernels.
 *   "workspaces_empty"      test hook: how many of the grow-only device workspaces of this context, of its hidden keypoint
 *                           lane contexts and of its multi-device state have never been reserved (capacity 0).
 *   "debug_poison_bytes"    test hook: the bytes the last "debug_poison" (stk_set_option) filled; 0 before the first. */
stk_status  stk_get_counter(const stk_ctx* ctx, const char* name, int64_t* out);
/* Pinned (page-locked) host memory for frames: stacks handed over in such buffers cross PCIe by DMA at link rate and
 * overlap with the alignment of the frames that have already arrived (a decoder — the Rust shim's imread — writes into
 * them directly). Pageable frames work too (the HIP runtime locks large sources on the fly: 25 MB frames measured the same
 * 55 GB/s; small or fragmented buffers go through its staging path). */
stk_status  stk_host_alloc(size_t bytes, void** out);
void        stk_host_free(void* p);
/* Tuning knobs. None changes a frame's warp or the stacked image except where noted:
 *   "ecc_slots"          frames iterated concurrently by one ECC launch (0 = auto: the whole stack in one round up to 128 frames,
 *                        beyond that at least three equal rounds of at most 96; rounds of at most 64 for frames up to 1080p;
 *                        1..256); changes no result
 *   "ecc_blocks"         workgroups per ECC launch, all frames in flight together (0 = auto: per frame (column strips x rows) /
 *                        (4 x 112), at most 288 — a function of the frame size only: 288 at 4K, 72 at 1080p); a non-zero
 *                        value changes the f32 summation partition, i.e. results at round-off level (within the stated
 *                        ECC tolerance)
 *   "ecc_variant"        ECC pixel-pass kernel: 3 production (default), 0 the direct cross-check version
 *   "ecc_ring"           homography pass: 1 (default) frame-0 rows go through a per-wave LDS ring where a strip allows it,
 *                        0 every tap is gathered from global memory; the results are bit-identical
 *   "ecc_first_iter"     homography pass: 1 (default) the first iteration of a frame that starts at the identity reads frame 0 at
 *                        its own pixels and takes the sums that do not depend on the frame from one evaluation per call
 *                        (stk_get_counter "ecc_first_iter_slots"); 0 every iteration takes the general route; the results are bit-identical
 *   "ecc_ring_lookahead" debug: frame-0 rows the ring keeps ahead of the row being fetched (5; 1..4 make its run-time check
 *                        fire, the strips then fall back to the gather loop: stk_timing.ecc_ring_fallbacks); same bits
 *   "ecc_groups"         0 (default): by frame size; 2: the slots form two groups with their own (iterate, solve) launch sequences on
 *                        two streams, one group's solve and launch boundaries running under the other's iteration pass (pays for
 *                        device-resident stacks of frames up to 1080p with >= 32 slots); 1: one sequence. Per-frame results do not depend on it
 *   "ecc_chunk"          (iterate, solve) pairs enqueued between two polls of the completion counter (0 = default: 2 for frames larger
 *                        than 1080p, 4 otherwise)
 *   "kp_lanes"           3 (default; 1..8): device-resident keypoint stacks of >= 16 frames are cut into this many runs of frames (at
 *                        least 8 each) that go through the pipeline side by side, the later ones on hidden helper contexts of
 *                        the same device, so that one run's kernels fill the other runs' host steps; the fold follows run by
 *                        run in stack order. 1: one pipeline. Per-frame results and the stacked image do not depend on it
 *   "orb_resize_tables"  1 (default): ORB's pyramid steps read their bilinear coefficient tables from memory (computed once per
 *                        geometry); 0: every tile computes its own. Same bits either way
 *   "kp_tail_priority"   1 (default): on device-resident stacks that run in several lanes, a lane's descriptor / 2-NN / homography launches
 *                        go to a highest-priority stream (they queue behind the other lanes' large launches otherwise); 0: one stream
 *   "orb_device_cull"    1 (default): ORB's Harris cull (retainBest) and ordering run on the device; 0: on the host pool. Same keypoints
 *   "orb_fast_all"       1 (default): ORB's FAST, non-maximum suppression and short lists run for all pyramid levels in four launches
 *                        where the pyramid allows it (below 2^32 bytes per frame); 0: level by level, the route of larger
 *                        pyramids. Same keypoints either way
 *   "orb_patch_blur"     1 (default): ORB's 7x7 blur is computed by the descriptor kernel, for the 45 x 40 window around each kept
 *                        keypoint only; 0: every pyramid level is blurred whole first. Same bits either way
 *   "kp_workers"         host threads for the per-frame host steps of the keypoint path (Harris cull, RANSAC)
 *   "warp_subpixel_bits" 0 = exact f32 coordinates (OpenCV >= 4.11 kernels); 5 = classic 1/32-px quantised table
 *                        (changes results: it selects the other OpenCV behaviour)
 *   "warp_interpolation" 1 = STK_INTER_LINEAR (default): bilinear samples, the reference's INTER_LINEAR; 2 = STK_INTER_CUBIC: the
 *                        bicubic fold defined below ("Bicubic fold"), for every call that folds: stk_warp_accumulate, the
 *                        whole-stack, shard, mixed-size, files, hybrid and ranked calls, and the clip, quantile, weighted,
 *                        moments and normalised-rejection combines (changes results: an extension beyond the reference, which
 *                        knows bilinear samples only). Any other value: STK_INVALID_PARAMS. Cubic is defined on exact
 *                        coordinates only: with "warp_subpixel_bits" = 5 every call that folds returns STK_INVALID_PARAMS (the
 *                        pair is checked at the call, so the two options may be set in either order). In the local-weighted
 *                        fold the sample is cubic and the weight omega stays bilinear. Alignment (ECC,
 *                        ORB, homography) does not depend on it: warps, iteration counts and `dropped` are the same
 *   "profile"            0 off, 1 per-stage events (stk_get_timing), 2 + event pairs around ECC launches
 *   "profile_stride"     with profile = 2: bracket every n-th ECC launch only
 *   "prep_stream"        1 (default): ECC templates of a run of frames by the streaming grey + blur kernel, one launch per
 *                        run; 0: the LDS-tiled kernel, frame by frame. Same bits either way
 *   "prep_overlap"       1 (default): on a device-resident stack of more than 2 x "ecc_slots" frames the ECC templates are
 *                        prepared on a second stream while the first frames already iterate; 0: all templates first.
 *                        Same bits either way (stk_timing.prep_ms then covers the reference frame only)
 *   "upload_batch"       host-fed stacks: frames per host -> HBM batch (default 8); a batch is the unit the ECC queue
 *                        and the batched ORB wait for
 *   "quantile_band_rows" quantile combines: rows per band of samples. 0 (default): as many as fit a 4 GiB sample buffer;
 *                        n > 0: at most n. Same bits either way
 *   "calibrate_chunk"    stk_calibrate: frames a workgroup runs through with its tile of the masters in registers. 0
 *                        (default): 16; 1 .. 4096 as given (1: the masters are read once per frame, for measuring what
 *                        holding them buys). Same bits either way
 *   "debug_poison"       debug, acts at once and is not remembered: value b, 0 .. 255 (anything else: STK_INVALID_PARAMS,
 *                        nothing touched). Every stream of the context is drained; every grow-only device workspace (over
 *                        its whole capacity) and every page-locked host block the context owns is filled with the byte b;
 *                        the streams are drained again; the same happens to every hidden keypoint lane context, to every
 *                        member of a multi-device context and to its accumulators. What the context remembers about the
 *                        CONTENT of a workspace (the ECC reference planes' zero border, the ORB resize tables) is forgotten;
 *                        memory of the caller's is never written. The contract it tests: the outputs and per-frame
 *                        statistics of a call are a function of the call's arguments and the context's options only, never
 *                        of what the context did before. Changes no result (stk_get_counter "debug_poison_bytes") */
stk_status  stk_set_option(stk_ctx* ctx, const char* name, int64_t value);
const char* stk_version(void);

/* ---- whole-stack entry points: replace lib.rs:129-144 and lib.rs:702-717 -- */
/* keypoint_match(files, params, scale_down_width) -> (dropped, Mat).
 * scale_down_width <= 0 means None. */
stk_status stk_keypoint_match(stk_ctx* ctx, const stk_frames* frames,
                              const stk_keypoint_params* params, float scale_down_width,
                              stk_image_f32* out, int32_t* dropped,
                              stk_frame_stats* stats_or_null);
/* keypoint_match on frames of DIFFERING size, as the reference handles them: every frame is read on its own, ORB runs at
 * the frame's own size, and warp_perspective's dsize is the FIRST frame's (lib.rs:166, 200-204, 290-299) — `out` has
 * geometry[0]'s size. geometry: n entries (frames->width / height / row_stride_bytes are ignored), or NULL = the stack of
 * one geometry `frames` describes; a stack whose entries are all equal takes the batched pipeline of stk_keypoint_match,
 * any other goes frame by frame through the same stages (same per-frame results). 8-bit BGR(A) frames. scale_down_width > 0 is
 * keypoint_match_scale_down (lib.rs:355-601) on such a stack: validated against the FIRST frame's width, every grey shrunk
 * (or enlarged) by scale_image to ITS OWN smaller dimension = scale_down_width, the homography rescaled by that frame's own ratios.
 * (ecc_match has no such form: on frames of differing size the reference fails in cv::add, lib.rs:809 —
 * stk_ecc_match_files reports that as STK_BACKEND_ERROR.) */
stk_status stk_keypoint_match_mixed(stk_ctx* ctx, const stk_frames* frames, const stk_frame_geometry* geometry,
                                    const stk_keypoint_params* params, float scale_down_width, stk_image_f32* out,
                                    int32_t* dropped, stk_frame_stats* stats_or_null);
/* ecc_match(files, params, scale_down_width) -> Mat. */
stk_status stk_ecc_match(stk_ctx* ctx, const stk_frames* frames,
                         const stk_ecc_params* params, float scale_down_width,
                         stk_image_f32* out, stk_frame_stats* stats_or_null);

/* ---- shard-level entry points (one process per GPU; frames[0] is always the
 * reference frame, the remaining entries are this rank's slice of 1..N-1).
 * They produce the UN-normalised f32 sum (the Rayon fold accumulator,
 * lib.rs:306-316 / 807-814) in `sum` (device memory) and the number of frames
 * added; the caller reduces sums/counts across ranks (RCCL) and then calls
 * stk_finalize_mean once on the root. add_reference != 0 adds frame 0 itself
 * (lib.rs:194-196, 752-754) — exactly one rank does that.
 * On any status other than STK_OK the contents of `sum` are UNDEFINED (the fold is enqueued on the device behind the
 * alignment and may already have overwritten it when a frame's failure reaches the host; the reference's `?` yields no
 * image at all): do not reduce or reuse it. */
stk_status stk_ecc_match_shard(stk_ctx* ctx, const stk_frames* frames,
                               const stk_ecc_params* params, float scale_down_width,
                               int32_t add_reference, stk_image_f32* sum,
                               int32_t* n_added, stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_shard(stk_ctx* ctx, const stk_frames* frames,
                                    const stk_keypoint_params* params, float scale_down_width,
                                    int32_t add_reference, stk_image_f32* sum,
                                    int32_t* n_added, int32_t* n_dropped,
                                    stk_frame_stats* stats_or_null);
/* img / (n as f64)  ==  img * (float)(1.0/n)  (lib.rs:339-345, 836-839). In place if out==sum. */
stk_status stk_finalize_mean(stk_ctx* ctx, const stk_image_f32* sum, int64_t n_frames,
                             stk_image_f32* out);

/* ---- Bicubic fold: an EXTENSION beyond the reference ------------------------------------------------
 * The reference samples bilinearly (INTER_LINEAR, lib.rs:296, 541, 787, 799, 969, 980), and so does every fold here by
 * default. Option "warp_interpolation" = STK_INTER_CUBIC replaces the sample — and nothing else — in every call that folds
 * and every combine built on the fold. For destination pixel (x, y), table entry i and channel c:
 *   - (X, Y), `finite`, ix = floor X, iy = floor Y, tx = X - ix and ty = Y - iy are exactly what the linear fold computes
 *     under warp_subpixel_bits = 0: the same fma chains, the same division, the same finite test.
 *   - Footprint test: finite && ix >= 1 && ix + 2 <= sw - 1 && iy >= 1 && iy + 2 <= sh - 1 (sw x sh: the source frame).
 *   - Where the test fails the sample is the linear fold's sample, bit for bit, border mode and border value included.
 *     That covers frames narrower or lower than 4 pixels and the one-pixel ring around every warped frame's image: the
 *     resampler drops to the lower order at the edge, it does not invent taps.
 *   - kappa (the coverage weight of the weighted and normalised-rejection combines) is the linear fold's everywhere. It
 *     is exactly 1.0f wherever the test holds, so participation, `coverage`, the overlap moments and every rim rule keep
 *     their meaning unchanged.
 *   - Where the test holds, with A = -0.75f (OpenCV's INTER_CUBIC kernel in factored form); all values f32, each
 *     operation rounded on its own except where an fma is written. For t in {tx, ty}:
 *         u = 1 - t;  tt = t * t;  uu = u * u
 *         w0 = (A * t) * uu
 *         w1 = fma(fma(1.25f, t, -2.25f), tt, 1.0f)
 *         w2 = fma(fma(1.25f, u, -2.25f), uu, 1.0f)
 *         w3 = (A * u) * tt
 *         p[r][k] = (float)src[iy - 1 + r][ix - 1 + k][c] * alpha          r, k = 0 .. 3
 *         h_r = fma(wx3, p[r][3], fma(wx2, p[r][2], fma(wx1, p[r][1], wx0 * p[r][0])))
 *         s   = fma(wy3, h_3,     fma(wy2, h_2,     fma(wy1, h_1,     wy0 * h_0)))
 * Consequences:
 *   - t = 0 gives the weights (-0, 1, 0, -0): an integer translation of finite data returns the linear fold's bits.
 *   - t = 0.5 gives exactly (-3, 19, 19, -3) / 32.
 *   - The weights have negative lobes (sum |w| <= 1.375 per axis): a sample may leave the range of its taps, and the
 *     stacked image is not clamped.
 *   - It is NOT bit-matched to OpenCV's INTER_CUBIC warp, which quantises coordinates to 1/32 px; nothing here pins that.
 * Cubic is defined on exact coordinates only: with warp_subpixel_bits = 5 every call that folds is STK_INVALID_PARAMS. */

/* ---- sigma-clipped stacking: an EXTENSION beyond the reference ---------------------------------------
 * Kappa-sigma rejection over the same samples the mean adds: per pixel and channel the samples s_i are the warped,
 * converted frames in fold order (frame 0 through the identity, then the kept frames in ascending index) with the fold's
 * own warp, border and alpha. Everything is f32, each operation rounded on its own (`/` and sqrt correctly rounded):
 *   start:  c = the plain mean ((sum of s_i in order) * (float)(1.0 / N)), L = -inf, U = +inf
 *   passes t = 1 .. iterations + 1, each over the samples in order:
 *           k = 0, a = 0, b = 0;  for each s: d = s - c; if (L <= s && s <= U) { k += 1; a = a + d; b = b + d*d; }
 *           last pass: out = k > 0 ? c + a / (float)k : c; counts = k
 *           otherwise, if k >= 3: ma = a / k; m = c + ma; v = b / k - ma*ma; sigma = sqrt(max(v, 0));
 *                                 L = max(L, m - kappa_low sigma); U = min(U, m + kappa_high sigma); c = m
 *                     (k < 3: c, L and U stay)
 * `counts` (optional) receives k of the last pass: width * height * channels int32 in the location of `out`. `out` must
 * be tightly packed. stk_timing.finalize_ms of these calls is the device time of the clip passes (warp_ms etc. are the
 * plain call's). A multi-device context runs them on its first device (like the mixed-size route): the plain mean they
 * start from is then the single-device one. */
typedef struct {
    float   kappa_low, kappa_high;  /* rejection below c - kappa_low sigma / above c + kappa_high sigma: > 0, finite */
    int32_t iterations;             /* clipping passes T before the final pass, 1 .. 16 */
    int32_t reserved;               /* 0 */
} stk_clip_params;

/* ecc_match with the clipped combine: stats, warps, iterations and errors are those of stk_ecc_match on the same input
 * (every frame is a sample: the reference aborts the stack on any ECC failure). */
stk_status stk_ecc_match_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                 const stk_clip_params* clip, stk_image_f32* out, int32_t* counts_or_null,
                                 stk_frame_stats* stats_or_null);
/* keypoint_match with the clipped combine: stats and `dropped` as stk_keypoint_match; the samples are frame 0 and the
 * frames with status 0, folded with the params' border mode and value. */
stk_status stk_keypoint_match_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                      float scale_down_width, const stk_clip_params* clip, stk_image_f32* out, int32_t* dropped,
                                      int32_t* counts_or_null, stk_frame_stats* stats_or_null);
/* The combine alone, for a caller holding its own warps (e.g. the stats of stk_hybrid_match): M is n x 9 doubles, the
 * forward matrices exactly as stk_warp_accumulate takes them, frame 0's entry included; include_or_null: n flags (non-zero
 * = a sample) or NULL = every frame. border_mode as stk_warp_accumulate (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101). */
stk_status stk_clip_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                          int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                          const stk_clip_params* clip, stk_image_f32* out, int32_t* counts_or_null);

/* ---- median and quantile stacking: an EXTENSION beyond the reference ---------------------------------
 * An order statistic over the same samples the mean adds: per pixel and channel the samples s_1 .. s_N are the warped,
 * converted frames in fold order (frame 0 through the identity, then the kept frames in ascending index; in
 * stk_quantile_stack the included frames in index order under the caller's matrices) with the fold's own warp, border
 * mode and value, alpha and warp_subpixel_bits. Border-constant samples at frame edges count, as in the mean: N is the
 * same for every pixel. With s_(k) the k-th smallest sample (k from 0), in f32, each operation rounded on its own:
 *   vi = (float)(N - 1) * quantile;  j = floor(vi);  g = vi - j;
 *   lo = s_(j);  hi = s_(min(j + 1, N - 1));  d = hi - lo;
 *   out = g == 0 ? lo : (g >= 0.5 ? hi - d * (1 - g) : lo + d * g)
 * Apart from the g == 0 rule this is numpy.quantile(samples, quantile, axis=0) with method 'linear', bit for bit (an f32
 * stack, a Python-float quantile). The rule is deliberate: numpy gives NaN where lo is finite and hi is +-inf, i.e. at the
 * very pixels (one inf hot pixel) that a median is meant to clean up. Any NaN sample makes the output there NaN. -0 and +0
 * are equal: either sign may come back. The median is quantile = 0.5; at even N it can differ from numpy.median by 1 ulp
 * (numpy.median takes (lo + hi) / 2). N is at most 4096 (STK_NOT_IMPLEMENTED beyond).
 * `out` must be tightly packed. stk_timing.finalize_ms of these calls is the combine's device time (warp_ms etc. are the
 * plain call's). The samples go through a device buffer band by band (rows [y0, y0 + R) of all N frames at a time; option
 * "quantile_band_rows"). A multi-device context runs these calls on its first device. */
typedef struct {
    float   quantile;               /* 0 <= quantile <= 1: 0 = min, 0.5 = median, 1 = max */
    int32_t reserved;               /* 0 */
} stk_quantile_params;

/* ecc_match with the quantile combine: stats, warps, iterations and errors are those of stk_ecc_match on the same input. */
stk_status stk_ecc_match_quantile(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                  const stk_quantile_params* quantile, stk_image_f32* out, stk_frame_stats* stats_or_null);
/* keypoint_match with the quantile combine: stats and `dropped` as stk_keypoint_match; the samples are frame 0 and the
 * frames with status 0, folded with the params' border mode and value. */
stk_status stk_keypoint_match_quantile(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                       float scale_down_width, const stk_quantile_params* quantile, stk_image_f32* out,
                                       int32_t* dropped, stk_frame_stats* stats_or_null);
/* The combine alone over caller-held warps, with the arguments of stk_clip_stack. */
stk_status stk_quantile_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                              int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                              const stk_quantile_params* quantile, stk_image_f32* out);

/* ---- weighted, coverage-aware stacking with per-frame normalisation: an EXTENSION beyond the reference ---------
 * A weighted mean with a per-frame linear map (gain, offset), a per-frame weight and a per-pixel coverage weight, and a
 * device pass that estimates the gains and offsets from the overlap with frame 0.
 * Samples. As in the clipped combine: per destination pixel and channel, s_i is the value the mean fold adds for table
 * entry i. Entry 0 is frame 0 through the identity, then the kept frames in ascending index (in stk_weighted_stack and
 * stk_overlap_moments: the included frames in index order under the caller's matrices). The fold's warp, border mode and
 * value, alpha and warp_subpixel_bits apply.
 * Coverage weight kappa_i(x, y), one per pixel and entry, not per channel. It is the sample the same fold produces for a
 * frame of the same size whose every value is 1.0f, with alpha = 1, BORDER_CONSTANT and border value 0: the bilinear
 * weight that falls on in-frame taps, computed by the very lerp chain (or the classic four-weight sum) that computes s_i.
 * It is exactly 1.0f wherever all four taps are inside and 0 where none is. A non-finite coordinate gives 0. With
 * coverage = 0, kappa_i = 1 by definition and the border samples count, as in the mean. With coverage = 1 the fold must
 * run under BORDER_CONSTANT with border value 0 in every channel; anything else is STK_INVALID_PARAMS. Only then is s_i
 * the premultiplied sum that belongs to kappa_i.
 * Combine. f32, each operation rounded on its own, `/` correctly rounded, entries in fold order:
 *   num_c = 0;  den = 0
 *   for each entry i:   v = s_i,c * g_i,c + o_i,c * kappa_i
 *                       num_c = num_c + w_i * v
 *                       den   = den   + w_i * kappa_i
 *   out_c = den > 0 ? num_c / den : 0;     coverage_out (optional, w x h f32, in the location of `out`) = den
 * g, o are per frame and channel, w is per frame. w_i must be finite and >= 0, g and o finite; otherwise
 * STK_INVALID_PARAMS. The same status results if every included w_i is 0.
 * Overlap moments (the estimator's input). For entry i >= 1 and channel c, take the destination pixels with
 * x % step == 0, y % step == 0 and kappa_i == 1.0f. kappa_i here is always the BORDER_CONSTANT one, whatever the fold's
 * border mode. With X = (double)s_i,c and Y = (double)s_0,c, the six f64 values are n, sum X, sum Y, sum X^2, sum Y^2,
 * sum XY. The products are formed in f64, so each term is exact and only the order of summation is free. The order is
 * fixed by the geometry and the step alone (per-wave partials written out and reduced in index order, no floating-point
 * atomics): the same bits on every call, whatever the options.
 * Estimator, on the host in f64, results rounded to f32. With mx = sum X / n, my = sum Y / n, vx = sum X^2 / n - mx^2 and vy
 * likewise:
 *   normalize 0 NONE:    gain 1,              offset 0
 *             1 OFFSET:  gain 1,              offset my - mx             (sky level)
 *             2 GAIN:    gain my / mx,        offset 0                   (exposure / transparency)
 *             3 LINEAR:  gain sqrt(vy / vx),  offset my - g mx           (g: the f64 gain, before rounding)
 * Entry 0 always has g = 1, o = 0. If n == 0, a denominator is <= 0, or a result is not finite, that frame and channel
 * fall back to (1, 0) and bit c of stk_frame_weight.flags is set. These are plain moments, not robust ones: a bright
 * transient inside the overlap biases them.
 * `out` must be tightly packed. stk_timing.finalize_ms of the whole-stack calls is the device time of the moments pass
 * plus the weighted fold (warp_ms etc. are the plain call's). A multi-device context runs these calls on its first
 * device. */
typedef struct {
    int32_t normalize;              /* 0 NONE, 1 OFFSET, 2 GAIN, 3 LINEAR */
    int32_t coverage;               /* 0: border samples count, kappa = 1;  1: divide by the covered weight */
    int32_t stat_step;              /* moments on every stat_step-th row and column, 1 .. 64; 0 = default (4) */
    int32_t reserved;               /* 0 */
} stk_weight_params;
typedef struct {
    float   gain[4];
    float   offset[4];
    float   weight;
    int32_t flags;                  /* bit c: channel c fell back to (1, 0) */
} stk_frame_weight;

/* ecc_match with the weighted combine (definition above): stats, warps, iterations and errors are those of stk_ecc_match
 * on the same input; the fold runs under BORDER_CONSTANT 0 with alpha = 1/255. weights_or_null: n weights by frame index,
 * NULL = all 1. coverage_or_null: den, width * height f32 in the location of `out`. applied_or_null: n records by frame
 * index, what the fold used. */
stk_status stk_ecc_match_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                  const stk_weight_params* weight, const float* weights_or_null, stk_image_f32* out,
                                  float* coverage_or_null, stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null);
/* keypoint_match with the weighted combine: stats and `dropped` as stk_keypoint_match; the samples are frame 0 and the
 * frames with status 0, folded with the params' border mode and value (coverage = 1 needs BORDER_CONSTANT 0). In
 * `applied` a dropped frame has weight 0 and gains 1, offsets 0. */
stk_status stk_keypoint_match_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                       float scale_down_width, const stk_weight_params* weight, const float* weights_or_null,
                                       stk_image_f32* out, int32_t* dropped, float* coverage_or_null,
                                       stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null);
/* The combine alone over caller-held warps, with the arguments of stk_clip_stack (definition above). per_frame: n records
 * by frame index, used as given (flags ignored; excluded frames' records are not read). coverage: 0 or 1. */
stk_status stk_weighted_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                              int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                              const stk_frame_weight* per_frame, int32_t coverage, stk_image_f32* out, float* coverage_or_null);
/* The overlap moments alone (definition above) of every included frame i >= 1 against frame 0, which must be included.
 * stat_step: 1 .. 64. moments: n x channels x 6 doubles on the host, frame index order, per channel n, sum X, sum Y,
 * sum X^2, sum Y^2, sum XY; frame 0 and excluded frames: zeros. */
stk_status stk_overlap_moments(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                               int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                               int32_t stat_step, double* moments);

/* ---- per-pixel weight maps and local-sharpness (lucky-region) stacking: an EXTENSION beyond the reference --------
 * The weighted combine above with a weight that varies per pixel, and a device pass that turns a frame into a local
 * quality map, so that a stack whose frames are each sharp somewhere else is as sharp as its sharpest frame everywhere.
 * Local quality map Q_i of frame i. 8-bit input only, in the frame's own pixel grid, integer arithmetic throughout:
 *   g          the integer grey of the frame: stk_grey's value bit for bit. A one-channel frame is taken as it is; the
 *              fourth channel of BGRA is ignored.
 *   r101(p, n) OpenCV's borderInterpolate(p, n, BORDER_REFLECT_101), iterated until the index is inside; n == 1 gives 0.
 *   ml(x, y)   = |2 g(x,y) - g(r101(x-1,w), y) - g(r101(x+1,w), y)| + |2 g(x,y) - g(x, r101(y-1,h)) - g(x, r101(y+1,h))|:
 *              the per-pixel term of LAPM, 0 .. 1020.
 *   mlT        = ml >= threshold ? ml : 0   (Nayar's sum-modified-Laplacian threshold: without it sensor noise, whose ml
 *              is small but everywhere, dilutes the measure).
 *   Q(x, y)    = the sum over dy, dx in [-radius, radius] of mlT(r101(x+dx, w), r101(y+dy, h)), stored as f32. It is at
 *              most 1020 x 31^2 = 980 220 < 2^24: every value is an exactly represented integer, and no tiling,
 *              summation order or launch shape can change a bit.
 * Local-weighted fold. The samples s_i,c, the fold order, alpha, warp, warp_subpixel_bits, warp_interpolation and the
 * coverage weight kappa_i are exactly those of the weighted combine with coverage = 1. The fold must run under
 * BORDER_CONSTANT with border value 0 in every channel; anything else is STK_INVALID_PARAMS, because a weight taken
 * outside a frame means nothing. Per destination pixel, entries in fold order; all values f32, each operation rounded on
 * its own, `/` correctly rounded:
 *   omega_i = the sample the LINEAR fold gives for plane map_i taken as a one-channel f32 frame of the source size, at
 *             this entry's coordinates, alpha = 1, BORDER_CONSTANT 0: the same lerp chain, or under warp_subpixel_bits = 5
 *             the classic four-weight sum. Always bilinear, also under STK_INTER_CUBIC: negative lobes would make
 *             negative weights.
 *   b     = omega_i + floor * kappa_i
 *   u     = b;  repeated (power - 1) times: u = u * b
 *   W     = w_i * u
 *   v_c   = s_i,c * g_i,c + o_i,c * kappa_i
 *   num_c = num_c + W * v_c
 *   den   = den + W * kappa_i
 *   out_c = den > 0 ? num_c / den : 0;     den_out (optional, w x h f32, in the location of `out`) = den
 * g, o, w are the stk_frame_weight records of the weighted combine and follow its validity rules. On the rim s, omega and
 * kappa are all premultiplied by the same coverage, so a constant scene comes back constant up to round-off. The floor
 * keeps a pixel that no frame finds sharp (a flat sky: every Q is 0) a plain coverage-weighted mean instead of 0 / 0. Map
 * values are expected finite and >= 0; they are not checked, and what they produce follows from the arithmetic above.
 * Entry 0 is frame 0 through the identity, so omega_0 = map_0 exactly. A multi-device context runs these calls on its
 * first device. */
typedef struct {
    int32_t radius;                 /* box window (2 radius + 1)^2 of the local sum: 1 .. 15 */
    int32_t threshold;              /* modified-Laplacian values below it count 0: 0 .. 1020 */
    int32_t power;                  /* the weight is the quality to this power: 1 .. 4 */
    float   floor;                  /* added to the quality before the power: finite, >= 0 */
    int32_t reserved[2];            /* 0 */
} stk_local_params;

/* The maps alone: Q of every frame in device passes over the stack. frames: 8-bit, 1, 3 or 4 channels, host or device
 * memory, any row stride (a frame whose base address or row stride is no multiple of 4 is read byte by byte: same bits,
 * slower); host frames are copied over in batches that fit the context's frame workspace. maps: n planes, width x
 * height f32, tightly packed, in frames->location. power and floor are validated but unused. 16-bit and f32 frames:
 * STK_NOT_IMPLEMENTED. stk_timing.prep_ms is the device time of the pass (for host frames with their copies). */
stk_status stk_local_sharpness(stk_ctx* ctx, const stk_frames* frames, const stk_local_params* local, float* const* maps);
/* The fold alone over caller-held warps and caller-held maps, with the arguments of stk_weighted_stack. The maps may be
 * any non-negative weights: Q, a trail mask, a vignetting weight, an inverse variance. Any depth, 1 / 3 / 4 channels.
 * maps: n planes (width x height f32, tightly packed) by frame index, in frames->location; planes of excluded frames
 * are not read. per_frame_or_null: NULL = gain 1, offset 0, weight 1. floor, power: as in stk_local_params. */
stk_status stk_local_weighted_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                    int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                    const stk_frame_weight* per_frame_or_null, const float* const* maps, float floor,
                                    int32_t power, stk_image_f32* out, float* den_or_null);
/* stk_ecc_match_weighted / stk_keypoint_match_weighted with the local-weighted fold: stats, warps, iteration counts,
 * `dropped` and errors are the plain call's; gains and offsets come from the overlap-moments pass under weight->normalize;
 * weight->coverage must be 1, else STK_INVALID_PARAMS. The maps of the frames that enter the fold are computed on the
 * device from the full-size frames, also under scale_down_width (n_entries x width x height x 4 bytes of device memory;
 * a failed allocation is STK_HIP_ERROR with the byte count in stk_last_error). By definition the result is
 * stk_local_weighted_stack with the stats' warps, the `applied` records and stk_local_sharpness's maps, bit for bit.
 * 8-bit BGR(A) frames only (16-bit, f32: STK_NOT_IMPLEMENTED). stk_timing.finalize_ms is the device time of the map
 * pass plus the moments pass plus the fold. */
stk_status stk_ecc_match_local_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                        const stk_weight_params* weight, const float* weights_or_null,
                                        const stk_local_params* local, stk_image_f32* out, float* den_or_null,
                                        stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_local_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                             float scale_down_width, const stk_weight_params* weight, const float* weights_or_null,
                                             const stk_local_params* local, stk_image_f32* out, int32_t* dropped,
                                             float* den_or_null, stk_frame_weight* applied_or_null,
                                             stk_frame_stats* stats_or_null);

/* ---- local alignment: per-frame displacement fields on a node grid: an EXTENSION beyond the reference -------------
 * Every other alignment here is one global map per frame. The atmosphere moves each part of a frame by its own one to
 * three pixels, which no homography removes; this section measures, per frame, a residual displacement on a grid of nodes
 * on top of the frame's global warp ("alignment points"), and folds through it. w x h is the destination size, which is
 * frame 0's; sw x sh the source frames' (all frames of a stk_frames share one geometry, so sw = w and sh = h).
 * Grid. gw = (w - 1 + step - 1) / step + 1, gh likewise from h (stk_mesh_grid). Node (j, k) sits at destination pixel
 *   (cx, cy) = (k step, j step); the last column and row may lie on or beyond the image edge. A field is gh x gw x 2 f32
 *   (dx, dy interleaved), tightly packed; a status plane is gh x gw int32.
 * Estimation ("local align"). 8-bit frames of 1, 3 or 4 channels. g_i is stk_grey's integer grey of frame i (a one-channel
 *   frame as it is; the fourth channel of BGRA ignored). For an included frame i >= 1, M_i is the fold's own f32
 *   destination -> source matrix: the forward warp inverted in double (cv::invert's adjugate, or invertAffineTransform),
 *   then cast to f32. Template gradients, exact integers: Tx(x,y) = g_0(x+1,y) - g_0(x-1,y), Ty(x,y) = g_0(x,y+1) - g_0(x,y-1).
 *   Per node the patch P is the set of integer pixels with |x - cx| <= radius, |y - cy| <= radius, 1 <= x <= w - 2 and
 *   1 <= y <= h - 2. P empty: status -1. Otherwise d = (0, 0) in f32, and for it = 1 .. max_iters:
 *   1. per pixel of P, in f32, each operation rounded on its own: fx = (float)x + dx, fy = (float)y + dy; (X, Y), finite,
 *      ix, iy, ax, ay exactly the fold's at (fx, fy) under warp_subpixel_bits = 0 with M_i and is_affine (fma chains, true
 *      division, floor; finite = |X| < 1e9 and |Y| < 1e9). The pixel is live iff finite && ix >= 0 && ix + 1 <= sw - 1 &&
 *      iy >= 0 && iy + 1 <= sh - 1. I = the fold's lerp chain over (float)g_i at the four taps: t0 = fma(ax, p01 - p00, p00),
 *      t1 = fma(ax, p11 - p10, p10), I = fma(ay, t1 - t0, t0). e = I - (float)g_0(x,y).
 *   2. over the live pixels, in f64: n, Sxx = sum Tx^2, Sxy = sum Tx Ty, Syy = sum Ty^2 (integers, exact), bx = sum Tx e,
 *      by = sum Ty e (every product exact; the order of the additions is the kernel's, and it is fixed: a lane's pixels in
 *      patch order, then a xor-shuffle tree over the wave).
 *   3. 2 n < |P|: status -2.
 *   4. lam = 0.5 ((Sxx + Syy) - sqrt((Sxx - Syy)^2 + 4 Sxy^2)), det = Sxx Syy - Sxy^2, in f64, each operation rounded on
 *      its own. det <= 0 or lam < (4 min_eig) n: status -3 (the factor 4: the gradients are the unscaled differences).
 *   5. Dx = 2 (Syy bx - Sxy by) / det, Dy = 2 (Sxx by - Sxy bx) / det; dx = (float)((double)dx - Dx), dy likewise.
 *   6. dx^2 + dy^2 (in f64) > max_shift^2, or not finite: status -4.
 *   7. Dx^2 + Dy^2 (in f64) < epsilon^2: stop.
 *   The status is the number of iterations run, 1 .. max_iters; a node that exhausts max_iters is valid and keeps its last
 *   d. An invalid node has d = (0, 0). Frame 0 and excluded frames get no field: their planes are not written.
 *   This is inverse-compositional Lucas-Kanade for a translation in DESTINATION space: the warped frame W(p) = I_i(M_i p)
 *   is matched to frame 0 at p + d, so the fold only has to move the destination coordinate before it applies its matrix.
 * Fill. `fill` Jacobi passes over each frame's grid. m = 1 for valid nodes; k = [1 2 1]^T [1 2 1]. For every node with
 *   m = 0, over its in-grid 3 x 3 neighbours with m = 1 in row-major order, in f32: den = den + k, num_c = num_c + k d_c;
 *   den > 0: d = num / den and the node counts as valid from the next pass on. Valid nodes never change. The status plane
 *   keeps the estimation's codes. (No smoothing of valid nodes: a 3 x 3 binomial smoothing made the prototype worse.)
 * Mesh fold. Destination pixel (x, y), table entry i with field D: k = x / step, j = y / step, k1 = min(k + 1, gw - 1),
 *   j1 = min(j + 1, gh - 1); u = (float)(x - k step) * (1.0f / step), v likewise (both exact); per component c:
 *   t0 = fma(u, D[j][k1][c] - D[j][k][c], D[j][k][c]), t1 the same on row j1, d_c = fma(v, t1 - t0, t0);
 *   fx = (float)x + d_0, fy = (float)y + d_1. Everything after that is the existing fold, unchanged: coordinates, sample,
 *   border, alpha, kappa, and the local-weighted fold's omega at the displaced coordinates. Frame 0 has no field (its plane
 *   is not read). A zero field returns the plain fold's bits. Field values are expected finite and are not checked.
 *   warp_subpixel_bits = 5: STK_INVALID_PARAMS. warp_interpolation = STK_INTER_CUBIC: STK_NOT_IMPLEMENTED for the mesh
 *   folds (the bicubic mesh fold is a follow-up). A multi-device context runs these calls on its first device. */
typedef struct {
    int32_t step;       /* node spacing in destination pixels: 8, 16, 32, 64, 128 or 256 (a power of two) */
    int32_t radius;     /* patch half size, patch = (2 radius + 1)^2: 2 .. 32 */
    int32_t max_iters;  /* 1 .. 32 */
    float   epsilon;    /* stop when |delta|^2 < epsilon^2; finite, >= 0 (0: always max_iters iterations) */
    float   max_shift;  /* a node whose |d| exceeds it is invalid: finite, > 0, <= 64 */
    float   min_eig;    /* texture threshold, grey levels^2 per live pixel: finite, >= 0 */
    int32_t fill;       /* hole-filling passes: 0 .. 16 */
    int32_t reserved;   /* 0 */
} stk_mesh_params;

/* ---- coarse-to-fine local alignment (the *_pyramid calls below): shifts beyond a patch's capture range ---------------
 * The estimation above starts every node at d = (0, 0) and follows the gradient of one patch: beyond a fraction of the
 * finest scene period it settles in a wrong minimum with a positive status. The pyramid form runs the same estimation on
 * `levels` = 1 .. 4 levels, coarsest first, and seeds each level with the one above. Level l has scale s = 2^l.
 * Level images. g_i^0 is stk_grey's integer grey, as above. g_i^l(x, y) = (g^{l-1}(2x, 2y) + g^{l-1}(2x+1, 2y) +
 *   g^{l-1}(2x, 2y+1) + g^{l-1}(2x+1, 2y+1) + 2) >> 2, stored as u8; w_l = w_{l-1} >> 1, h_l likewise (an odd last column
 *   or row is dropped). The planes are exact integers.
 * Level matrices. Pixel x of level l sits at full-resolution coordinate s x + (s - 1) / 2: C_l = [[s, 0, c], [0, s, c],
 *   [0, 0, 1]] with c = (s - 1) / 2. The destination -> source matrix of level l is C_l^-1 Minv_i C_l in double, Minv_i the
 *   double inverse of the single-level definition, then cast to f32. In operations, each rounded on its own, row r of
 *   A = Minv_i C_l is (m_r0 s, m_r1 s, (m_r0 c + m_r1 c) + m_r2), and rows 0 and 1 of the product are
 *   A_r (1 / s) - (c / s) A_2, row 2 is A_2 (an affine last row stays (0, 0, 1)). Level 0 is Minv_i itself.
 * Nodes. Every level uses the same gw x gh grid. Node (j, k) of level l is centred at the integer level pixel
 *   ((k step) >> l, (j step) >> l); its patch has the same `radius` in level pixels, limited to 1 <= x <= w_l - 2 and
 *   1 <= y <= h_l - 2.
 * Estimation at level l. Steps 1 - 7 above on g_0^l and g_i^l with w_l, h_l and the level matrix, but d starts at the
 *   node's seed instead of (0, 0), and max_shift is replaced by max_shift 2^-l (exact in f32), tested on the total d.
 *   epsilon, min_eig and max_iters are unchanged, in level pixels and level grey.
 * Carrying. Each node carries a validity bit m. The top level l = levels - 1 starts with seed (0, 0) and m_seed = 0. After
 *   the estimation at level l a node with status > 0 has its d and m = 1; any other node has d = seed and m = m_seed. The
 *   `fill` Jacobi passes then run on (d, m): the arithmetic of "Fill" above with m in place of status > 0. For the next
 *   level down, seed = 2 d (f32, exact) and m_seed = m after the fill.
 * Result. The field is level 0's d after its fill; the status plane is level 0's estimation codes. A node that fails at
 *   level 0 therefore keeps a negative code but carries the coarser level's measurement. levels = 1 is stk_local_align
 *   (estimation and fill) bit for bit.
 * Refusals, STK_INVALID_PARAMS: levels outside 1 .. 4; step >> (levels - 1) < 4; min(w, h) >> (levels - 1) < 16;
 *   everything stk_local_align refuses. 16-bit and f32 frames: STK_NOT_IMPLEMENTED.
 * The drizzle forms get no pyramid entry point: the fields of stk_local_align_pyramid go into stk_mesh_drizzle_stack as
 *   they are. */

/* The grid of a width x height destination. Bad arguments (a step that is no power of two in 8 .. 256, a NULL pointer):
 * STK_INVALID_PARAMS. */
stk_status stk_mesh_grid(int32_t width, int32_t height, int32_t step, int32_t* gw, int32_t* gh);
/* The fields alone. M: forward warps by frame index (9 doubles each), include_or_null, is_affine: as in stk_weighted_stack.
 * fields / status_or_null: n planes by frame index, in frames->location; entries for frame 0 and for excluded frames may
 * be NULL and are not written; status_or_null or single entries of it may be NULL. Host frames are copied over in batches
 * that fit the context's frame workspace. 16-bit and f32 frames: STK_NOT_IMPLEMENTED. stk_timing.align_ms is the device
 * time of the pass (estimation and fill). */
stk_status stk_local_align(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null, int32_t is_affine,
                           const stk_mesh_params* mesh, float* const* fields, int32_t* const* status_or_null);
/* The plain mean through the fields: the sums in fold order x (float)(1.0 / N), N = the included frames. Arguments as
 * stk_clip_stack's; any depth, 1 / 3 / 4 channels, border modes 0 .. 4. fields: n planes by frame index in
 * frames->location for the grid of `step`; those of frame 0 and of excluded frames are not read. `out` tightly packed. */
stk_status stk_mesh_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null, int32_t is_affine,
                          int32_t border_mode, const double* border_value, double alpha, const float* const* fields, int32_t step,
                          stk_image_f32* out);
/* stk_local_weighted_stack through the fields: its arguments, its checks, its arithmetic at the displaced coordinates. */
stk_status stk_mesh_local_weighted_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                         int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                         const stk_frame_weight* per_frame_or_null, const float* const* maps, float floor,
                                         int32_t power, const float* const* fields, int32_t step, stk_image_f32* out,
                                         float* den_or_null);
/* stk_ecc_match / stk_keypoint_match with local alignment: stats, warps, iteration counts, `dropped` and errors are the
 * plain call's. The fields of the frames that enter the fold are computed on the device from the full-size resident frames
 * with the stats' warps, also under scale_down_width. local_or_null == NULL: the result is stk_mesh_stack's (alpha 1 / 255;
 * BORDER_CONSTANT 0, or the keypoint parameters' border); otherwise stk_mesh_local_weighted_stack's with NULL records,
 * stk_local_sharpness's maps and local's floor and power (the keypoint parameters' border must then be BORDER_CONSTANT 0).
 * By definition the result equals those parts bit for bit. 8-bit BGR(A) frames only (16-bit, f32: STK_NOT_IMPLEMENTED).
 * stk_timing.finalize_ms is the device time of the field pass plus the map pass plus the fold. A failed device
 * allocation is STK_HIP_ERROR with the byte count in stk_last_error. */
stk_status stk_ecc_match_local_aligned(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                       const stk_mesh_params* mesh, const stk_local_params* local_or_null, stk_image_f32* out,
                                       stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_local_aligned(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                            float scale_down_width, const stk_mesh_params* mesh, const stk_local_params* local_or_null,
                                            stk_image_f32* out, int32_t* dropped, stk_frame_stats* stats_or_null);
/* Levels 1 .. levels - 1 of the box pyramid of ONE 8-bit frame (frames->n == 1; 1, 3 or 4 channels, any row stride):
 * planes[l] receives (w >> l) x (h >> l) bytes, tightly packed, in frames->location; planes[0] is not used. levels is
 * 2 .. 4 with min(w, h) >> (levels - 1) >= 1, else STK_INVALID_PARAMS. The pyramid kernel on its own, so that it can be
 * held to exact integers. */
stk_status stk_grey_pyramid(stk_ctx* ctx, const stk_frames* frame, int32_t levels, uint8_t* const* planes);
/* stk_local_align, coarse to fine (definition above): its arguments and conventions, plus `levels`. Host frames go through
 * the frame workspace in batches behind frame 0, whose pyramid is built once. stk_timing.prep_ms is the device time of the
 * pyramid pass, align_ms that of the levels' estimations and fills. A failed device allocation is STK_HIP_ERROR with the
 * byte count in stk_last_error. */
stk_status stk_local_align_pyramid(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                   int32_t is_affine, const stk_mesh_params* mesh, int32_t levels, float* const* fields,
                                   int32_t* const* status_or_null);
/* stk_ecc_match_local_aligned / stk_keypoint_match_local_aligned with the coarse-to-fine field pass: by definition the
 * plain call + stk_local_align_pyramid on the stats' warps + the mesh fold (with local_or_null: the map pass and the mesh
 * local-weighted fold), bit for bit. */
stk_status stk_ecc_match_local_aligned_pyramid(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                               float scale_down_width, const stk_mesh_params* mesh, int32_t levels,
                                               const stk_local_params* local_or_null, stk_image_f32* out,
                                               stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_local_aligned_pyramid(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                                    float scale_down_width, const stk_mesh_params* mesh, int32_t levels,
                                                    const stk_local_params* local_or_null, stk_image_f32* out, int32_t* dropped,
                                                    stk_frame_stats* stats_or_null);

/* ---- drizzle integration onto a finer or larger output grid: an EXTENSION beyond the reference --------------------
 * Variable-pixel linear reconstruction (Fruchter & Hook 2002). Every other combine writes onto frame 0's own grid and
 * samples by interpolation; this one has an output grid with its own scale, origin and size, shrinks every source pixel to
 * a "drop" of side pixfrac before it spreads it over the output pixels it overlaps, and records in a weight image how much
 * landed where. Formulated as a GATHER: one output pixel collects from the source pixels that reach it, entries in fold
 * order, no scatter, no atomics, the same bits on every call whatever the options. sw x sh is the source frames' size,
 * ow x oh the output's (taken from `out`), s = scale, p = pixfrac.
 * Output grid. The centre of output pixel (X, Y) lies at the frame-0 coordinate
 *   x0 = (X + 0.5) / s - 0.5 + origin_x,   y0 = (Y + 0.5) / s - 0.5 + origin_y.
 *   s = 1 with origin 0 is frame 0's own grid; a negative origin with a larger `out` is a canvas that extends past frame 0.
 * Coordinates. For table entry i (the included frames in index order; in the whole-stack forms frame 0 through the
 *   identity, then the kept frames) the host composes in double, each operation rounded on its own:
 *     inv = the fold's inverse of the forward matrix M_i (cv::invert's adjugate, or invertAffineTransform)
 *     g = 1.0 / (double)s;  tx = (0.5 * g - 0.5) + (double)origin_x;  ty = (0.5 * g - 0.5) + (double)origin_y
 *     per row r:  A[r][0] = inv[r][0] * g;  A[r][1] = inv[r][1] * g;  A[r][2] = (inv[r][0] * tx + inv[r][1] * ty) + inv[r][2]
 *   and rounds A to f32. (u, v) of output pixel (X, Y), `finite`, ix = floor u, iy = floor v and the fractions ax = u - ix,
 *   ay = v - iy are exactly the fold's under warp_subpixel_bits = 0 with matrix A at ((float)X, (float)Y): the same fma
 *   chains, the same true division for a homography, the same test finite = |u| < 1e9 and |v| < 1e9.
 *   warp_subpixel_bits = 5: every drizzle call is STK_INVALID_PARAMS, as for cubic. warp_interpolation is ignored: drizzle
 *   does not interpolate.
 * Everything below is f32 multiplies, adds, subtractions, one reciprocal, min and max, each rounded on its own (no fma);
 * min and max are C's fminf / fmaxf (a NaN operand gives the other one); `/` is correctly rounded.
 * Local coordinates. The nearest source pixel and the offset from it, so that no large magnitudes cancel:
 *   jn = ax >= 0.5f ? ix + 1 : ix;   d = ax >= 0.5f ? ax - 1.0f : ax      (exact; d in [-0.5, 0.5]; jn = floor(u + 0.5), d = u - jn)
 *   kn and e likewise from iy and ay.
 * Footprint. The output pixel's half-extent in source pixels is half the bounding box of its image under the local
 *   Jacobian: hx = (|du/dX| + |du/dY|) / 2, hy = (|dv/dX| + |dv/dY|) / 2, both clamped to [0, hmax], hmax = 1.5f - 0.5f * p.
 *   With |d| <= 0.5 the clamp keeps the footprint [d - hx, d + hx] inside (-2 + p/2, 2 - p/2): it never reaches the drop of
 *   source pixel jn - 2 or jn + 2, so THREE TAPS PER AXIS ARE ALWAYS SUFFICIENT.
 *   Affine entry (constants of the entry, on the host in double from the f32 values of A, rounded to f32, then the clamp):
 *     hx = fminf((float)(0.5 * (|A00| + |A01|)), hmax);   hy = fminf((float)(0.5 * (|A10| + |A11|)), hmax)
 *   Perspective entry (per pixel):
 *     uu = (float)jn + d;  vv = (float)kn + e;  W = (A20 * (float)X + A21 * (float)Y) + A22;  rw = 1.0f / |W|
 *     hx = fminf(((|A00 - uu * A20| + |A01 - uu * A21|) * rw) * 0.5f, hmax)
 *     hy = fminf(((|A10 - vv * A20| + |A11 - vv * A21|) * rw) * 0.5f, hmax)
 * Taps and weights. hp = 0.5f * p. For a in {-1, 0, 1}:
 *     ox_a = fmaxf(0, fminf(d + hx, (float)a + hp) - fmaxf(d - hx, (float)a - hp))
 *   and ox_a = 0 if column jn + a is outside [0, sw) or the coordinate is not finite; oy_b likewise from e, hy, kn and sh.
 *   Tap (jn + a, kn + b) is LIVE iff ox_a > 0 and oy_b > 0 and, with maps, the entry's map value there is > 0. Its weight
 *   is wgt = ox_a * oy_b, with maps (ox_a * oy_b) * map value. Only live taps are read. There is no border mode: what is
 *   outside a frame contributes nothing. maps: sw x sh f32 planes by frame index exactly as stk_local_weighted_stack takes
 *   them, read at the integer tap, no interpolation; a NULL plane (or maps == NULL) means all ones. This is how bad-pixel
 *   masks and inverse-variance maps enter: a pixel whose map value is 0 is never read, whatever it holds.
 * Combine. Entries in fold order, live taps row-major (b outer, a inner):
 *     num_c = 0;  den = 0
 *     for each entry i with w_i > 0:
 *         s_c = 0;  k = 0
 *         for each live tap:  t = (float)src[tap][c] * alpha;  s_c = s_c + wgt * t;  k = k + wgt
 *         if k > 0:  num_c = num_c + w_i * (s_c * g_i,c + o_i,c * k);  den = den + w_i * k
 *     out_c = den > 0 ? num_c / den : fill;     den_out (optional, ow x oh f32, in the location of `out`) = den
 *   g, o, w are the stk_frame_weight records of the weighted combine (NULL = gain 1, offset 0, weight 1). den is the
 *   drizzle weight image.
 * Consequences.
 *   - s = 1, p = 1, origin 0, no maps, a pure translation: hx = hy = 0.5 and ox_a = max(0, 1 - |d - a|), the bilinear
 *     weights. The result is the mathematics of the weighted combine with coverage = 1, not its bits (the order differs).
 *   - Small p with few frames leaves holes: den = 0 and out = fill.
 *   - The bounding-box footprint over-covers under rotation: this is the "turbo" approximation of the drizzle literature,
 *     not polygon clipping. The clamp cuts the footprint of a map that shrinks the output by more than 3 - p per axis.
 * Validation, on the host before any launch; anything else is STK_INVALID_PARAMS: s finite in [1, 4]; p finite in (0, 1];
 * origins and fill finite; reserved = 0; 1 <= ow, oh <= 32768; out->channels = the frames'; `out` tightly packed; weights
 * finite and >= 0 and at least one included weight > 0; gains and offsets finite. stk_timing.finalize_ms is the device
 * time of the drizzle launch (in the whole-stack forms warp_ms etc. are the plain call's). A multi-device context runs
 * these calls on its first device. */
typedef struct {
    float   scale, pixfrac;         /* output pixels per frame-0 pixel: 1 .. 4;  drop side in source pixels: (0, 1] */
    float   origin_x, origin_y;     /* frame-0 coordinate of the output grid's corner pixel at scale 1 (see above) */
    float   fill;                   /* value of output pixels nothing landed on: finite */
    int32_t reserved;               /* 0 */
} stk_drizzle_params;

/* Drizzle over caller-held warps. M, include_or_null, is_affine, alpha: as in stk_clip_stack. Any depth, 1 / 3 / 4 channels.
 * Frames and maps are in frames->location (host frames and their maps are copied over), `out` and den_or_null in
 * out->location. per_frame_or_null: n records by frame index (flags ignored; excluded frames' records are not read).
 * maps_or_null: n plane pointers by frame index, single entries may be NULL. out: ow x oh x channels, tightly packed. */
stk_status stk_drizzle_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                             int32_t is_affine, double alpha, const stk_drizzle_params* drizzle,
                             const stk_frame_weight* per_frame_or_null, const float* const* maps_or_null, stk_image_f32* out,
                             float* den_or_null);
/* stk_ecc_match / stk_keypoint_match with the drizzle combine: the stack is aligned exactly as the plain call aligns it
 * (stats, warps, iteration counts, `dropped` and errors are the plain call's), then frame 0 (identity) and the kept frames
 * (keypoint: status 0) are drizzled from the full-size resident frames with alpha = 1 / 255, all weights 1 and no maps. The
 * keypoint parameters' border mode is not used. By definition the result equals stk_drizzle_stack on the stats' warps bit
 * for bit. 8-bit BGR(A) frames, as the plain calls take them. */
stk_status stk_ecc_match_drizzle(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                 const stk_drizzle_params* drizzle, stk_image_f32* out, float* den_or_null,
                                 stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_drizzle(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                      float scale_down_width, const stk_drizzle_params* drizzle, stk_image_f32* out,
                                      int32_t* dropped, float* den_or_null, stk_frame_stats* stats_or_null);

/* ---- mesh-displaced drizzle: drizzle through local-alignment fields: an EXTENSION beyond the reference -------------
 * The two sections above in one combine: the drizzle of a stack whose frames carry, on top of their global warp, the
 * residual displacement fields of stk_local_align. The grid map of drizzle is a scaling and a shift, so moving the frame-0
 * coordinate of an output pixel by d is moving the output coordinate by s d: the host's composed matrix A_i stays as it
 * is, and the fold's fragment runs at the displaced output coordinate. s, g, tx, ty and A_i are the drizzle definition's
 * own; D_i is entry i's field, gh x gw x 2 f32 on the grid of stk_mesh_grid(sw, sh, step), exactly the planes
 * stk_local_align writes; shift = log2 step. Everything is f32 with each operation rounded on its own, except where fma is
 * written.
 * Frame-0 coordinate of output pixel (X, Y):  x0 = (float)X * (float)g + (float)tx;  y0 = (float)Y * (float)g + (float)ty
 *   (at s = 1, origin 0: (float)X and (float)Y exactly).
 * Field sample. xc = fminf(fmaxf(x0, 0), (float)(sw - 1));  k = (int)xc >> shift;  k1 = min(k + 1, gw - 1);
 *   u = (xc - (float)(k << shift)) * (1.0f / step);  yc, j, j1 and v likewise from y0, sh and gh. Per component c:
 *     t0 = fma(u, D[j][k1][c] - D[j][k][c], D[j][k][c]);  t1 the same on row j1;  d_c = fma(v, t1 - t0, t0)
 *   the mesh fold's own chain. Outside frame 0's image (a canvas) the field is that of the nearest edge. Every field address
 *   comes from the clamped coordinate, never from a field value.
 * Field slopes, from the differences the lerp already has. With a_c = D[j][k1][c] - D[j][k][c], b_c the same on row j1,
 *   p_c = D[j1][k][c] - D[j][k][c] and q_c the same on column k1:
 *     dxd_c = fma(v, b_c - a_c, a_c) * (1.0f / step);   dyd_c = fma(u, q_c - p_c, p_c) * (1.0f / step)
 *   and dxd_c = 0 where x0 != xc (the coordinate was clamped along x), dyd_c = 0 where y0 != yc. (On a last node column
 *   that lies on the image's last column k1 = k: a_c = b_c = 0 and the slope along x is 0 there; rows likewise.)
 * Displaced coordinate.  Xd = (float)X + (float)s * d_0;  Yd = (float)Y + (float)s * d_1.  (u, v), finite, ix, iy, ax, ay are
 *   the fold's under warp_subpixel_bits = 0 with A_i at (Xd, Yd) instead of ((float)X, (float)Y); the perspective W of the
 *   footprint uses (Xd, Yd) too.
 * Footprint. The un-halved rows of drizzle's local Jacobian times the displacement's own Jacobian E = I + grad d:
 *     e00 = 1.0f + dxd_0;  e01 = dyd_0;  e10 = dxd_1;  e11 = 1.0f + dyd_1
 *   Affine entry:       hx = fminf((|A00 * e00 + A01 * e10| + |A00 * e01 + A01 * e11|) * 0.5f, hmax);  hy the same from A10, A11
 *   Perspective entry:  j0 = A00 - uu * A20;  j1 = A01 - uu * A21 (uu, vv, W, rw as in drizzle, at the displaced coordinates);
 *                       hx = fminf(((|j0 * e00 + j1 * e10| + |j0 * e01 + j1 * e11|) * rw) * 0.5f, hmax);  hy the same from vv and
 *                       A10, A11. (rw multiplies the sum, as in drizzle, not each row: a zero field then gives drizzle's bits.)
 *   Without the slope term den is no area measure where a field stretches or compresses.
 * Everything after that is the drizzle definition, unchanged: local coordinates, overlaps, taps, maps, records, combine, fill.
 * An entry whose field pointer is NULL (frame 0, or any the caller leaves out) is plain drizzle arithmetic, including the
 * host's affine footprint table. Field values are expected finite and are not checked; a non-finite value makes the
 * coordinate non-finite, so every overlap is 0 and the entry contributes nothing at that pixel.
 * Consequences: NULL fields, or all-zero fields, return stk_drizzle_stack's bits; at s = 1, origin 0 the displaced
 * coordinates inside frame 0 are the mesh fold's bits; two calls return the same bits. */

/* stk_drizzle_stack through the fields: its arguments and checks, plus `fields` / `step` as stk_mesh_stack takes them: n
 * plane pointers by frame index, the planes in frames->location; those of frame 0 and of excluded frames are not read, a
 * NULL entry means no displacement. fields == NULL, or a step that is no power of two in 8 .. 256: STK_INVALID_PARAMS, as
 * is warp_subpixel_bits = 5. */
stk_status stk_mesh_drizzle_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                  int32_t is_affine, double alpha, const stk_drizzle_params* drizzle,
                                  const stk_frame_weight* per_frame_or_null, const float* const* maps_or_null,
                                  const float* const* fields, int32_t step, stk_image_f32* out, float* den_or_null);
/* stk_ecc_match_drizzle / stk_keypoint_match_drizzle with local alignment: the plain call, then stk_local_align's field
 * pass on the full-size resident frames with the stats' warps, then the mesh drizzle of frame 0 (no field) and the kept
 * frames. By definition the result equals stk_local_align + stk_mesh_drizzle_stack on the stats' warps bit for bit. 8-bit
 * BGR(A) frames only (16-bit, f32: STK_NOT_IMPLEMENTED). Device memory is reserved before the plain call runs; a failed
 * allocation is STK_HIP_ERROR with the byte count in stk_last_error. stk_timing.finalize_ms is the device time of the
 * field pass plus the drizzle launch. A multi-device context runs these calls on its first device. */
stk_status stk_ecc_match_local_aligned_drizzle(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                               float scale_down_width, const stk_mesh_params* mesh,
                                               const stk_drizzle_params* drizzle, stk_image_f32* out, float* den_or_null,
                                               stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_local_aligned_drizzle(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                                    float scale_down_width, const stk_mesh_params* mesh,
                                                    const stk_drizzle_params* drizzle, stk_image_f32* out, int32_t* dropped,
                                                    float* den_or_null, stk_frame_stats* stats_or_null);

/* ---- blot-and-compare rejection maps for drizzle: an EXTENSION beyond the reference ------------------------------
 * Drizzle has no rejection of its own: a trail, a cosmic-ray hit or a hot pixel of one frame goes straight into num / den.
 * This pass makes the per-frame masks that keep them out (Fruchter & Hook's `blot` and `driz_cr`): a clean image on frame
 * 0's grid (a robust combine, e.g. stk_quantile_stack_weighted at 0.5) is resampled ("blotted") into each frame's own pixel
 * grid, the frame is compared with that model under a tolerance that grows with the model's local gradient (an undersampled
 * frame legitimately differs from an interpolated model at edges), and the failures, grown by one pixel under a tighter
 * tolerance, become a sw x sh f32 plane per frame that stk_drizzle_stack, stk_mesh_drizzle_stack and
 * stk_local_weighted_stack take as `maps`.
 * All arithmetic is f32, each operation rounded on its own, no contraction except where fma is written; sqrt is correctly
 * rounded; fmaxf is C's. sw x sh is the frames' geometry and the clean image's (frame 0's grid is the destination grid), cn
 * the channel count (all cn channels are judged). C is the clean image, sh x sw x cn f32, tightly packed, at the level of
 * normalised samples; cnt an optional sh x sw int32 plane, exactly what stk_quantile_stack_weighted writes to `counts`.
 * For an included frame i with forward matrix M_i and record (g, o) (per_frame_or_null; NULL = 1, 0), for EVERY lattice
 * point (x, y), integer, also outside the frame:
 * Blot coordinate. (X, Y), finite, ix, iy, ax, ay are exactly the fold's under warp_subpixel_bits = 0 at ((float)x, (float)y)
 *   with the matrix F_i: the nine doubles of the FORWARD matrix cast to f32, NOT inverted (the forward map takes frame-i
 *   pixels to frame-0 coordinates). is_affine selects the division as in the fold. warp_subpixel_bits = 5:
 *   STK_INVALID_PARAMS, as for drizzle. warp_interpolation is ignored: the model is always bilinear.
 * Valid. valid(x, y) iff finite && ix >= 0 && ix + 1 <= sw - 1 && iy >= 0 && iy + 1 <= sh - 1 and, with cnt, cnt >= min_count
 *   at all four taps. Only valid points read C or cnt: every address is inside by construction.
 * Model. t0 = fma(ax, C01 - C00, C00);  t1 = fma(ax, C11 - C10, C10);  B_c = fma(ay, t1 - t0, t0)    (the fold's lerp chain;
 *   C00 = C[iy][ix][c], C01 = C[iy][ix + 1][c], C10 = C[iy + 1][ix][c], C11 = C[iy + 1][ix + 1][c]).
 * Gradient. D_c(x, y) = the maximum of |B_c(n) - B_c(x, y)| over those of the four neighbours n = (x-1, y), (x+1, y),
 *   (x, y-1), (x, y+1), in that order, that are valid; D_c starts from 0 (no valid neighbour: 0), D_c = fmaxf(D_c, |..|). A
 *   neighbour may lie outside the frame's pixel grid: B is a function of the lattice point, not of the frame.
 * Sample. u_c = ((float)src[y][x][c] * alpha) * g_c + o_c.
 * Noise. sigma_c = sqrt(rn * rn + pg * fmaxf(B_c, 0)), rn = read_noise, pg = poisson_gain, both in the units of the samples
 *   after alpha.
 * Judged. judged(x, y) iff valid && 0 <= x < sw && 0 <= y < sh and, with maps_in and a non-NULL entry, maps_in[i][y][x] > 0.
 * First flag. e_c = |u_c - B_c|;  f1 = judged && any c with e_c > scale1 * D_c + snr1 * sigma_c (the products and the sum
 *   each rounded). A NaN makes the comparison false: the pixel is kept.
 * Grow. f2 = judged && (any f1 in the 3 x 3 around (x, y), itself included) && any c with e_c > scale2 * D_c + snr2 * sigma_c.
 * Result. rej = f1 || f2;  maps_out[i][y][x] = rej ? 0 : (maps_in entry ? its value : 1.0f). An unjudged pixel keeps its
 *   input value (or 1): what cannot be compared is not rejected. rejected[i] = the number of pixels with rej,
 *   judged_count[i] = the number judged: int64, host memory, optional, 0 for excluded frames; exact integers, so any
 *   reduction order gives the same values. Frame 0 is processed like every other frame: a trail in the reference is
 *   rejected too. Planes of excluded frames are not written. maps_out[i] may BE maps_in[i] (in place; the definition reads a
 *   pixel's own input value only, the engine works from a copy of such a plane); planes that overlap in any other way are
 *   not supported.
 * Consequences. An identity matrix with C equal to the frame rejects nothing. An integer translation blots exactly
 *   (ax = ay = 0): B is C shifted. On a constant C the gradient is 0 and the test is |u - C| > snr * rn (pg = 0). The
 *   one-pixel ring of frame-0 coverage (ix + 1 > sw - 1) is never judged; on a 1 x 1 stack nothing is. Two calls return the
 *   same bits.
 * Validation, on the host before any launch; anything else is STK_INVALID_PARAMS with a message: snr1, snr2 finite and > 0;
 * scale1, scale2, read_noise, poisson_gain finite and >= 0 (read_noise = poisson_gain = 0 is allowed: then only the
 * gradient term tolerates anything); min_count >= 0; reserved = 0; gains and offsets finite (the records are checked as
 * stk_weighted_stack checks them; the weights themselves are not used). */
typedef struct {
    float   snr1, snr2;          /* > 0, finite; astrodrizzle's defaults are 4, 3 */
    float   scale1, scale2;      /* >= 0, finite; defaults 1.2, 0.7 */
    float   read_noise;          /* >= 0, finite */
    float   poisson_gain;        /* >= 0, finite */
    int32_t min_count;           /* >= 0; with a counts plane, a clean pixel with fewer samples judges nothing; 3 recommended */
    int32_t reserved;            /* 0 */
} stk_reject_params;

/* The pass over caller-held warps. M, include_or_null, is_affine, alpha: as in stk_drizzle_stack. Any depth, 1 / 3 / 4
 * channels, any row stride. `clean`, clean_counts_or_null, the planes of maps_in_or_null (n pointers by frame index, single
 * entries may be NULL = all ones) and of maps_out (n pointers by frame index; those of included frames must not be NULL)
 * are in frames->location. rejected_or_null, judged_or_null: n int64 each, host memory. stk_timing.finalize_ms is the device
 * time of the pass. A multi-device context runs it on its first device. */
stk_status stk_reject_maps(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                           int32_t is_affine, double alpha, const stk_frame_weight* per_frame_or_null,
                           const float* clean, const int32_t* clean_counts_or_null, const stk_reject_params* reject,
                           const float* const* maps_in_or_null, float* const* maps_out,
                           int64_t* rejected_or_null, int64_t* judged_or_null);
/* stk_ecc_match_drizzle / stk_keypoint_match_drizzle with rejection. In this order: (1) the plain call: its stats, warps,
 * `dropped` and errors are the result's; (2) the records exactly as stk_ecc_match_weighted / stk_keypoint_match_weighted
 * make them (the moments pass and the estimator under weight->normalize, the caller's weights_or_null by frame index);
 * (3) the clean image: stk_quantile_stack_weighted at quantile = 0.5, coverage = 1, BORDER_CONSTANT 0, alpha = 1 / 255 with
 * those records over frame 0 (identity) and the kept frames, with its `counts`; (4) stk_reject_maps with those counts and
 * reject->min_count, the records, alpha = 1 / 255 and no input maps; (5) stk_drizzle_stack with the records and the maps. By
 * definition the result equals those parts called one after another on the stats' warps, bit for bit: the image, den, the
 * maps and the counts. weight->coverage must be 1 (and, for the keypoint form, the parameters' border BORDER_CONSTANT 0, as
 * stk_keypoint_match_weighted asks under coverage); anything else is STK_INVALID_PARAMS. maps_or_null: n planes by frame
 * index in frames->location, entries may be NULL, receiving the maps the drizzle used (a dropped frame's plane is not
 * written). rejected_or_null: n int64, host. applied_or_null: the records, as stk_ecc_match_weighted returns them. 8-bit
 * BGR(A) frames only, as for the other whole-stack drizzle forms. Device memory is reserved before the plain call runs
 * (n x sw x sh x 4 bytes of maps, the clean image and its counts, plus what the median and the drizzle need); a failed
 * allocation is STK_HIP_ERROR with the byte count in stk_last_error. stk_timing.finalize_ms is the sum of the device times
 * of moments + median + reject + drizzle; warp_ms etc. stay the plain call's. A multi-device context runs these calls on
 * its first device. */
stk_status stk_ecc_match_drizzle_rejected(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                          float scale_down_width, const stk_drizzle_params* drizzle,
                                          const stk_weight_params* weight, const float* weights_or_null,
                                          const stk_reject_params* reject, stk_image_f32* out, float* den_or_null,
                                          float* const* maps_or_null, int64_t* rejected_or_null,
                                          stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_drizzle_rejected(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                               float scale_down_width, const stk_drizzle_params* drizzle,
                                               const stk_weight_params* weight, const float* weights_or_null,
                                               const stk_reject_params* reject, stk_image_f32* out, int32_t* dropped,
                                               float* den_or_null, float* const* maps_or_null, int64_t* rejected_or_null,
                                               stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null);

/* ---- normalised, coverage-aware sigma-clip and quantile stacking: an EXTENSION beyond the reference -------------
 * The two rejection combines with the per-frame gain, offset and weight and the coverage of the weighted combine: frames
 * are compared after each has been mapped onto frame 0's level, and a frame that does not cover a pixel is no sample of
 * it. Samples s_i, fold order, alpha, warp, border handling and warp_subpixel_bits are the clipped combine's; kappa_i is
 * the weighted combine's coverage weight (always the BORDER_CONSTANT one, whatever the fold's border mode); g, o are per
 * frame and channel, w per frame (stk_frame_weight), validated as stk_weighted_stack validates them. All arithmetic is
 * f32, each operation rounded on its own, `/` and sqrt correctly rounded, entries in fold order; max and min are C's
 * fmaxf / fminf (a NaN operand gives the other one).
 * Participation (one flag per pixel and entry, not per channel): entry i is a sample of the pixel iff w_i > 0 and, with
 * coverage = 1, kappa_i == 1.0f (all taps that carry weight are inside the frame). With coverage = 0 only w_i > 0 is
 * asked and border samples count. A partly covered sample (0 < kappa < 1) is a dimmed value that cannot be compared or
 * ranked, so it is left out. coverage = 1 puts no condition on the border mode or value: a border tap never reaches a
 * participating sample with non-zero weight.
 * Normalised sample: u = s * g_i,c + o_i,c.
 * Clip (kappa_low, kappa_high, iterations = T as in stk_clip_params):
 *   centre pass:  sw = 0; a = 0;  for each participating u: sw = sw + w; a = a + w * u
 *                 c = sw > 0 ? a / sw : 0;  L = -inf;  U = +inf
 *   passes t = 1 .. T + 1:  k = 0; sw = 0; a = 0; b = 0
 *                 for each participating u: d = u - c
 *                     if (L <= u && u <= U) { k += 1; sw = sw + w; a = a + w * d; b = b + w * (d * d); }
 *                 last pass: out = k > 0 ? c + a / sw : c;  counts = k;  kept_weight = sw   (per pixel and channel)
 *                 otherwise, if k >= 3: ma = a / sw; m = c + ma; v = b / sw - ma*ma; sigma = sqrt(max(v, 0));
 *                                       L = max(L, m - kappa_low sigma); U = min(U, m + kappa_high sigma); c = m
 * A pixel no entry participates in gives out = 0, counts = 0, kept_weight = 0. The centre is a pass of its own (T + 2
 * folds in all): the clipped combine's starting centre, the plain mean, counts border samples and un-normalised frames.
 * With all weights 1 the T + 1 passes are the clipped combine's formulas; only the centre differs (a / sw against
 * sum * (float)(1.0 / N)), so bit equality with stk_clip_stack is not promised.
 * Quantile (quantile = q as in stk_quantile_params): with N_p the number of participating entries of the pixel and u_(k)
 * the k-th smallest participating normalised sample of the pixel and channel (k from 0):
 *   N_p == 0:  out = 0
 *   else:      vi = (float)(N_p - 1) * q;  j = floor(vi);  g = vi - j;  lo = u_(j);  hi = u_(min(j + 1, N_p - 1));  d = hi - lo
 *              out = g == 0 ? lo : (g >= 0.5 ? hi - d * (1 - g) : lo + d * g);   any participating NaN -> NaN
 *   counts (optional, width * height int32, one per PIXEL) = N_p
 * w enters only through w_i > 0: an order statistic of the participating samples, not a weighted quantile. With every
 * entry participating, g = 1 and o = 0 this is stk_quantile_stack bit for bit on a finite stack.
 * Statuses as in the forms these extend. stk_timing.finalize_ms of the whole-stack calls is the device time of the
 * moments pass plus the combine. A multi-device context runs these calls on its first device. */

/* stk_clip_stack with stk_weighted_stack's per_frame records and coverage flag. counts_or_null: width * height *
 * channels int32; kept_weight_or_null: width * height * channels f32; both in the location of `out`. */
stk_status stk_clip_stack_weighted(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                   int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                   const stk_clip_params* clip, const stk_frame_weight* per_frame, int32_t coverage,
                                   stk_image_f32* out, int32_t* counts_or_null, float* kept_weight_or_null);
/* stk_quantile_stack with the per_frame records and the coverage flag. counts_or_null: width * height int32 (N_p). */
stk_status stk_quantile_stack_weighted(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                       int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                       const stk_quantile_params* quantile, const stk_frame_weight* per_frame, int32_t coverage,
                                       stk_image_f32* out, int32_t* counts_or_null);
/* The whole-stack forms: the plain call (its stats, warps and errors), the records as stk_ecc_match_weighted /
 * stk_keypoint_match_weighted make them (weight: normalize, coverage, stat_step; weights_or_null: n weights by frame
 * index, NULL = all 1; the moments pass and the estimator when normalize != 0), then the combine above. applied_or_null:
 * n records by frame index, what the combine used; a dropped frame has weight 0 and gains 1, offsets 0. */
stk_status stk_ecc_match_clipped_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                          float scale_down_width, const stk_clip_params* clip, const stk_weight_params* weight,
                                          const float* weights_or_null, stk_image_f32* out, int32_t* counts_or_null,
                                          float* kept_weight_or_null, stk_frame_weight* applied_or_null,
                                          stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_clipped_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                               float scale_down_width, const stk_clip_params* clip,
                                               const stk_weight_params* weight, const float* weights_or_null, stk_image_f32* out,
                                               int32_t* dropped, int32_t* counts_or_null, float* kept_weight_or_null,
                                               stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null);
stk_status stk_ecc_match_quantile_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                           float scale_down_width, const stk_quantile_params* quantile,
                                           const stk_weight_params* weight, const float* weights_or_null, stk_image_f32* out,
                                           int32_t* counts_or_null, stk_frame_weight* applied_or_null,
                                           stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_quantile_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                                float scale_down_width, const stk_quantile_params* quantile,
                                                const stk_weight_params* weight, const float* weights_or_null, stk_image_f32* out,
                                                int32_t* dropped, int32_t* counts_or_null, stk_frame_weight* applied_or_null,
                                                stk_frame_stats* stats_or_null);

/* ---- median / MAD sigma clipping: an EXTENSION beyond the reference -------------------------------------------
 * Rejection about a robust centre and scale. The clipped combine above judges the samples by their own mean and standard
 * deviation, and no sample of N lies further than sqrt(N - 1) population standard deviations from their mean (Samuelson's
 * inequality): with kappa = 3 it rejects nothing at N <= 10, with kappa = 2.5 nothing at N <= 7, whatever the data. Here
 * the centre is the median and the scale 1.4826 times the median absolute deviation (MAD), which one outlier among a
 * handful of frames does not move; the result is still the mean of the kept samples, so the noise reduction of stacking
 * stays (a median has about 1.25 times the noise of a mean at large N).
 * Samples. The clipped combine's: per pixel and channel s_1 .. s_N are the warped, converted frames in fold order (frame 0
 * through the identity, then the kept frames in ascending index; in stk_robust_clip_stack the included frames in index
 * order under the caller's matrices) with the fold's own warp, border mode and value, alpha, warp_subpixel_bits and
 * warp_interpolation. All arithmetic is f32, each operation rounded on its own, no contraction, `/` correctly rounded; max
 * and min are C's fmaxf / fminf (a NaN operand gives the other one). med(K) is the quantile combine's formula at
 * quantile = 0.5 over the multiset K of k samples: vi = (float)(k - 1) * 0.5f; j = floor(vi); g = vi - j; lo = the j-th
 * smallest (from 0), hi = the (min(j + 1, k - 1))-th; d = hi - lo; med = g == 0 ? lo : hi - d * (1 - g).
 *   K = all N samples; k = N; L = -inf; U = +inf; c = med(K)
 *   rounds t = 1 .. iterations:
 *       if k < 3: stop (c, L, U stay)
 *       e_i = |s_i - c| for the samples of K
 *       mad = med({e_i})
 *       sigma = max(1.4826f * mad, sigma_floor)
 *       L = max(L, c - kappa_low * sigma);  U = min(U, c + kappa_high * sigma)
 *       K = {s_i : L <= s_i && s_i <= U};  k = |K|
 *       if k > 0: c = med(K)
 *   final pass, the samples in fold order (the clipped combine's last pass, bit for bit):
 *       k = 0; a = 0;  for each s: d = s - c; if (L <= s && s <= U) { k += 1; a = a + d; }
 *       out = k > 0 ? c + a / (float)k : c;   counts (optional) = k
 * sigma_floor. The MAD is 0 whenever more than half of the samples are equal, which is common on 8-bit data (saturated or
 * flat regions, integer translations); with a scale of 0 every sample one grey level off the median would be rejected.
 * sigma_floor is the smallest scale the test uses, in the units of the samples (after alpha). Recommended: half a
 * quantisation step of the input after alpha, i.e. 0.5f / 255 for 8-bit frames under alpha = 1 / 255 (0.5f / 65535 for
 * 16-bit ones under alpha = 1 / 65535). 0 is allowed: then only samples equal to the centre survive where the MAD is 0.
 * Non-finite samples. Any NaN sample makes the output of that pixel and channel NaN, as in the quantile (c = NaN, L = -inf,
 * U = +inf; the final pass produces the NaN). One +-inf sample among finite ones is rejected and the result is finite.
 * Where the median itself is infinite (or the midpoint of a finite and an infinite sample, or of -inf and +inf, which is
 * NaN) the deviations inf - inf are NaN; a NaN deviation ranks above every number and a NaN mad gives sigma = sigma_floor:
 * the output of such a pixel and channel is NaN, and counts is the number of samples the bounds then keep.
 * N is at most 4096 (STK_NOT_IMPLEMENTED beyond). `out` must be tightly packed; counts_or_null: width * height * channels
 * int32 in the location of `out`. stk_timing.finalize_ms of these calls is the combine's device time (warp_ms etc. are
 * the plain call's). The samples go through the quantile combine's band buffer (option "quantile_band_rows"), the centre
 * and bounds through the clipped combine's planes. A multi-device context runs these calls on its first device.
 * stk_get_counter "robust_select_us": the device time of the last call's selection launches, in microseconds.
 * The participation form extends this as the normalised, coverage-aware clip extends the clipped combine: participation
 * and the normalised sample u = s * g + o are those of stk_clip_stack_weighted; centre and scale are UNWEIGHTED order
 * statistics of the participating normalised samples (w enters through w > 0 only, as in stk_quantile_stack_weighted); the
 * final pass is the weighted clip's last pass: a = a + w * d, sw = sw + w, out = k > 0 ? c + a / sw : c, counts = k,
 * kept_weight = sw. A pixel no entry participates in gives out = 0, counts = 0, kept_weight = 0. With all weights 1,
 * g = 1, o = 0 and every entry participating this is stk_robust_clip_stack bit for bit on a finite stack. */
typedef struct {
    float   kappa_low, kappa_high;  /* rejection below c - kappa_low sigma / above c + kappa_high sigma: > 0, finite */
    float   sigma_floor;            /* >= 0, finite, in the units of the samples (after alpha); 0.5f / 255 recommended for 8-bit */
    int32_t iterations;             /* rounds T of median / MAD bounds before the final pass, 1 .. 16 */
} stk_robust_clip_params;

/* ecc_match / keypoint_match with the median / MAD clip: stats, warps, `dropped` and errors are the plain call's, the
 * samples those of stk_ecc_match_clipped / stk_keypoint_match_clipped. */
stk_status stk_ecc_match_robust_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                        const stk_robust_clip_params* clip, stk_image_f32* out, int32_t* counts_or_null,
                                        stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_robust_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                             float scale_down_width, const stk_robust_clip_params* clip, stk_image_f32* out,
                                             int32_t* dropped, int32_t* counts_or_null, stk_frame_stats* stats_or_null);
/* The combine alone over caller-held warps, with the arguments of stk_clip_stack. */
stk_status stk_robust_clip_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                 int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                 const stk_robust_clip_params* clip, stk_image_f32* out, int32_t* counts_or_null);
/* The participation form, with the arguments of stk_clip_stack_weighted (coverage = 1 puts no condition on the border mode
 * or value, as there). */
stk_status stk_robust_clip_stack_weighted(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                          int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                          const stk_robust_clip_params* clip, const stk_frame_weight* per_frame, int32_t coverage,
                                          stk_image_f32* out, int32_t* counts_or_null, float* kept_weight_or_null);
/* The whole-stack participation forms, with the arguments of stk_ecc_match_clipped_weighted /
 * stk_keypoint_match_clipped_weighted; finalize_ms is the device time of the moments pass plus the combine. */
stk_status stk_ecc_match_robust_clipped_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                                 float scale_down_width, const stk_robust_clip_params* clip,
                                                 const stk_weight_params* weight, const float* weights_or_null, stk_image_f32* out,
                                                 int32_t* counts_or_null, float* kept_weight_or_null,
                                                 stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_robust_clipped_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                                      float scale_down_width, const stk_robust_clip_params* clip,
                                                      const stk_weight_params* weight, const float* weights_or_null,
                                                      stk_image_f32* out, int32_t* dropped, int32_t* counts_or_null,
                                                      float* kept_weight_or_null, stk_frame_weight* applied_or_null,
                                                      stk_frame_stats* stats_or_null);

/* ---- local normalisation: per-frame gain and offset fields on a node grid: an EXTENSION beyond the reference --------
 * The weighted combine and the participation quantile map each frame onto frame 0's level with ONE gain and offset per
 * frame and channel. A sky gradient that turns over a session, thin cloud over one corner or vignetting under a dither
 * differ from frame 0 by a smooth field, not by a constant. This section estimates, per frame, a gain and an offset on
 * the node grid of the mesh section and folds through their bilinear interpolation, as the mesh fold does for geometry.
 * w x h is the destination size (frame 0's), cn the channel count. Samples s_i,c, fold order, alpha, warp, border
 * handling, warp_subpixel_bits and the coverage weight kappa_i are the weighted combine's.
 * Grids. Nodes are those of stk_mesh_grid(w, h, step): gw x gh, node (j, k) at destination pixel (k step, j step), step a
 *   power of two in 8 .. 256. Cells: cw = (w + step - 1) / step by ch likewise; cell (J, K) covers x in [K step,
 *   min((K + 1) step, w)) and y likewise.
 * Cell moments. For entry i >= 1, cell (J, K) and channel c: the destination pixels of the cell with x % stat_step == 0,
 *   y % stat_step == 0 and kappa_i == 1.0f, kappa_i being the BORDER_CONSTANT one whatever the fold's border mode, exactly
 *   as in stk_overlap_moments. X = (double)s_i,c, Y = (double)s_0,c; the samples are always the LINEAR fold's, also under
 *   STK_INTER_CUBIC (these are statistics, not an image). The six f64 values per channel are n, sum X, sum Y, sum X^2,
 *   sum Y^2, sum XY; products are formed in f64, so every term is exact. The order of the additions is fixed by the
 *   geometry, step and stat_step alone (one wave per cell and entry: a lane's pixels in row-major order, then a
 *   xor-shuffle tree; no atomics): the same bits on every call and under every option. A cell without a stepped pixel has
 *   n = 0.
 * Node moments of node (j, k): the sum of the existing cells among (j-1, k-1), (j-1, k), (j, k-1), (j, k), in that order,
 *   in f64: the 2 step square around the node; windows overlap by half.
 * Global moments of a frame: the sum of all its cells in row-major order, in f64. Not promised to be bit-equal to
 *   stk_overlap_moments (the order differs); n is equal.
 * Estimator, on the host in f64, results rounded to f32: per node and channel the weighted combine's formulas for
 *   normalize 0 .. 3 on the node moments. A (node, channel) is invalid if n < min_count, if the formula falls back (a
 *   denominator <= 0 or a non-finite result), or if the gain lies outside [0.25, 4].
 * Fill. `fill` Jacobi passes per channel on the pair (g_c, o_c): the arithmetic of the mesh section's "Fill" (k = [1 2 1]^T
 *   [1 2 1], in-grid neighbours in row-major order, f32, den = den + k, num = num + k value, value = num / den) with the
 *   channel's validity as m. A (node, channel) still invalid afterwards takes the frame's global (g_c, o_c), the same
 *   formulas on the global moments (no count or range test); where that falls back it is (1, 0). The global record
 *   (stk_frame_weight: gains, offsets, weight 1; bit c of flags set iff the global formula of channel c fell back) is
 *   returned beside the plane.
 * Plane: gh x gw x 2 cn f32, tightly packed, per node g_0 .. g_{cn-1}, o_0 .. o_{cn-1}. Planes are small and always HOST
 *   memory, whatever the frames' location. Frame 0 and excluded frames have no plane.
 * Locally normalised fold. Destination pixel (x, y): k = x / step, j = y / step, k1 = min(k + 1, gw - 1), j1 = min(j + 1,
 *   gh - 1); u = (float)(x - k step) * (1.0f / step), v likewise (both exact). For entry i with plane P and each of the 2 cn
 *   components q, the mesh fold's chain: t0 = fma(u, P[j][k1][q] - P[j][k][q], P[j][k][q]), t1 the same on row j1, value =
 *   fma(v, t1 - t0, t0): G_c = value of q = c, O_c = value of q = cn + c. An entry with a NULL plane uses its record's gain
 *   and offset as constants. Then, as in the weighted combine, v_c = s_i,c * G_c + O_c * kappa_i; num_c = num_c + w_i * v_c;
 *   den = den + w_i * kappa_i; out_c = den > 0 ? num_c / den : 0. For an entry with a plane w_i comes from the record and
 *   the record's gain and offset are ignored. NULL records mean unit records. coverage as in stk_weighted_stack.
 * Locally normalised quantile: the participation quantile of the section above with u = s * G_c + O_c.
 * Consequences. With every plane NULL, or every plane constant and equal to its record, the results are
 *   stk_weighted_stack's and stk_quantile_stack_weighted's bit for bit (fma(u, 0, g) = g). warp_subpixel_bits = 5 and
 *   STK_INTER_CUBIC are served (generic kernels, as the local-weighted fold). A multi-device context runs these calls on
 *   its first device. Plane values are expected finite and are not checked. */
typedef struct {
    int32_t step;        /* node spacing: 8 .. 256, a power of two */
    int32_t stat_step;   /* 1 .. 64; 0 = 4 */
    int32_t normalize;   /* 0 NONE .. 3 LINEAR, as stk_weight_params */
    int32_t coverage;    /* as stk_weight_params */
    int32_t min_count;   /* pixels a node's window needs: >= 1; 0 = 16 */
    int32_t fill;        /* 0 .. 16 */
    int32_t reserved[2]; /* 0 */
} stk_local_norm_params;

/* The cell moments alone of every included frame i >= 1 against frame 0, which must be included. Arguments as
 * stk_overlap_moments; step: the node spacing; stat_step: 1 .. 64. moments: n x (ch cw) x channels x 6 doubles on the host,
 * frame index order, cells in row-major order; frame 0 and excluded frames: zeros. stk_timing.finalize_ms is the pass. */
stk_status stk_local_moments(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                             int32_t is_affine, int32_t border_mode, const double* border_value, double alpha, int32_t step,
                             int32_t stat_step, double* moments);
/* Estimator and fill for one frame: pure host code, no context (a bad argument is STK_INVALID_PARAMS without a message).
 * cell_moments_of_one_frame: (ch cw) x channels x 6 doubles; plane: gh x gw x 2 channels f32; global_or_null: the global
 * record; valid_or_null: gh x gw int32, bit c = (node, channel c) was valid BEFORE the fill. params->coverage is not read. */
stk_status stk_local_norm_estimate(int32_t width, int32_t height, int32_t channels, const stk_local_norm_params* params,
                                   const double* cell_moments_of_one_frame, float* plane, stk_frame_weight* global_or_null,
                                   int32_t* valid_or_null);
/* The locally normalised mean alone over caller-held warps: stk_weighted_stack's arguments with per_frame_or_null, then
 * norm_or_null: n host planes by frame index for the grid of `step` (an entry, or the array, may be NULL: no plane). */
stk_status stk_local_norm_stack(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                const stk_frame_weight* per_frame_or_null, const float* const* norm_or_null, int32_t step,
                                int32_t coverage, stk_image_f32* out, float* den_or_null);
/* The locally normalised quantile alone: stk_quantile_stack_weighted's arguments with per_frame_or_null, then the planes. */
stk_status stk_quantile_stack_local_norm(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                         int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                         const stk_quantile_params* quantile, const stk_frame_weight* per_frame_or_null,
                                         const float* const* norm_or_null, int32_t step, int32_t coverage, stk_image_f32* out,
                                         int32_t* counts_or_null);
/* The whole-stack forms: the plain call (its stats, warps, `dropped` and errors), the cell moments on the stats' warps over
 * the resident frames, the estimator, then the mean (quantile_or_null == NULL) or the quantile through the planes; by
 * definition the result of those parts, bit for bit. The records are units with weights_or_null's weights (NULL = all 1).
 * den_or_null (w x h f32, the mean only) and counts_or_null (w x h int32, the quantile only) are in the location of `out`;
 * the one that does not belong to the chosen combine must be NULL (STK_INVALID_PARAMS). norm_out_or_null: n host planes by
 * frame index, NULL entries skipped; frame 0's and a dropped frame's are not written. applied_or_null: n records by frame
 * index: the frame's global record with its weight; frame 0: a unit record; a dropped frame: weight 0. The fold runs under
 * the plain call's border (coverage = 1 needs BORDER_CONSTANT 0). finalize_ms is the moments pass plus the combine. */
stk_status stk_ecc_match_local_normalized(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                          float scale_down_width, const stk_local_norm_params* norm,
                                          const stk_quantile_params* quantile_or_null, const float* weights_or_null,
                                          stk_image_f32* out, float* den_or_null, int32_t* counts_or_null,
                                          float* const* norm_out_or_null, stk_frame_weight* applied_or_null,
                                          stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_local_normalized(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                               float scale_down_width, const stk_local_norm_params* norm,
                                               const stk_quantile_params* quantile_or_null, const float* weights_or_null,
                                               stk_image_f32* out, int32_t* dropped, float* den_or_null,
                                               int32_t* counts_or_null, float* const* norm_out_or_null,
                                               stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null);

/* Local normalisation, continued: the two clip combines through the planes.
 * Locally normalised clip: stk_clip_stack_weighted's definition, word for word, with one change: the normalised sample is
 *   u = s * G_c + O_c, (G_c, O_c) the entry's plane at the destination pixel by the chain "Locally normalised fold" states
 *   (k, j, k1, j1, u, v, then t0, t1, value by fma). An entry with a NULL plane uses its record's gain and offset as
 *   constants. For an entry with a plane w comes from the record and the record's gain and offset are ignored. NULL
 *   records mean unit records. Unchanged from stk_clip_stack_weighted: participation (w > 0 and, with coverage = 1,
 *   kappa == 1.0f), the centre pass, passes 1 .. T + 1, the k >= 3 rule, out, counts, kept_weight, and the pixel that no
 *   entry participates in.
 * Locally normalised median / MAD clip: the participation form of stk_robust_clip_stack_weighted with the same u: centre
 *   and scale are unweighted order statistics of the participating u; the final pass is the locally normalised clip's
 *   last pass.
 * Consequences. With every plane NULL, or every plane constant and equal to its record, the results are
 *   stk_clip_stack_weighted's and stk_robust_clip_stack_weighted's bit for bit, also where those run the u8 BGR fast
 *   kernels (the new calls run them too: BGR u8 under BORDER_CONSTANT with exact coordinates). warp_subpixel_bits = 5 and
 *   STK_INTER_CUBIC are served. A multi-device context runs these calls on its first device. Plane values are expected
 *   finite and are not checked.
 * Checks: those of stk_clip_stack_weighted / stk_robust_clip_stack_weighted (coverage = 1 puts no condition on the border;
 *   the median / MAD form keeps N <= 4096: STK_NOT_IMPLEMENTED beyond), then stk_local_norm_stack's step check.
 * The caller-held forms: stk_clip_stack_weighted's / stk_robust_clip_stack_weighted's arguments with per_frame_or_null, then
 * norm_or_null and step as in stk_local_norm_stack. counts_or_null (w x h x cn int32) and kept_weight_or_null (w x h x cn
 * f32) are in the location of `out`. */
stk_status stk_clip_stack_local_norm(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                     int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                     const stk_clip_params* clip, const stk_frame_weight* per_frame_or_null,
                                     const float* const* norm_or_null, int32_t step, int32_t coverage, stk_image_f32* out,
                                     int32_t* counts_or_null, float* kept_weight_or_null);
stk_status stk_robust_clip_stack_local_norm(stk_ctx* ctx, const stk_frames* frames, const double* M, const int32_t* include_or_null,
                                            int32_t is_affine, int32_t border_mode, const double* border_value, double alpha,
                                            const stk_robust_clip_params* clip, const stk_frame_weight* per_frame_or_null,
                                            const float* const* norm_or_null, int32_t step, int32_t coverage, stk_image_f32* out,
                                            int32_t* counts_or_null, float* kept_weight_or_null);
/* The whole-stack forms: by definition the result of their parts, bit for bit: the plain call, stk_local_moments on its
 * warps, stk_local_norm_estimate per frame, then stk_clip_stack_local_norm (clip_or_null given) or
 * stk_robust_clip_stack_local_norm (robust_or_null given) with unit records carrying weights_or_null. Exactly one of
 * clip_or_null / robust_or_null must be non-NULL (STK_INVALID_PARAMS otherwise). norm_out_or_null, applied_or_null and
 * finalize_ms (moments plus combine) as in stk_ecc_match_local_normalized. */
stk_status stk_ecc_match_local_normalized_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params,
                                                  float scale_down_width, const stk_local_norm_params* norm,
                                                  const stk_clip_params* clip_or_null, const stk_robust_clip_params* robust_or_null,
                                                  const float* weights_or_null, stk_image_f32* out, int32_t* counts_or_null,
                                                  float* kept_weight_or_null, float* const* norm_out_or_null,
                                                  stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null);
stk_status stk_keypoint_match_local_normalized_clipped(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                                       float scale_down_width, const stk_local_norm_params* norm,
                                                       const stk_clip_params* clip_or_null,
                                                       const stk_robust_clip_params* robust_or_null, const float* weights_or_null,
                                                       stk_image_f32* out, int32_t* dropped, int32_t* counts_or_null,
                                                       float* kept_weight_or_null, float* const* norm_out_or_null,
                                                       stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null);

/* ---- star registration: detect stars, match triangles, align the stack: an EXTENSION beyond the reference ----------
 * A third aligner beside stk_ecc_match and stk_keypoint_match, for 8-bit star fields (1, 3 or 4 channels; the whole-stack
 * forms 3 or 4): BRIEF descriptors of point sources on a black sky are not distinctive, and ECC starts at the identity
 * with a capture range of a few pixels. Stars are found as background-subtracted centroids, matched by triangle
 * similarity (rotation-, scale- and flip-free up to the tolerance), fitted with findHomography. Depth 16 / 32:
 * STK_NOT_IMPLEMENTED.
 * Detection, all in integers (kernels_star.hip). g: the 8-bit grey (stk_grey's; one-channel frames as they are),
 * r = radius, T: the 64 x 64 tile (origin at multiples of 64) that holds the pixel in question.
 *   1. Tile statistics. n = the tile's pixels inside the frame, k = (n + 1) / 2; med_T = the k-th smallest g of the tile,
 *      mad_T = the k-th smallest |g - med_T|; d_T = max((int)ceilf(ks * (float)mad_T), min_contrast) with
 *      ks = (float)(kappa * 1.4826) (the product in double); thr_T = med_T + d_T.
 *   2. Pixel p = (px, py) of tile T is a peak when r <= px < w - r and r <= py < h - r (the whole window inside the frame,
 *      no reflection); g(p) >= thr_T; for every q != p of the (2r + 1)^2 window g(q) < g(p) if q precedes p in raster
 *      order and g(q) <= g(p) otherwise (a plateau yields its raster-first pixel); and
 *      npix = #{q in the window: g(q) >= thr_T} >= min_pixels (a hot pixel has npix 1).
 *   3. Moments over the window with v(q) = max(g(q) - med_T, 0): S = sum v, Sx = sum v (qx - px), Sy = sum v (qy - py), int32.
 *   4. Per tile the peaks are ranked by the key (S descending, py ascending, px ascending); the first STK_STAR_TILE_CAP are
 *      kept. Per frame the tiles' peaks are merged, sorted by the same key and cut to max_stars. n_peaks counts every peak
 *      of the frame, those beyond a tile's cap and beyond max_stars included.
 *   5. x = (float)((double)px + (double)Sx / (double)S), y likewise, flux = (float)S; peak = g(p).
 *   The same bits on every call: no float arithmetic but the one multiply and ceil, no ordering races.
 * Matching (star_match.cpp: host only, f64 on the f32 coordinates; a distance is sqrt(dx*dx + dy*dy)).
 *   1. Triangles of a list: P = its first min(match_stars, count) stars. For each star i its `neighbours` nearest others in
 *      P (ties: lower index; fewer when P is smaller); one triangle for every pair of them with i; deduplicated by the sorted
 *      index triple and kept in that (lexicographic) order. Sides a >= b >= c, a side named by its opposite vertex, ties
 *      to the lower opposite vertex index; skipped when a <= 0 or c / a < 0.1. Descriptor (b / a, c / a); vertices listed
 *      as (opposite a, opposite b, opposite c).
 *   2. Votes: each triangle of the moving list takes the reference triangle of smallest squared descriptor distance (ties:
 *      lower index), accepted when that is <= tri_tolerance^2; an accepted pair adds one vote to each of its three vertex
 *      correspondences.
 *   3. Pairs: moving star i pairs with j = argmax of row i (lowest j on ties) when votes >= min_votes and i is the argmax
 *      of column j (lowest i on ties); in ascending i.
 *   4. Fit: with >= 4 pairs, findHomography(moving -> frame 0, method, ransac_reproj_threshold) as stk_find_homography.
 *   5. Refine (refine = 1): every star of the frame is projected by H; it pairs with the nearest reference star (all of
 *      frame 0's stars) at distance <= ransac_reproj_threshold (ties: lower index) when it is in turn the nearest projected
 *      star of that reference star (ties: lower index); with >= 4 such pairs a second fit, kept when found with at least
 *      the first fit's inliers.
 *   6. A frame is DROPPED (status 1, never an error) with fewer than min_stars stars (frame 0 below min_stars drops every
 *      frame), fewer than 4 pairs, no model, or fewer than min_inliers inliers. Every moving frame dropped: the call fails
 *      as stk_keypoint_match does (STK_INVALID_PARAMS), the stats filled all the same.
 *   Stats: n_keypoints = the stars kept, n_matches = the pairs of the last fit run, n_inliers and warp = the kept fit's
 *   (frame 0: its stars, the identity).
 * Checks: radius 2 .. 7, kappa finite and >= 0, min_contrast 1 .. 255, min_pixels 1 .. (2r+1)^2, max_stars 4 .. 1024,
 *   match_stars 4 .. 200, neighbours 2 .. 8, tri_tolerance finite and > 0, min_votes >= 1, refine 0 / 1, min_stars >= 4,
 *   min_inliers >= 4, method 0 / STK_METHOD_LMEDS / STK_METHOD_RANSAC (RHO, USAC: STK_NOT_IMPLEMENTED), threshold finite and
 *   > 0, border_mode as stk_keypoint_match: STK_INVALID_PARAMS otherwise. The stack forms need n >= 2 (STK_NOT_ENOUGH_FILES).
 * A multi-device context runs these calls on its first device. 16-bit and f32 frames: the *_deep calls of the next section.
 * Follow-ups, not here: a similarity or affine model for fields of fewer than about 12 stars, whole-stack star_match_* forms
 * of each combine, a shard form, a files form, an interpolated (non-piecewise) background, a device-side matcher. */
enum { STK_STAR_TILE_CAP = 32 };
typedef struct {
    float   x, y, flux;
    int32_t px, py, peak, npix, reserved;
} stk_star;
typedef struct {
    int32_t radius;                 /* 2 .. 7, default 4 */
    float   kappa;                  /* default 4 */
    int32_t min_contrast;           /* >= 1, default 8 */
    int32_t min_pixels;             /* 1 .. (2r+1)^2, default 3 */
    int32_t max_stars;              /* 4 .. 1024, default 200 */
    int32_t match_stars;            /* brightest m used for triangles, 4 .. 200, default 50 */
    int32_t neighbours;             /* 2 .. 8, default 5 */
    double  tri_tolerance;          /* default 0.01 */
    int32_t min_votes;              /* default 2 */
    int32_t refine;                 /* 1 (default): guided re-match of all stars under the first H */
    int32_t min_stars;              /* a frame with fewer detected stars is dropped, >= 4, default 6 */
    int32_t min_inliers;            /* >= 4, default 7: a homography fits ANY four pairs exactly, so 4 rejects nothing; a frame
                                       of another star field reached 4 - 6 inliers in 80 seeded trials, a true 12-star field 13 */
    int32_t method;                 /* STK_METHOD_*, as stk_keypoint_params */
    double  ransac_reproj_threshold;   /* default 2.0 */
    int32_t border_mode;            /* STK_BORDER_* (stk_star_match's fold) */
    double  border_value[4];
} stk_star_params;

/* The stars of every frame, brightest first: stars holds n x max_stars entries (frame i from i * max_stars; entries from
 * n_stars[i] on are zeroed), n_stars n counts, n_peaks_or_null n counts before truncation. Host or device frames, padded
 * rows, 1 / 3 / 4 channels. All outputs are host memory. */
stk_status stk_star_detect(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, stk_star* stars,
                           int32_t* n_stars, int32_t* n_peaks_or_null);
/* Steps 1 - 3 on two lists; no context, no GPU. pairs: up to match_stars x 2 int32 (moving index, reference index). */
stk_status stk_star_match_lists(const stk_star* moving, int32_t n_moving, const stk_star* ref, int32_t n_ref,
                                const stk_star_params* params, int32_t* pairs, int32_t* n_pairs);
/* Detection and steps 1 - 6, no fold: stats (n entries) feed any *_stack combine as M with include[i] = (status == 0) and
 * is_affine = 0. dropped: the number of moving frames dropped. */
stk_status stk_star_align(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, int32_t* dropped,
                          stk_frame_stats* stats);
/* stk_star_align, then the plain mean over frame 0 and the kept frames: by definition stk_warp_accumulate of those frames
 * under the stats' warps in frame order (alpha 1 / 255, the params' border, never affine), then
 * stk_finalize_mean(n - dropped), bit for bit. */
stk_status stk_star_match(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params, stk_image_f32* out,
                          int32_t* dropped, stk_frame_stats* stats_or_null);

/* ---- star registration on 8-bit, 16-bit and f32 frames: an EXTENSION beyond the reference ---------------------------------
 * The three calls above on the data the front half of a pipeline produces (stk_calibrate and stk_demosaic return u16 or f32):
 * a star 200 - 300 counts over a 16-bit sky of sigma 40 is less than one grey level of the (g + 128) / 257 reduction. Detection
 * runs on a 16-bit integer KEY K(p) in 0 .. 65535 (kernels_star_deep.hip); stk_star_params, stk_star, stk_star_match_lists and
 * the matching, fits, refine and drop rules are those of the section above, to the letter.
 * The key. Depth 8: K = the 8-bit grey above. Depth 16: K = stk_grey's 16-bit grey,
 *   (b * 1868 + g * 9617 + r * 4899 + 2^13) >> 14. Depth 32: gf = b * 0.114f + g * 0.587f + r * 0.299f (every product and
 *   sum rounded to f32, no contraction: stk_grey's), K = (int)fminf(fmaxf(rintf(gf * f32_scale), 0.0f), 65535.0f); a NaN
 *   gives 0, +inf 65535, -inf 0. One-channel frames: the value itself in place of the grey. The fourth channel is not read.
 * Detection: steps 1 - 5 of stk_star_params with K in place of g, and these changes only:
 *   - med_T and mad_T are the exact k-th smallest K and the exact k-th smallest |K - med_T| of the tile's pixels inside the
 *     frame (a two-level radix selection on integer histograms: no estimate, no dependence on scheduling);
 *   - d_T = max((int)fminf(ceilf(ks * (float)mad_T), 65536.0f), min_contrast);
 *   - min_contrast is in key units and is checked as 1 .. 65535 by these entry points; every other check is the 8-bit calls';
 *   - S, Sx, Sy stay int32: S <= 225 * 65535 = 14 745 375, |Sx|, |Sy| <= 840 * 65535 = 55 049 400 (840 = the sum of |dx|
 *     over the 15 x 15 window).
 * Consequences. On 8-bit frames every output equals the 8-bit call's, bit for bit (stk_star_match_deep with alpha 1 / 255
 *   equals stk_star_match). A one-channel u16 frame holding values <= 255 gives the stars of the u8 frame with the same
 *   values. An f32 frame holding a u16 frame's values gives, under f32_scale = 1, the u16 frame's stars.
 * Refusals: a null `deep`, reserved != 0, f32_scale not finite or <= 0 at depth 32, a non-finite alpha: STK_INVALID_PARAMS;
 *   everything else as the 8-bit calls refuse. A multi-device context runs these calls on its first device. */
typedef struct {
    float   f32_scale;   /* depth 32 only: key = rint(grey * f32_scale), clamped; finite, > 0. Ignored at depth 8 / 16 */
    int32_t reserved;    /* 0 */
} stk_star_deep_params;

/* stk_star_detect on the key: the same outputs. */
stk_status stk_star_detect_deep(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params,
                                const stk_star_deep_params* deep, stk_star* stars, int32_t* n_stars, int32_t* n_peaks_or_null);
/* stk_star_align on the key: the stats feed any *_stack combine of the frames' own depth. */
stk_status stk_star_align_deep(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params,
                               const stk_star_deep_params* deep, int32_t* dropped, stk_frame_stats* stats);
/* stk_star_align_deep, then the plain mean over frame 0 and the kept frames: by definition, and bit for bit,
 * stk_warp_accumulate of those frames under the stats' warps in frame order (at the frames' depth, the given alpha, the
 * params' border, never affine), then stk_finalize_mean(n - dropped). */
stk_status stk_star_match_deep(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params,
                               const stk_star_deep_params* deep, double alpha, stk_image_f32* out, int32_t* dropped,
                               stk_frame_stats* stats_or_null);

/* ---- star shapes per frame: FWHM, eccentricity, SNR, quality weights: an EXTENSION beyond the reference -------------------
 * A deep-sky stacker grades a star-field frame by the size and roundness of its stars: seeing, focus drift, wind and tracking
 * errors show there and nowhere else (stk_stack_sharpness sums gradients of 8-bit greys, which a star field's noise and star
 * count dominate). stk_star_measure measures every detected star's shape in exact integers on the device
 * (kernels_star_measure.hip); host code (f64, no context, no GPU) turns the measurements into per-frame quality, into scores
 * that stk_rank_frames takes unchanged and into weights that every *_stack combine takes unchanged.
 *
 * 1. The measurement. Input: the frames and the star lists stk_star_detect / stk_star_detect_deep return; only px and py are
 *    read. K is the 16-bit key of stk_star_deep_params (f32_scale at depth 32), to the letter. Per star p = (px, py), with
 *    dx = qx - px, dy = qy - py, R = radius, Ri = ring_inner, Ro = ring_outer; everything is integer except the one multiply
 *    and ceilf, which are detection's:
 *    0. px - R < 0, py - R < 0, px + R > w - 1 or py + R > h - 1 (coordinates outside the frame included): flags bit 0 and
 *       every other field 0. Decided on the host: such a star never reaches the device; the kernel guards it as well.
 *    1. Ring: the pixels q inside the frame with Ri^2 <= dx^2 + dy^2 <= Ro^2 (a ring pixel outside the frame forms no address
 *       and does not count). n_ring = their number, k = (n_ring + 1) / 2, bg = the exact k-th smallest K of the ring, mad =
 *       the exact k-th smallest |K - bg| (n_ring = 0, possible only on frames narrower than the ring: bg = mad = 0).
 *    2. thr = max((int)fminf(ceilf(ks * (float)mad), 65536.0f), min_contrast), ks = (float)((double)kappa * 1.4826).
 *    3. Aperture: dx^2 + dy^2 <= R^2; v(q) = K(q) - bg if that is >= thr, else 0. npix = #{v > 0}, peak = max K over the
 *       aperture, S = sum v, Sx = sum v dx, Sy = sum v dy, Sxx = sum v dx^2, Syy = sum v dy^2, Sxy = sum v dx dy, all int64
 *       (Sxx reaches 65535 x 144 x 441 > 2^31).
 *    4. flags bit 1: saturation > 0 and peak >= saturation. flags bit 2: npix < min_pixels or S == 0.
 *    No result depends on scheduling: the selection is a two-level radix selection on integer histograms, the sums are
 *    integer trees. Checks: radius 2 .. 12, ring_inner radius + 1 .. 15, ring_outer ring_inner .. 16, kappa finite and >= 0,
 *    min_contrast 1 .. 65535, min_pixels >= 1, saturation 0 (off) or 1 .. 65535, reserved 0: STK_INVALID_PARAMS otherwise.
 *
 * 2. Derived values, stk_star_shape_derive (host, f64): for a shape with flags == 0, each operation rounded on its own, only
 *    + - x / and sqrt:
 *      mx = Sx/S;  my = Sy/S;  x = px + mx;  y = py + my
 *      cxx = Sxx/S - mx mx;  cyy = Syy/S - my my;  cxy = Sxy/S - mx my
 *      tr = cxx + cyy;  df = sqrt((cxx - cyy)(cxx - cyy) + 4 (cxy cxy));  l1 = (tr + df)/2;  l2 = (tr - df)/2
 *      not (l2 > 0): flags bit 3, fwhm = ecc = snr = 0 (x, y and the moments stay)
 *      fwhm = 2.3548200450309493 sqrt(tr/2);  ecc = sqrt(max(1 - l2/l1, 0))
 *      snr  = S / (max(1.4826 mad, 0.5) sqrt((double)npix))
 *    A shape with flags != 0 gets zeros in every double. These are ISOPHOTAL moments, as SExtractor's are: sums over the
 *    pixels above thr. The FWHM of a Gaussian comes out a few per cent low, because the threshold cuts the wings; noise gives
 *    round stars an ecc floor of 0.2 - 0.35. The values compare frames with each other; they do not fit PSFs.
 *
 * 3. Frame quality, scores, weights (host, no context).
 *    stk_star_frame_quality: over frame i's shapes with flags == 0 (m of them; shapes holds n x max_stars entries, frame i
 *      from i * max_stars, n_stars[i] of them filled), each of fwhm, ecc, snr, bg and noise (= 1.4826 mad) is the lower
 *      median, the ((m + 1) / 2)-th smallest, each taken on its own. n_stars and n_measured = m are filled; m = 0: all 0.
 *    stk_star_quality_scores: scores[i] = {m ? 1 / fwhm : 0, m ? 1 - ecc : 0, snr, (double)m}, higher is better; the columns
 *      are STK_STAR_SCORE_*. stk_rank_frames orders, keeps and weights on them as on sharpness scores, select->metric naming
 *      the column: a star stack is ranked at any depth.
 *    stk_star_quality_weights: frame i PASSES when it is included (include_or_null), n_measured >= min_measured and
 *      (fwhm_max == 0 or fwhm <= fwhm_max) and (ecc_max == 0 or ecc <= ecc_max). Frame `reference` (-1 = none) passes whatever
 *      the limits say when it is included; reference >= n, < -1, not included or with n_measured == 0: STK_INVALID_PARAMS.
 *      Over the passing frames F = min fwhm, E = max (1 - ecc), Z = max snr. w = u_i (weights_or_null[i], or 1), then
 *      w = w (F / fwhm_i) fwhm_power times, w = w ((1 - ecc_i) / E) ecc_power times, w = w (snr_i / Z) snr_power times; a
 *      factor whose denominator is 0 is 1. All in f64, in that order; weights_out[i] = (float)w. A failing frame gets weight
 *      0 and include_out 0; rejected counts the included frames that failed. No passing frame, a non-finite or negative
 *      input (fwhm, ecc, snr, u_i), limits not finite or < 0, min_measured < 1, a power outside 0 .. 4, reserved != 0, n < 1
 *      or a null quality, params or weights_out: STK_INVALID_PARAMS. include_out and rejected may be null.
 *
 * 4. stk_star_match_quality_weighted. By definition, and bit for bit, it equals its parts: (1) stk_star_align_deep;
 *    (2) stk_star_detect_deep + stk_star_measure on every frame; (3) stk_star_frame_quality; (4) stk_star_quality_weights with
 *    include = (status == 0), reference 0 and the caller's weights_or_null as u; (5) stk_weighted_stack of the frames that
 *    passed (include_out) under the stats' warps with records (gain 1, offset 0, weight w), the params' border, is_affine 0
 *    and the given alpha and coverage. The refusals are the parts'; stk_star_align_deep's "every frame dropped" fails the
 *    call behind the filled stats. The frames are not uploaded twice and detection runs once. dropped: the alignment's;
 *    rejected: step 4's. A multi-device context uses its first device, like the other star calls. */
typedef struct {
    int32_t radius;                 /* aperture R, 2 .. 12, default 7 */
    int32_t ring_inner;             /* Ri, R + 1 .. 15, default 10 */
    int32_t ring_outer;             /* Ro, Ri .. 16, default 14 */
    float   kappa;                  /* finite, >= 0, default 3 */
    int32_t min_contrast;           /* 1 .. 65535, key units, default 1 */
    int32_t min_pixels;             /* >= 1, default 5 */
    int32_t saturation;             /* 0 = off, else 1 .. 65535, default 0 */
    int32_t reserved;               /* 0 */
} stk_star_measure_params;
typedef struct {
    int64_t S, Sx, Sy, Sxx, Syy, Sxy;
    int32_t px, py, bg, mad, thr, npix, peak, n_ring;
    int32_t flags;                  /* bit 0: aperture not inside the frame; bit 1: saturated; bit 2: npix < min_pixels or
                                       S == 0; bit 3 (stk_star_shape_derive): no positive minor axis */
    int32_t reserved;
    double  x, y, cxx, cyy, cxy, fwhm, ecc, snr;
} stk_star_shape;
typedef struct {
    double  fwhm, ecc, snr, bg, noise;   /* lower medians over the frame's shapes with flags == 0 */
    int32_t n_stars, n_measured;
} stk_star_quality;
typedef struct {
    double  fwhm_max;               /* 0 = off */
    double  ecc_max;                /* 0 = off */
    int32_t min_measured;           /* >= 1, default 5 */
    int32_t fwhm_power;             /* 0 .. 4, default 2 */
    int32_t ecc_power;              /* 0 .. 4, default 0 */
    int32_t snr_power;              /* 0 .. 4, default 0 */
    int32_t reserved;               /* 0 */
} stk_star_quality_params;
enum { STK_STAR_SCORE_FWHM = 0, STK_STAR_SCORE_ROUND = 1, STK_STAR_SCORE_SNR = 2, STK_STAR_SCORE_COUNT = 3 };

/* The shapes of the stars of every frame: stars and n_stars as stk_star_detect(_deep) returned them for the same frames
 * (n x max_stars entries, max_stars 1 .. 4096; n_stars[i] 0 .. max_stars); shapes: n x max_stars, entries from n_stars[i] on
 * zeroed; the derived values are filled (stk_star_shape_derive). Frames of depth 8, 16 or 32, 1 / 3 / 4 channels, host or
 * device memory, padded and misaligned rows; host frames and large stacks go through the context's workspaces as in
 * stk_star_detect_deep. All other arguments are host memory. deep: as in stk_star_detect_deep. stk_timing.prep_ms is the
 * device time of the measure launches. A multi-device context uses its first device. */
stk_status stk_star_measure(stk_ctx* ctx, const stk_frames* frames, const stk_star_deep_params* deep,
                            const stk_star_measure_params* params, const stk_star* stars, const int32_t* n_stars,
                            int32_t max_stars, stk_star_shape* shapes);
/* Section 2 on `count` shapes in place: reads the integers, writes the doubles and flags bit 3. count < 0 or a null list
 * with count > 0: STK_INVALID_PARAMS. */
stk_status stk_star_shape_derive(stk_star_shape* shapes, int32_t count);
stk_status stk_star_frame_quality(const stk_star_shape* shapes, const int32_t* n_stars, int32_t n, int32_t max_stars,
                                  stk_star_quality* out /* n */);
stk_status stk_star_quality_scores(const stk_star_quality* quality, int32_t n, double* scores /* n x 4 */);
stk_status stk_star_quality_weights(const stk_star_quality* quality, int32_t n, const stk_star_quality_params* params,
                                    int32_t reference, const int32_t* include_or_null, const float* weights_or_null,
                                    float* weights_out /* n */, int32_t* include_out_or_null /* n */, int32_t* rejected_or_null);
stk_status stk_star_match_quality_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_star_params* params,
                                           const stk_star_deep_params* deep, const stk_star_measure_params* measure,
                                           const stk_star_quality_params* quality, double alpha, int32_t coverage,
                                           const float* weights_or_null, stk_image_f32* out, float* coverage_or_null,
                                           int32_t* dropped, int32_t* rejected, stk_frame_weight* applied_or_null,
                                           stk_frame_stats* stats_or_null, stk_star_quality* quality_or_null);

/* ---- frame calibration: an EXTENSION beyond the reference ---------------------------------------------------------------
 * The front half of a stacking pipeline: bias, dark and flat masters applied to every frame of a stack, defective pixels
 * repaired from their neighbours, the defect map found from the masters, and the masters themselves built from stacks of
 * calibration frames. The frames stay where they are (host or device); a calibrated stack feeds every aligner and combine.
 * stk_calibrate. Per frame i, pixel p and channel c < min(channels, 3), f32 throughout, each operation rounded on its own,
 * no contraction, `/` correctly rounded; B, D, F are the masters' values at (p, c), s_i = dark_scale[i] (1 without):
 *   v = (float)raw
 *   bias:  v = v - B
 *   dark:  v = v - s_i * D                           (s_i * D rounded first)
 *   flat:  t = v * flat_mean[c];  v = t / fmaxf(F, flat_min)      (C's fmaxf: a NaN F gives flat_min)
 *   v = v + pedestal                                  (always, also without any master)
 * Channel 3 (alpha) is (float)raw, untouched by masters, pedestal and repair. The masters are in the frames' RAW sample units
 * (what stk_master_stack returns for raw calibration frames): no alpha scaling anywhere.
 * Defect repair, where bit c of defects[p] is set. N = the positions among the eight at offsets (+-step, 0), (0, +-step),
 * (+-step, +-step) (step = defect_step) that lie inside the frame and whose bit c is clear; a_0 <= .. <= a_(m-1) the values
 * v (as computed above: unrepaired, nothing cascades) of those m positions. The order is the total order of the bit
 * patterns: -0 below +0, every NaN above every number (a NaN enters as the canonical quiet NaN). The repaired value is
 * a_((m-1)/2) for odd m, (a_(m/2-1) + a_(m/2)) * 0.5f for even m, and v itself when m = 0.
 * Output. out_depth = STK_DEPTH_F32: v. Otherwise (out_depth = frames->depth, integer frames only): r = rintf(v) (half to
 * even, cvRound), then fminf(fmaxf(r, 0), 255 or 65535) converted; a NaN gives 0. out: n pointers in the frames' location,
 * rows out_row_stride_bytes apart (0 = tightly packed; else at least a row's bytes and a multiple of the element size).
 * Only the pixel bytes of `out` are written: row padding keeps its contents. `out` must not overlap any frame, master or
 * the map (STK_INVALID_PARAMS); in-place calibration is a follow-up, because repair reads the neighbours' raw values.
 * Every depth, 1 / 3 / 4 channels, padded and misaligned rows, any subset of the masters and the map (none: a plain
 * conversion plus pedestal). Masters and map may each be host or device memory whatever the frames' location; a master may
 * have padded rows (row_stride_bytes a multiple of 4). STK_INVALID_PARAMS: a master whose width, height or channels differ
 * from the frames'; out_depth neither frames->depth nor STK_DEPTH_F32; defect_step outside {1, 2}; with a flat, a flat_mean[c]
 * (c < min(channels, 3)) or flat_min that is not finite or not > 0; a non-finite pedestal or dark_scale; null outputs.
 * Kernel (kernels_calibrate.hip): a workgroup owns a 64 x 4 tile and a chunk of 16 frames (option "calibrate_chunk"); a
 * thread keeps its pixel's master values and map byte in registers across the chunk, so the masters are read once per chunk,
 * not once per frame. A wave in which some lane is defective takes the neighbour path (a ballot); the others never see it.
 * stk_defect_map. Per pixel p and channel c < min(channels, 3) of a master: X = its value, med = the median rule above over
 * the master's own values at ALL in-frame positions among the eight at +-step (no exclusion; m = 0: no test applies).
 *   bit c = !isfinite(X)  ||  (tests & 1 && X - med > high_abs)  ||  (tests & 2 && X < low_ratio * med)
 * (a NaN med fails both comparisons). accumulate = 1: the byte is ORed into the one already in `map`, else it replaces it.
 * map: width * height bytes, tightly packed, in map_location; the same bytes on every call. counts_or_null: 4 int64 on the
 * host, the set bits per channel of the map after the call (counts[3] = 0; integer sums, any order). The map is what
 * stk_calibrate takes as `defects`, and, as weight = (byte == 0), what stk_drizzle_stack takes through `maps`.
 * STK_INVALID_PARAMS: tests outside 1 .. 3, high_abs not finite or < 0, low_ratio outside [0, 1], step outside {1, 2},
 * accumulate outside {0, 1}.
 * stk_image_mean. Per-channel means of an f32 image (host or device): f64 sums, one partial per image row (a wave per row,
 * lanes striding the row, a fixed shuffle tree), the rows' partials added in row order; mean = sum / (width * height). The
 * order depends on the geometry alone: the same bits on every call. mean[c] = 0 for c >= channels. The source of flat_mean.
 * stk_master_stack. By definition, and bit for bit, a composition of existing calls: stk_robust_clip_stack_weighted over
 * all n frames under identity matrices (is_affine 0, STK_BORDER_CONSTANT 0, alpha = 1, coverage 0, weights 1) with
 * normalize = 0 (bias, darks): gains 1, offsets 0;
 * normalize = 2 (flats):       the GAIN records of the estimator above from stk_overlap_moments (same matrices, border and
 *                              alpha, stat_step; 0 = 4) against frame 0: every flat is brought to frame 0's level first.
 * Any other normalize: STK_INVALID_PARAMS; otherwise it refuses what those calls refuse (more than 4096 frames:
 * STK_NOT_IMPLEMENTED; "warp_interpolation" = 2 with "warp_subpixel_bits" = 5). The identity fold returns each pixel's value
 * exactly for every depth, the last row and column included, under the default options ("warp_interpolation" 1,
 * "warp_subpixel_bits" 0) and finite samples: the lerp chain is fma(0, b - a, a) = a. The one exception is f32 frames that
 * hold +-inf or NaN: b - a is then not finite and 0 * inf is NaN, so such a sample comes back NaN (an infinity included)
 * and so do its left, upper and upper-left neighbours. That case is not refused (finding it would cost a pass over the
 * stack): it is a property of the fold to know. Under the other options the masters are those options' folds.
 * A multi-device context runs these calls on its first device. Follow-ups, not here: in-place calibration; dark-scale
 * optimisation (choosing s_i by minimising the residual noise); per-frame cosmetic detection without masters; (demosaicing
 * and Bayer drizzle: the next section;) whole-stack *_match_calibrated forms (calibrate, then call any existing entry point); shard and
 * files forms; a u8 BGR dword-window fast path of the calibration kernel. */
typedef struct {
    const stk_image_f32* bias_or_null;  /* masters: width x height x frames->channels f32, in the frames' RAW sample units */
    const stk_image_f32* dark_or_null;  /* (what stk_master_stack returns); host or device; channel 3 is never read */
    const stk_image_f32* flat_or_null;
    const float*   dark_scale_or_null;  /* n per-frame factors (exposure ratio), host; NULL = all 1 */
    float          flat_mean[4];        /* the level the flat is divided by, per channel; finite and > 0 with a flat */
    float          flat_min;            /* > 0: the flat is clamped from below to this before the division */
    float          pedestal;            /* added last; finite */
    int32_t        reserved;            /* 0 */
    const uint8_t* defects_or_null;     /* width x height bytes, bit c = channel c of that pixel is defective; tightly packed */
    int32_t        defects_location;    /* STK_HOST | STK_DEVICE */
    int32_t        defect_step;         /* 1, or 2 for a colour-filter mosaic held in one channel */
    int32_t        out_depth;           /* frames->depth (rounded, saturated) or STK_DEPTH_F32 */
    int32_t        reserved2;           /* 0 */
} stk_calibration;
typedef struct {
    int32_t tests;                      /* bit 0: high test, bit 1: low test */
    float   high_abs;                   /* flagged when X - med > high_abs (dark: hot pixels); finite, >= 0 */
    float   low_ratio;                  /* flagged when X < low_ratio * med (flat: dead pixels, dust); 0 .. 1 */
    int32_t step;                       /* 1 or 2, as defect_step */
    int32_t accumulate;                 /* 1: OR into the map already there (dark first, then flat) */
    int32_t reserved;                   /* 0 */
} stk_defect_params;

stk_status stk_calibrate(stk_ctx* ctx, const stk_frames* frames, const stk_calibration* cal, void* const* out,
                         size_t out_row_stride_bytes);
stk_status stk_defect_map(stk_ctx* ctx, const stk_image_f32* master, const stk_defect_params* params, uint8_t* map,
                          int32_t map_location, int64_t* counts_or_null);
stk_status stk_image_mean(stk_ctx* ctx, const stk_image_f32* image, double* mean);
stk_status stk_master_stack(stk_ctx* ctx, const stk_frames* frames, int32_t normalize, int32_t stat_step,
                            const stk_robust_clip_params* clip, stk_image_f32* out, int32_t* counts_or_null);

/* ---- colour-filter mosaics: an EXTENSION beyond the reference ------------------------------------------------------------
 * The step between calibration and alignment for a one-shot-colour camera: a stack of single-channel Bayer mosaics in, a
 * stack of B G R frames out (stk_demosaic), and the colour mask of a pattern (stk_cfa_mask), with which the existing drizzle
 * integrates a mosaic without interpolating it. The order of a pipeline: stk_calibrate on the mosaic as ONE channel
 * (defect_step 2, preferably to f32), stk_demosaic, then any aligner or combine.
 * Site colours. A pattern is named by its 2 x 2 cell in reading order; the colour of pixel (x, y) is
 * cell[(y & 1) * 2 + (x & 1)], the cell's top-left sample being pixel (0, 0). The red sites of STK_CFA_RGGB / GRBG / GBRG /
 * BGGR have (x & 1, y & 1) = (0, 0) / (1, 0) / (0, 1) / (1, 1) = (pattern & 1, pattern >> 1); blue is diagonal to red.
 * Cropping: a window of a mosaic that starts on an odd column is the mosaic of pattern ^ 1, on an odd row of pattern ^ 2.
 * Borders. BORDER_REFLECT_101 on the MOSAIC: index -k is k, index w - 1 + k is w - 1 - k, applied again where the result
 * is still outside (a 3-wide mosaic under HA). The reflection keeps an index's parity, so a reflected sample has the colour
 * its position asks for. Width and height are at least 3 (SUPERPIXEL: 2), anything smaller is STK_INVALID_PARAMS.
 * Integer mosaics (u8, u16). Every sum below is exact in int32 and every value is a numerator S over a power of two D
 * (|S| < 2^24 for u16). Integer output: floor((S + D / 2) / D) saturated to [0, 255 or 65535]; f32 output: (float)S *
 * (1.0f / D), exact. A site's own colour is the sample itself. With c the site, N S W E at distance 1, N2 S2 W2 E2 at distance
 * 2, NW NE SW SE the diagonals:  h1 = W + E, v1 = N + S, h2 = W2 + E2, v2 = N2 + S2, x1 = v1 + h1, x2 = v2 + h2,
 * d = (NW + NE) + (SW + SE).
 *   STK_DEMOSAIC_BILINEAR   the mean of the same-colour sites of the 3 x 3 window (2 or 4 under the reflection):
 *       G at R / B: x1 / 4.  R or B at a G site: h1 / 2 or v1 / 2, the pair of that colour.  R at B, B at R: d / 4.
 *   STK_DEMOSAIC_MHC        Malvar, He, Cutler 2004, "High-quality linear interpolation for demosaicing of Bayer-patterned
 *       color images", the coefficients doubled to integers, D = 16:
 *       G at R / B:                                    8c + 4 x1 - 2 x2
 *       R or B at a G site whose ROW holds it:         10c + 8 h1 - 2 d - 2 h2 + v2
 *       R or B at a G site whose COLUMN holds it:      10c + 8 v1 - 2 d - 2 v2 + h2
 *       R at B, B at R:                                12c + 4 d - 3 x2
 *   STK_DEMOSAIC_HA         Hamilton-Adams green, colour differences for red and blue. At every R / B site
 *       tH = 2c - W2 - E2, dH = |W - E| + |tH|, gH = 2 h1 + tH, and tV, dV, gV the same vertically;
 *       G8 = 2 gH if dH < dV, 2 gV if dV < dH, else gH + gV: the green in eighths, unrounded, unclamped; D8 = 8c - G8.
 *       At a G site G8 = 8c. Green out: G8 / 8. R or B at a G site with that colour in its row: (2 G8 + D8(W) + D8(E)) / 16,
 *       in its column: (2 G8 + D8(N) + D8(S)) / 16. R at B, B at R: (4 G8 + (D8(NW) + D8(NE)) + (D8(SW) + D8(SE))) / 32.
 *       The reach on the mosaic is 3. G8 at a position outside the frame is the formula on the reflected mosaic; for
 *       integer mosaics that is G8 at the reflected position (the formulas are symmetric in W / E and N / S); for f32 the two
 *       may differ by the order of the two subtractions of tH.
 *   STK_DEMOSAIC_SUPERPIXEL the output is (width / 2) x (height / 2), one pixel per cell of the pattern: B and R are the
 *       cell's samples, G = (G1 + G2) / 2; nothing is interpolated (a last odd row or column is not read). The choice for
 *       oversampled data.
 * f32 mosaics: the same formulas in f32, one rounding per operation, no contraction; terms are added left to right as
 * written, parenthesised groups and the named sums (h1, x2, d, tH ..) first; tH = (2c - W2) - E2; products by powers of two
 * are exact, 10 * c, 12 * c and 3 * x2 round once each; the last step is a multiplication by 1 / D (none for a site's own
 * colour). The HA comparisons are plain `<`: a NaN takes the gH + gV branch. Non-finite samples spread through the stencil
 * and are not refused.
 * Which method: MHC and HA use the correlation between the colour planes and roughly halve BILINEAR's error on natural and
 * astronomical scenes (DESIGN §4.25 has the figures); where the planes are NOT correlated (synthetic scenes with independent
 * colours, narrow-band filters in front of a colour sensor) they are worse, and BILINEAR is the right choice.
 * Outputs. out: n pointers in the mosaic's location, each 3 channels (B G R interleaved, as everywhere) of out_depth =
 * the mosaic's depth or STK_DEPTH_F32 (f32 mosaics: f32 only), rows out_row_stride_bytes apart (0 = tightly packed; else at
 * least a row's bytes and a multiple of the element size). Only pixel bytes are written: row padding keeps its contents. Of
 * plane i the bytes [data[i], data[i] + row_stride_bytes * (height - 1) + width * depth / 8) are read, pixel bytes only. An
 * output that overlaps a plane is STK_INVALID_PARAMS.
 * STK_INVALID_PARAMS: a null context, mosaic, table, plane or output; n < 1; a pattern, method, depth or location outside
 * the enums; out_depth neither the depth nor STK_DEPTH_F32; a size below the minimum or above 2^30 pixels; a row stride
 * below a row or no multiple of the element size. STK_NOT_IMPLEMENTED: n > 65535, or more than 65535 tile rows (16 mosaic
 * rows each; SUPERPIXEL: 8).
 * Kernel (kernels_demosaic.hip): a workgroup of 256 threads owns a 64 x 16 tile of one frame, a thread one 2 x 2 cell on a
 * cell grid shifted by the pattern, so that every lane runs the same code on one R, two G and one B site; the tile and its
 * halo are staged in LDS with the reflection applied on the way in; HA keeps a second LDS plane of G8.
 * stk_cfa_mask. plane: width x height f32, tightly packed, host or device: 1.0f where the colour of (x, y) is `channel` (0 =
 * B, 1 = G, 2 = R), else 0.0f. It is the plane stk_drizzle_stack, stk_local_weighted_stack and stk_reject_maps take through
 * `maps`; a pixel whose map value is 0 is never read, so drizzling the mosaic as single-channel frames once per colour with
 * that colour's mask (the same plane n times) is Bayer drizzle: no interpolated sample enters the result, and den shows the
 * 1 : 2 : 1 coverage. STK_INVALID_PARAMS: a null context or plane, width or height < 1, pattern, channel or location out of
 * range.
 * A multi-device context runs these calls on its first device. Follow-ups, not here: a fused three-colour CFA drizzle kernel
 * and CFA-aware rejection maps; X-Trans and other patterns that are not 2 x 2; VNG / AHD; demosaicing inside stk_calibrate's
 * launch; whole-stack *_match_cfa forms (stk_demosaic, then any entry point); a shard form; file front-ends for raw formats;
 * wider loads and stores for 8-bit rows (a dword store path through LDS was measured and was slower: DESIGN §4.25). */
enum { STK_CFA_RGGB = 0, STK_CFA_GRBG = 1, STK_CFA_GBRG = 2, STK_CFA_BGGR = 3 };
enum { STK_DEMOSAIC_BILINEAR = 0, STK_DEMOSAIC_MHC = 1, STK_DEMOSAIC_HA = 2, STK_DEMOSAIC_SUPERPIXEL = 3 };
typedef struct {
    const void* const* data;        /* n single-channel planes */
    int32_t n, width, height;
    int32_t depth;                  /* STK_DEPTH_U8 / U16 / F32 */
    int32_t location;               /* STK_HOST | STK_DEVICE */
    int32_t pattern;                /* STK_CFA_*: the 2 x 2 cell whose top-left sample is pixel (0, 0) */
    size_t  row_stride_bytes;       /* 0 = tightly packed; else >= a row and a multiple of the element size */
} stk_mosaic;
stk_status stk_demosaic(stk_ctx* ctx, const stk_mosaic* mosaic, int32_t method, int32_t out_depth, void* const* out,
                        size_t out_row_stride_bytes);
stk_status stk_cfa_mask(stk_ctx* ctx, int32_t width, int32_t height, int32_t pattern, int32_t channel, float* plane,
                        int32_t location);

/* ---- stage-level entry points (parity tests bind these) ------------------ */
/* cvt_color(BGR2GRAY) on the integer image, utils.rs:136-142. out: w*h of the input depth
 * (u8 / u16 / f32), tightly packed, same location as the frame. */
stk_status stk_grey(stk_ctx* ctx, const stk_frames* frame /* n==1 */, void* out);
/* Mat::convert_to(CV_32F, alpha) utils.rs:133 (alpha = 1/255 there). */
stk_status stk_convert_f32(stk_ctx* ctx, const stk_frames* frame /* n==1 */, double alpha,
                           float* out);
/* ---- BASELINE configs[4]: ORB-seeded ECC on 8- or 16-bit stacks — an EXTENSION beyond the reference --------------
 * (both reference paths reject 16-bit input). Definition: ORB + RANSAC homography on the 8-bit grey
 * ((grey16 + 128) / 257 for 16-bit frames), H / h22 cast to f32 is the initial warp of findTransformECC (Homography)
 * on float(grey), fold with alpha = 1/65535 (16-bit) or 1/255 (8-bit). A frame without a homography starts from the
 * identity; nothing is dropped. stats carry the ECC result plus the keypoint / match / inlier counts. */
stk_status stk_hybrid_match(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* kp_params,
                            const stk_ecc_params* ecc_params, stk_image_f32* out, stk_frame_stats* stats);
stk_status stk_hybrid_match_shard(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* kp_params,
                                  const stk_ecc_params* ecc_params, int32_t add_reference, stk_image_f32* sum,
                                  int32_t* n_added, stk_frame_stats* stats);

/* ---- file front-end ---------------------------------------------------------
 * imgcodecs::imread(path, IMREAD_UNCHANGED) (utils.rs:110-117, 132) for binary PNM (P5 / P6, 8 or 16 bit), grey / YCbCr / CMYK
 * JPEG (libjpeg-turbo's libjpeg.so.8, OpenCV's decoder family at its default settings), PNG (libpng16.so.16: 8- and 16-bit
 * grey / RGB, palette -> BGR, 1/2/4-bit grey -> 8 bit; anything with alpha — RGBA, grey + alpha, a tRNS chunk — comes out as
 * FOUR channels B G R A, as OpenCV's decoder delivers it under IMREAD_UNCHANGED) and 8/16-bit grey / RGB TIFF, stripped or
 * tiled (libtiff.so.5 / .6), the libraries loaded at run time: BGR(A) or grey rows, tightly packed, into `data` (capacity_bytes);
 * data == NULL only reports the geometry. ctx may be NULL. A file that is unreadable or not an image: STK_BACKEND_ERROR (the
 * reference's empty Mat + cvtColor). RGBA TIFF gives four channels; BMP (no library:
 * uncompressed 24-bit, 32-bit -> B G R A, 8-bit palette -> BGR or grey); still WebP (libwebp.so.7: BGR, or B G R A when the
 * bitstream has alpha). CMYK / YCCK JPEG comes out as B G R through
 * OpenCV's own conversion. Flavours no decoder here takes (planar TIFF, RLE / 1- / 4- / 16-bit BMP, animated WebP,
 * EXR / JPEG 2000 ...): STK_NOT_IMPLEMENTED — the caller decodes those itself and uses the frame-based entry points. */
stk_status stk_imread(stk_ctx* ctx, const char* path, void* data, size_t capacity_bytes, int32_t* width,
                      int32_t* height, int32_t* channels, int32_t* depth);
/* keypoint_match / ecc_match in the reference's own call shape: a list of file paths, first = reference frame
 * (lib.rs:129-137, 702-710). `out` is a host or device image as for the frame-based entry points. */
stk_status stk_keypoint_match_files(stk_ctx* ctx, const char* const* paths, int32_t n, const stk_keypoint_params* params,
                                    float scale_down_width, stk_image_f32* out, int32_t* dropped, stk_frame_stats* stats);
stk_status stk_ecc_match_files(stk_ctx* ctx, const char* const* paths, int32_t n, const stk_ecc_params* params,
                               float scale_down_width, stk_image_f32* out, stk_frame_stats* stats);
/* stk_hybrid_match on a list of paths (8-bit PNM / PNG / TIFF, 16-bit PNM / TIFF). */
stk_status stk_hybrid_match_files(stk_ctx* ctx, const char* const* paths, int32_t n, const stk_keypoint_params* kp_params,
                                  const stk_ecc_params* ecc_params, stk_image_f32* out, stk_frame_stats* stats);

/* sharpness_modified_laplacian / _variance_of_laplacian / _tenengrad(k_size) / _normalized_gray_level_variance
 * (lib.rs:1030-1166; the pre-filter of examples/main.rs:40-47) of a single-channel 8-bit or f32 image, tightly packed.
 * `ksize` is read by TENG only (1, 3, 5 or 7, else STK_INVALID_PARAMS like lib.rs:1105). */
enum { STK_SHARPNESS_LAPM = 0, STK_SHARPNESS_LAPV = 1, STK_SHARPNESS_TENG = 2, STK_SHARPNESS_GLVN = 3 };
stk_status stk_sharpness(stk_ctx* ctx, const void* grey, int32_t depth, int32_t width, int32_t height,
                         int32_t location, int32_t metric, int32_t ksize, double* out);

/* ---- score and rank a whole stack: the first half of the example program (examples/main.rs:35-64) ---------------
 * All four metrics of every frame of an 8-bit stack in ONE device pass: each frame is read once, its integer grey
 * (stk_grey's, bit for bit; one-channel frames are taken as they are) exists in on-chip memory only, and one copy behind
 * one synchronisation brings the sums of all frames back. scores: n x 4 doubles, frame-major, in the order of the
 * STK_SHARPNESS_* enum; each is the very double stk_sharpness returns for stk_grey of that frame (the sums are exact
 * integers, so nothing depends on how the pass is cut up). frames: 1, 3 or 4 channels, host or device memory, any
 * row stride (a frame whose base address or row stride is no multiple of 4 is read byte by byte: same result, slower);
 * host frames are copied over in batches that fit the context's frame workspace. ksize is TENG's: 1, 3, 5
 * or 7, else STK_INVALID_PARAMS ("Kernel size must be 1, 3, 5, or 7", lib.rs:1105). 16-bit and f32 frames:
 * STK_NOT_IMPLEMENTED (the reference scores 8-bit greys, and the int64 sums hold 8-bit input only; for the same reason
 * frames above 2^27 pixels). stk_timing.prep_ms is the device time of the pass (for host frames with their copies), every
 * other field 0. A multi-device context scores on its first device. */
stk_status stk_stack_sharpness(stk_ctx* ctx, const stk_frames* frames, int32_t ksize, double* scores /* n x 4 */);

enum { STK_QUALITY_WEIGHT_NONE = 0, STK_QUALITY_WEIGHT_SCORE = 1 };
typedef struct {
    int32_t metric;                 /* STK_SHARPNESS_*: the column the frames are ranked by (the example: TENG) */
    int32_t ksize;                  /* TENG's kernel size for the scoring pass: 1, 3, 5 or 7 (stk_rank_frames ignores it) */
    int32_t drop_worst;             /* the example's skip(1): this many of the lowest-ranked frames are dropped; >= 0 */
    float   keep_fraction;          /* 0 = off; in (0, 1]: keep the best max(1, ceil(keep_fraction * n)) frames (the product in
                                       double, from the float's own value); not together with drop_worst != 0 */
    int32_t weight_mode;            /* STK_QUALITY_WEIGHT_* */
    int32_t reserved;               /* 0 */
} stk_select_params;

/* The example's sort / skip / reverse (main.rs:53, 64) on scores as stk_stack_sharpness returns them. Host code: no
 * context, no GPU. A stable ascending sort by the chosen metric, skip the first drop_worst, reverse: order[0 .. n_kept)
 * are the kept frames' indices, best first — order[0] is the frame the example makes the reference —, and equal scores
 * come out in DESCENDING frame index. The rest of order holds the dropped frames (best first), so order is always a
 * permutation of 0 .. n-1. n_kept = n - drop_worst, or max(1, ceil(keep_fraction * n)), at most n; n_kept < 1 (and
 * n < 1): STK_NOT_ENOUGH_FILES. The example compares with partial_cmp(..).unwrap_or(Equal): a NaN score is equal to every
 * other, which orders nothing consistently; defined here as what a straight insertion sort (Rust's own on short slices)
 * makes of it: the NaN frame keeps its place and no frame moves across it (computed run by run: O(n log n) for any n).
 * weights_or_null: n floats BY POSITION IN order (weights[i] belongs to frame order[i]) for the `weights` of the weighted
 * combines: STK_QUALITY_WEIGHT_SCORE gives a kept frame (float)(its score / the best kept score), or 1 if that best
 * score is 0; STK_QUALITY_WEIGHT_NONE, and every dropped frame, 1. */
stk_status stk_rank_frames(const double* scores /* n x 4 */, int32_t n, const stk_select_params* select,
                           int32_t* order /* n */, int32_t* n_kept, float* weights_or_null /* n */);

/* stk_ecc_match / stk_keypoint_match behind the ranking: score the stack (stk_stack_sharpness with select->ksize), select
 * (stk_rank_frames), and run the plain call on the kept frames in ranked order — by definition the plain call's result
 * on the list {frames->data[order[0]], .., frames->data[order[n_kept - 1]]}, bit for bit; only the pointers are
 * permuted. out, dropped, stats and errors are the plain call's; stats_or_null has n_kept entries in the order of that
 * list. order: n entries, n_kept, scores_or_null (n x 4) as above. 8-bit BGR(A) frames; host frames cross to the device
 * twice, for the scoring pass and again, in ranked order, inside the plain call. stk_timing is the plain call's with the
 * scoring pass's device time added to prep_ms. The clipped, quantile and weighted combines have no ranked form:
 * score, rank, permute the list and call them (stk_rank_frames' weights fit their `weights`). */
stk_status stk_ecc_match_ranked(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                stk_image_f32* out, stk_frame_stats* stats_or_null, const stk_select_params* select,
                                int32_t* order, int32_t* n_kept, double* scores_or_null);
stk_status stk_keypoint_match_ranked(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                     float scale_down_width, stk_image_f32* out, int32_t* dropped,
                                     stk_frame_stats* stats_or_null, const stk_select_params* select, int32_t* order,
                                     int32_t* n_kept, double* scores_or_null);

/* ---- per-frame noise estimation and inverse-variance frame weights (an extension beyond the reference) -----------
 * Every combine takes a per-frame weight; for a deep-sky stack the weight that minimises the result's noise is the
 * inverse of the frame's noise variance. stk_stack_noise measures that noise, per frame and channel, on the frame's OWN
 * grid (before any warp: interpolation changes the noise), from two exact histograms that one device pass produces:
 *   HV: the counts of v(x, y) over all w x h pixels; BV = 256 bins at depth 8, 65 536 at depth 16.
 *   HR: the counts of min(|r(x, y)|, BR - 1) over the (w - 2)(h - 2) interior pixels 1 <= x <= w - 2, 1 <= y <= h - 2 (no
 *       border extension: a pixel outside the frame forms no address), r = Immerkaer's noise mask in integers,
 *           r = v(x-1,y-1) - 2 v(x,y-1) + v(x+1,y-1) - 2 v(x-1,y) + 4 v(x,y) - 2 v(x+1,y) + v(x-1,y+1) - 2 v(x,y+1) + v(x+1,y+1).
 *       Depth 8: BR = 2041 (|r| <= 8 x 255: the cap never acts). Depth 16: BR = 65 536, and the last bin collects every
 *       |r| >= 65 535 (the overflow bin).
 * Counts are uint32 and exact: tiling, launch shape and summation order cannot change a bit.
 *
 * stk_noise_from_hist reduces one (frame, channel)'s pair of histograms. Host code: no context, no GPU; f64 and integers,
 * in this order:
 *   1. n = sum HV, k = (n + 1) / 2; median = the k-th smallest value; mad = the k-th smallest |v - median| (the smallest d
 *      with #{|v - median| <= d} >= k, from the cumulative counts). An empty histogram gives 0 and 0.
 *   2. m = sum HR, k' = (m + 1) / 2; res_median = the k'-th smallest capped |r|.
 *   3. s = max(1.4826 * (double)res_median, 0.5); top = overflow_bin ? br - 2 : br - 1; prev = -1.
 *   4. at most 16 rounds: cut = min((int)floor(3.0 * s), top); stop when cut == prev, else prev = cut;
 *      N = sum_{b <= cut} HR[b], Q = sum_{b <= cut} b^2 HR[b] (int64, exact); if N == 0 or Q == 0: sigma = 0, flag bit 0,
 *      stop; s = sqrt((double)Q / (double)N) * 1.0136 (the 3-sigma truncation correction 1 / sqrt(1 - 6 phi(3) / (2 Phi(3) - 1))).
 *   5. sigma = s / 6.0 (the mask's coefficients have squared sum 36); kept = N of the last round.
 *   6. flag bit 1: overflow_bin is set and the last cut == top — the noise is beyond what the capped histogram resolves.
 * bv in [1, 65 536], br in [2, 65 536], overflow_bin 0 or 1, no null pointer: else STK_INVALID_PARAMS. Below sigma = 1.5
 * grey levels the quantisation's 1/12 biases the estimate upward. */
typedef struct {
    int32_t median;                 /* of the values */
    int32_t mad;                    /* median absolute deviation of the values from `median` */
    int32_t res_median;             /* median of the capped |r| */
    int32_t flags;                  /* bit 0: no residual energy under the cut (sigma = 0); bit 1: the cut reached the cap */
    double  sigma;                  /* the noise's standard deviation in grey levels of the frame's depth */
    int64_t kept;                   /* residuals under the last cut */
} stk_noise_stat;
stk_status stk_noise_from_hist(const uint32_t* hv, int32_t bv, const uint32_t* hr, int32_t br, int32_t overflow_bin,
                               stk_noise_stat* out);

/* The histograms and statistics of every frame and channel of a u8 or u16 stack in one device pass: each frame is read
 * once. frames: 1, 3 or 4 channels (a fourth channel is treated like the others), host or device memory, any row stride (a
 * frame whose base address or row stride is no multiple of 4 is read element by element: same result, slower); host
 * frames and large stacks go through the context's workspaces in batches. stats: n x 4, frame-major, the unused channel
 * slots zeroed; each is stk_noise_from_hist of that frame and channel (overflow_bin = 1 at depth 16). hist_or_null: host
 * memory, n x channels x (BV + BR) uint32, HV then HR per frame and channel. The device histograms are zeroed on the
 * call's stream inside the call: no result depends on what the context held before. width or height below 3:
 * STK_INVALID_PARAMS; f32 frames, and frames above 2^27 pixels (the int64 sums stay exact within it): STK_NOT_IMPLEMENTED.
 * stk_timing.prep_ms is the device time of the pass (for host frames with their copies), every other field 0; the host
 * reduction is not in it. A multi-device context uses its first device. */
stk_status stk_stack_noise(stk_ctx* ctx, const stk_frames* frames, stk_noise_stat* stats /* n x 4 */, uint32_t* hist_or_null);

/* Inverse-variance weights from the statistics. Host code: no context, no GPU. With C = min(channels, 3),
 *   V_i = sum_{c < C} (g_ic * max(sigma_ic, sigma_floor))^2     (f64, c ascending; g_ic = records[i].gain[c], or 1 without records),
 *   w_i = (float)((u_i * V_ref) / V_i),                          u_i = weights_or_null[i], or 1; ref = the first included frame;
 * an excluded frame (include_or_null[i] == 0) gets weight 0. This is the inverse variance of the frame AFTER the combine's
 * own gain has mapped it onto the reference, so normalisation and weighting compose: pass the gains the fold will apply.
 * The change of the noise under the fold's interpolation (a bilinear or bicubic sample averages neighbours, by an amount
 * that depends on the sub-pixel phase) is NOT modelled. stats: n x 4 as stk_stack_noise returns them. sigma_floor must be
 * finite and > 0, every u_i finite and >= 0, every sigma read finite and >= 0, every gain read finite, V_i > 0, channels 1,
 * 3 or 4, n >= 1, one frame included: else STK_INVALID_PARAMS. */
stk_status stk_noise_weights(const stk_noise_stat* stats /* n x 4 */, int32_t n, int32_t channels,
                             const stk_frame_weight* records_or_null, const int32_t* include_or_null,
                             const float* weights_or_null, double sigma_floor, float* weights_out /* n */);

/* stk_ecc_match_weighted / stk_keypoint_match_weighted with the weights from the frames' noise. By definition each equals
 * its parts, bit for bit: (1) the plain call's stats; (2) the weighted form's gain / offset estimate from the overlap moments
 * (weight->normalize); (3) stk_stack_noise on the same frames; (4) stk_noise_weights with those records, the caller's
 * weights_or_null as u and sigma_floor, the frames the plain call dropped excluded; (5) stk_weighted_stack with the
 * resulting records. applied_or_null returns what the fold used; noise_or_null (n x 4) the statistics. The frames are
 * still resident in HBM for the noise pass: nothing is uploaded again. stk_timing is the plain call's but for
 * finalize_ms, which holds the moments pass, the noise pass and the fold. Frames of depth 8 or 16 where the plain call
 * takes them; the refusals of stk_stack_noise and stk_noise_weights apply. The clip, quantile, drizzle and star combines
 * have no such form: compose stk_stack_noise + stk_noise_weights + the *_stack call. */
stk_status stk_ecc_match_noise_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_ecc_params* params, float scale_down_width,
                                        const stk_weight_params* weight, const float* weights_or_null, double sigma_floor,
                                        stk_image_f32* out, float* coverage_or_null, stk_frame_weight* applied_or_null,
                                        stk_frame_stats* stats_or_null, stk_noise_stat* noise_or_null);
stk_status stk_keypoint_match_noise_weighted(stk_ctx* ctx, const stk_frames* frames, const stk_keypoint_params* params,
                                             float scale_down_width, const stk_weight_params* weight, const float* weights_or_null,
                                             double sigma_floor, stk_image_f32* out, int32_t* dropped, float* coverage_or_null,
                                             stk_frame_weight* applied_or_null, stk_frame_stats* stats_or_null,
                                             stk_noise_stat* noise_or_null);

/* ---- background model: per-frame sky level on a node grid: an EXTENSION beyond the reference ------------------------
 * A light-pollution or moonlight gradient is a smooth additive field of the frame, not of the stack: star detection's
 * piecewise tile median, local normalisation (which maps onto frame 0, gradient included) and the noise pass's one median
 * per frame all let it through. This section measures, per frame and colour channel, the sky level on the node grid of
 * the mesh section from exact clipped order statistics of the window around each node, interpolates it bilinearly and
 * subtracts it (flatten). It runs per frame before registration, or on a finished stack (a one-frame f32 stk_frames).
 * Grid and windows. Nodes are those of stk_mesh_grid(w, h, step), step 16, 32, 64 or 128; node (j, k) sits at
 *   q = (k step, j step). On one axis the window of a node is the inclusive pixel range a = max(q - step / 2, 0) ..
 *   b = min(q + step / 2, size - 1); it is empty when a > b (a last node beyond the frame); its centre is p = (a + b) / 2.
 *   Windows of neighbouring nodes share one pixel row or column; a window holds at most (step + 1)^2 pixels.
 * Key, per channel c < C = min(channels, 3) (a sky gradient is coloured; channel 3, alpha, is never read by the
 *   statistics): the sample itself for u8 and u16 frames; for f32 frames (int)fminf(fmaxf(rintf(sample * f32_scale), 0),
 *   65535) (NaN gives 0), the key of stk_star_deep_params.
 * Mask (optional): w x h bytes, tightly packed, host or device memory, one for the whole stack; a pixel whose byte is
 *   non-zero is excluded.
 * Window record (stk_bg_cell), all integers, on the device. W = the multiset of the window's unmasked keys, n = |W|.
 *   n = 0: the record is all zeros. Else lo_0 = 0, hi_0 = 65535 and for t = 0 .. T (T = clip_iters):
 *     S_t = {K in W : lo_t <= K <= hi_t}; m = (|S_t| + 1) / 2; med_t = the m-th smallest of S_t; mad_t = the m-th smallest
 *     |K - med_t| over S_t; for t < T: d = max((int)fminf(ceilf(ks * (float)mad_t), 65536.0f), 1), ks = (float)((double)kappa
 *     * 1.4826); lo_{t+1} = max(lo_t, med_t - d); hi_{t+1} = min(hi_t, med_t + d).
 *   S_t is never empty (med_t is in S_{t+1}). The record holds n, kept = |S_T|, med = med_T, mad = mad_T, lo = lo_T,
 *   hi = hi_T, sum = the sum of K and sum2 the sum of K^2 over S_T. Counts and sums are integers: no result depends on
 *   the order in which anything is added, and a call returns the same bits every time.
 * Estimator (stk_background_estimate: host code, no context), in f64 unless stated, per channel:
 *   mean = sum / kept. Level by `estimator`: 0 MEDIAN: med; 1 MEAN: mean; 2 MODE: s = 1.4826 max(mad, 1), the level is
 *   2.5 med - 1.5 mean when |mean - med| <= 0.3 s, else med. rms = sqrt(max(sum2 / kept - mean mean, 0)). A record with
 *   kept = 0 has level 0 and rms 0.
 *   A (node, channel) is valid iff kept >= min_count (0 = 64) and (double)(n - kept) <= (double)max_reject (double)n.
 *   Then, in this order:
 *   1. Recentre (recentre = 1): a window cut by the frame measures the level at p, not at q. An x pass over the input
 *      values (no cascade): for a valid node with p_k != q_k, kn = k + 1 if p_k > q_k, else k - 1; if kn is in the grid,
 *      (j, kn) is valid and p_kn != p_k: L' = L + ((L - L_kn) (q_k - p_k)) / (p_k - p_kn). Then the same along y on the x
 *      pass's output.
 *   2. For f32 frames level and rms are divided by (double)f32_scale. Both are rounded to f32: the planes are in SAMPLE
 *      units.
 *   3. Filter (filter = 1): a valid node whose 3 x 3 neighbourhood lies wholly in the grid and is wholly valid takes the
 *      5th smallest of the nine input values; every other node keeps its value.
 *   4. Edge extrapolation, for the last column and then the last row (the last node may lie beyond the frame with an
 *      empty or thin window): if (j, gw - 1) is invalid and (j, gw - 2) and (j, gw - 3) are valid, L = (a + a) - b in f32,
 *      a = L(j, gw - 2), b = L(j, gw - 3), and the node counts as valid. Then the same for row gh - 1, on that output.
 *   5. Fill: `fill` passes of the mesh section's "Fill" arithmetic on the level, with the validity so far as m.
 *   6. Fallback: a node still invalid takes the lower median of the channel's valid levels as they stood before the
 *      fill; when the channel has no valid node the level is 0 and bit c of `flags` is set.
 *   The rms plane skips steps 1, 3 and 4: it is filled with the validity the levels had before step 4 and takes the same
 *   kind of fallback (the lower median of its valid values, or 0).
 *   Outputs: the level plane gh x gw x C f32; the rms plane of the same shape; valid: gh x gw int32, bit c, as it stood
 *   before step 4; flags.
 * Apply. Pixel (x, y), channel c < C: B_c = the local-normalisation section's chain on the level plane (k, j, k1, j1, u, v,
 *   then three fmas on the C components per node); v = ((float)raw - B_c) + target[c], each operation rounded on its
 *   own. Channel 3 is (float)raw. out_depth, rounding, saturation, out, out_row_stride_bytes, the overlap refusal, padded
 *   and misaligned rows, host and device frames follow stk_calibrate. A NULL plane means B = 0. Plane values are expected
 *   finite and are not checked.
 * Not here: division (a multiplicative flatten), spline or polynomial surfaces, subtraction inside the folds, in-place
 *   output, shard and files forms. A multi-device context runs these calls on its first device. */
enum { STK_BG_MEDIAN = 0, STK_BG_MEAN = 1, STK_BG_MODE = 2 };
typedef struct {
    int32_t n;            /* unmasked pixels of the window */
    int32_t kept;         /* |S_T| */
    int32_t med, mad;     /* of S_T */
    int32_t lo, hi;       /* the last clip range */
    int32_t reserved[2];  /* 0 */
    int64_t sum;          /* of K over S_T */
    uint64_t sum2;        /* of K^2 over S_T */
} stk_bg_cell;            /* 48 bytes */
typedef struct {
    int32_t step;         /* node spacing: 16, 32, 64 or 128 */
    int32_t clip_iters;   /* T: 0 .. 5 */
    float   kappa;        /* finite, > 0 */
    float   f32_scale;    /* finite, > 0; read for f32 frames only */
    int32_t estimator;    /* STK_BG_MEDIAN, STK_BG_MEAN, STK_BG_MODE */
    int32_t min_count;    /* >= 0; 0 = 64 */
    float   max_reject;   /* 0 .. 1 */
    int32_t recentre;     /* 0 or 1 */
    int32_t filter;       /* 0 or 1 */
    int32_t fill;         /* 0 .. 16 */
    float   target[4];    /* finite: the level the flattened sky is put at, per channel */
    int32_t out_depth;    /* the frames' depth or STK_DEPTH_F32 (read by stk_background_flatten) */
    int32_t reserved[3];  /* 0 */
} stk_background_params;
/* Anything outside the ranges above is STK_INVALID_PARAMS.
 * The window records of every frame in one launch. mask_or_null: the mask in mask_location (STK_HOST or STK_DEVICE).
 * cells: n x gh x gw x C records on the host, frame index order. stk_timing.finalize_ms is the launch. */
stk_status stk_background_cells(stk_ctx* ctx, const stk_frames* frames, const stk_background_params* params,
                                const uint8_t* mask_or_null, int32_t mask_location, stk_bg_cell* cells);
/* The estimator for one frame: pure host code, no context (a bad argument is STK_INVALID_PARAMS without a message).
 * depth: the frames' (8, 16 or 32). cells_of_one_frame: gh x gw x C records. level: gh x gw x C f32. */
stk_status stk_background_estimate(int32_t width, int32_t height, int32_t channels, int32_t depth,
                                   const stk_background_params* params, const stk_bg_cell* cells_of_one_frame, float* level,
                                   float* rms_or_null, int32_t* valid_or_null, int32_t* flags_or_null);
/* Apply alone. planes: n host level planes by frame index for the grid of `step` (an entry, or the array, may be NULL:
 * B = 0). target: 4 floats. out: n images in the frames' location, as in stk_calibrate. finalize_ms is the launch. */
stk_status stk_background_apply(stk_ctx* ctx, const stk_frames* frames, const float* const* planes, int32_t step,
                                const float* target, int32_t out_depth, void* const* out, size_t out_row_stride_bytes);
/* The whole-stack form: by definition, and bit for bit, stk_background_cells, stk_background_estimate per frame and
 * stk_background_apply with params->target and params->out_depth, in sequence; host frames are uploaded once.
 * planes_out_or_null / rms_out_or_null: n host planes by frame index, NULL entries skipped; cells_out_or_null: all records
 * as stk_background_cells returns them. finalize_ms is the two launches. */
stk_status stk_background_flatten(stk_ctx* ctx, const stk_frames* frames, const stk_background_params* params,
                                  const uint8_t* mask_or_null, int32_t mask_location, void* const* out,
                                  size_t out_row_stride_bytes, float* const* planes_out_or_null, float* const* rms_out_or_null,
                                  stk_bg_cell* cells_out_or_null);

/* ---- deconvolution: Richardson-Lucy on a finished stack, with a PSF from its stars: an EXTENSION beyond the reference --
 * The consumer of the measured star shapes (stk_star_measure): a PSF model from their second moments, and the
 * Richardson-Lucy iteration of a linear f32 image with it, optionally with the total-variation regulariser of Dey et al.
 * It runs on the finished stack, after the combine and stk_background_flatten, before any stretch.
 * Everything is f32 and each operation is rounded on its own (no contraction); every fmaf below is one; `/` and sqrtf are
 * the correctly rounded ones.
 * Inputs: an stk_image_f32 d with 1, 3 or 4 channels; a PSF P[(2R+1)^2], row-major, R = radius; optionally a one-channel
 *   f32 mask plane M (width x height, its own row stride in bytes, 0 = tightly packed; host or device memory). Channels
 *   are processed independently with the same PSF; with 4 channels the fourth (alpha) is copied through unchanged.
 * 1. D(q) = d(q) + pedestal; a D that is not finite or is below 0 becomes 0. u_0 = D.
 * 2. For k = 0 .. iterations - 1, coordinates outside the image mapped by BORDER_REFLECT_101:
 *      A(q) = sum_j sum_i P[j+R][i+R] u_k(x - i, y - j): acc = 0.0f; acc = fmaf(P, u, acc), j = -R .. R outermost, i = -R .. R
 *        inside it (a true convolution).
 *      r(q) = D(q) / fmaxf(A(q), floor).
 *      C(q) = sum_j sum_i P[j+R][i+R] r(x + i, y + j), same order, same border (a correlation: the flipped PSF).
 *      v(q) = u_k(q) C(q).
 *      lambda == 0: u_{k+1} = v. lambda > 0, forward differences:
 *        gx(q) = u_k(x+1, y) - u_k(q), 0 in the last column; gy(q) = u_k(x, y+1) - u_k(q), 0 in the last row;
 *        n = sqrtf(fmaf(gx, gx, fmaf(gy, gy, e2))), e2 = tv_eps * tv_eps computed once on the host in f32;
 *        px = gx / n; py = gy / n; div(q) = (px(q) - px(x-1, y)) + (py(q) - py(x, y-1)), px at x = -1 and py at y = -1 are 0;
 *        u_{k+1}(q) = v(q) / fmaxf(fmaf(-lambda, div, 1.0f), 0.5f).
 * 3. m(q) = amount without a mask, else amount * M(q). m == 1.0f: o = u_K - pedestal; else o = fmaf(m, u_K - D, D) - pedestal.
 * Checks (anything else is STK_INVALID_PARAMS): iterations 1 .. 1000; radius 1 .. 16; width and height >= radius + 1;
 *   floor finite and > 0; pedestal finite; lambda finite and >= 0; tv_eps finite and > 0; amount 0 .. 1; reserved 0; every
 *   PSF tap finite and >= 0; the PSF's f64 sum (row-major order) within 1e-3 of 1.
 * In place: `out` may be exactly the input (same pointer, same row stride): the work runs on workspace copies. Any other
 *   overlap of out with the input or the mask in the same memory space is refused. out has the input's geometry and location.
 * No result depends on scheduling, on the tiling or on what the context held before; a padded or misaligned image gives
 *   the bits of its tight copy; host and device images give the same bits. Only pixel bytes are written.
 * Not here: an empirical PSF from star cut-outs, a separable path for rank-1 PSFs, per-channel or spatially varying PSFs,
 *   early stopping, automatic star-protection masks, shard and files forms. A multi-device context uses its first device. */
enum { STK_PSF_GAUSSIAN = 0, STK_PSF_MOFFAT = 1 };
typedef struct {
    int32_t iterations;   /* 1 .. 1000, default 30 */
    int32_t radius;       /* R, 1 .. 16, default 8 */
    float   floor;        /* finite, > 0, default 1e-6 */
    float   pedestal;     /* finite, default 0 */
    float   lambda;       /* finite, >= 0; 0 = no regulariser; default 0 */
    float   tv_eps;       /* finite, > 0, default 1e-3 */
    float   amount;       /* 0 .. 1, default 1 */
    int32_t reserved;     /* 0 */
} stk_deconv_params;
/* psf: (2R+1)^2 host floats. stk_timing.finalize_ms is the launches alone; prep_ms and warp_ms are the ratio and the update
 * launch of the last iteration. */
stk_status stk_deconvolve(stk_ctx* ctx, const stk_image_f32* in, const float* psf, const stk_deconv_params* params,
                          const float* mask_or_null, size_t mask_stride_bytes, int32_t mask_location, stk_image_f32* out);
/* A PSF model from a covariance (host code, f64, no context): with d = (i, j), i, j = -radius .. radius, and
 * q = d^T S^-1 d, S = [[cxx, cxy], [cxy, cyy]]: STK_PSF_GAUSSIAN exp(-q / 2); STK_PSF_MOFFAT
 * pow(1 + q (2^(1/beta) - 1) / (2 ln 2), -beta), which has the Gaussian's half-maximum contour. In f64, each operation
 * rounded on its own: det = cxx cyy - cxy cxy; q = ((cyy i) i - (2 cxy i) j + (cxx j) j) / det; Moffat's
 * g = (pow(2, 1 / beta) - 1) / (2 log(2)) once, value pow(1 + q g, -beta). Sampled at pixel centres, divided by the f64 sum taken in row-major order,
 * cast to f32; psf: (2 radius + 1)^2 floats, row j then column i. S not positive definite (cxx > 0, cyy > 0, det > 0,
 * all finite), beta not finite or <= 1 for Moffat, an unknown kind, radius outside 1 .. 16, null psf: STK_INVALID_PARAMS. */
stk_status stk_psf_model(int32_t kind, double beta, int32_t radius, double cxx, double cyy, double cxy, float* psf);
/* The covariance of a frame's stars (host code): over the `count` shapes with flags == 0 and snr >= min_snr the lower
 * medians (the ((m + 1) / 2)-th smallest of m) of cxx, cyy and cxy, each on its own, each multiplied by scale * scale
 * (isophotal moments read a few per cent low; 1 = as measured). used: m (may be null). No shape left, a result that is not
 * finite or not positive definite, count < 0, scale or min_snr not finite, scale <= 0, null arguments: STK_INVALID_PARAMS. */
stk_status stk_psf_from_shapes(const stk_star_shape* shapes, int32_t count, double min_snr, double scale, double* cxx,
                               double* cyy, double* cxy, int32_t* used_or_null);

/* ---- wavelet layers: the a trous (starlet) decomposition of a finished stack: an EXTENSION beyond the reference ---------
 * Multiscale denoising (thresholds on the fine layers against the noise those layers carry), sharpening (gains on the fine
 * layers), separation of structures by scale, and the noise of a finished f32 stack (the first layer's MAD). It runs on
 * the linear f32 stack beside stk_deconvolve: after the combine and stk_background_flatten, before any stretch.
 * Everything is f32 and each operation is rounded on its own (no contraction); every fmaf below is one. Channels are
 * processed independently; with 4 channels the fourth (alpha) is copied through unchanged.
 * Inputs: an stk_image_f32 d with 1, 3 or 4 channels, host or device, any row stride that is a multiple of 4 bytes;
 *   levels J, 1 .. 8; optionally a one-channel f32 mask plane M (width x height, its own row stride in bytes, 0 = tightly
 *   packed; host or device memory), as stk_deconvolve takes it.
 * 1. D(q) = d(q) if it is finite and fabsf(d) <= 1e30f, else 0. c_0 = D. Every later value is finite.
 * 2. For j = 0 .. J - 1, s = 2^j, indices outside the image mapped by BORDER_REFLECT_101 (one reflection is enough: see
 *    the size check):
 *      hx(x, y): a = 0.0625f c_j(x - 2s, y); a = fmaf(0.25f, c_j(x - s, y), a); a = fmaf(0.375f, c_j(x, y), a);
 *                a = fmaf(0.25f, c_j(x + s, y), a); a = fmaf(0.0625f, c_j(x + 2s, y), a).
 *      c_{j+1}(x, y): the same chain over hx(x, y - 2s), hx(x, y - s), hx(x, y), hx(x, y + s), hx(x, y + 2s).
 *      w_j = c_j - c_{j+1}.
 * 3. The layer operation, with the f32 values t_j (step 5), keep_j = 1 - layer_amount_j (f32, on the host) and gain_j;
 *    m = fabsf(w_j):
 *      STK_WAVELET_HARD: w' = m < t_j ? w_j keep_j : w_j.
 *      STK_WAVELET_SOFT: z = copysignf(fmaxf(m - t_j, 0), w_j); w' = fmaf(layer_amount_j, z - w_j, w_j).
 *      acc_0 = gain_0 w'_0; acc_j = acc_{j-1} + gain_j w'_j.
 * 4. res = fmaf(residual_gain, c_J, acc_{J-1}). mm = amount without a mask, else amount * M(q). mm == 1.0f: o = res; else
 *    o = fmaf(mm, res - D, D).
 * 5. t_j = (float)(threshold_j * sigma_c * e_j) in f64 on the host, for channel c. e_j is the standard deviation of layer j
 *    of unit white noise, derived from the filter (stk_wavelet_noise_table): with a_j the 1-D impulse response of the
 *    cascade up to c_j (a_0 = the unit impulse), e_j^2 = (sum a_j^2)^2 - 2 (sum a_j a_{j+1})^2 + (sum a_{j+1}^2)^2 in f64.
 *    sigma_c is the caller's (sigma_given != 0: sigma[c]) or estimated: sigma_c = (float)(1.4826 * (double)med_c / e_0),
 *    med_c the lower median (the ((N + 1) / 2)-th smallest of N = width * height) of fabsf(w_0) over the channel, exact.
 *    The estimation pass runs only where it is needed: some threshold_j > 0 (j < levels) with sigma not given, or the caller
 *    asked for sigma. sigma = 0 gives t = 0 and nothing is below it. A sigma that was neither given nor estimated reads 0.
 * Checks (anything else is STK_INVALID_PARAMS): levels 1 .. 8; min(width, height) >= 2^levels + 1; gains and residual_gain
 *   finite; thresholds finite and >= 0; layer_amount and amount 0 .. 1 (all eight entries of each table are checked); given
 *   sigmas finite and >= 0; a known mode; reserved 0; out has the input's geometry and location.
 * In place: `out` may be exactly the input (same pointer, same row stride). Any other overlap of an output with the input,
 *   the mask or another output in the same memory space is refused.
 * No result depends on scheduling, on the tiling or on what the context held before; a padded or misaligned image gives
 *   the bits of its tight copy; host and device images give the same bits. Only pixel bytes are written.
 * Not here: per-layer MAD instead of the table, a multiscale median transform, deringing, per-channel parameters, a
 *   stretch, shard and files forms. A multi-device context uses its first device. */
enum { STK_WAVELET_HARD = 0, STK_WAVELET_SOFT = 1 };
typedef struct {
    int32_t levels;           /* J, 1 .. 8, default 4 */
    int32_t mode;             /* STK_WAVELET_HARD (default) or STK_WAVELET_SOFT */
    int32_t sigma_given;      /* != 0: sigma[] holds the noise per channel; 0 (default): estimated where needed */
    int32_t reserved;         /* 0 */
    float   gain[8];          /* finite, default 1 */
    float   threshold[8];     /* finite, >= 0, in units of the layer's noise; default 0 */
    float   layer_amount[8];  /* 0 .. 1, default 1 */
    float   residual_gain;    /* finite, default 1 */
    float   amount;           /* 0 .. 1, default 1 */
    float   sigma[4];         /* finite, >= 0; read when sigma_given != 0 */
} stk_wavelet_params;
/* Steps 1 - 5. sigma_out_or_null: 4 floats, the sigma of each colour channel as used (given, estimated, or 0 where neither);
 * entries from min(channels, 3) on are 0. With the defaults the call is the reconstruction: the input to within the f32
 * rounding of the sums. stk_timing.finalize_ms is the launches alone; prep_ms is the estimation pass (0 where it did not
 * run), warp_ms the launch of the last level and align_ms that of the level before it (0 with one level). */
stk_status stk_wavelet_process(stk_ctx* ctx, const stk_image_f32* in, const stk_wavelet_params* params, const float* mask_or_null,
                               size_t mask_stride_bytes, int32_t mask_location, stk_image_f32* out, float* sigma_out_or_null);
/* Steps 1 - 2 alone: out is an array of levels + 1 images of the input's geometry and location, w_0 .. w_{J-1} then c_J; bit
 * for bit the w_j and c_J that stk_wavelet_process uses. With 4 channels every output's fourth channel is the input's.
 * No output may overlap the input or another output. */
stk_status stk_wavelet_layers(stk_ctx* ctx, const stk_image_f32* in, int32_t levels, stk_image_f32* out);
/* The estimate of step 5 alone, the noise of a finished f32 stack: sigma: 4 floats (entries from min(channels, 3) on are
 * 0); median_or_null: 4 floats, med_c. The image must be at least 3 x 3. */
stk_status stk_wavelet_sigma(stk_ctx* ctx, const stk_image_f32* in, float* sigma, float* median_or_null);
/* e_0 .. e_{levels-1} of step 5 (host code, no context): 0.8907963103, 0.2006638510, 0.0855075048, ... levels outside
 * 1 .. 8 or a null table: STK_INVALID_PARAMS. */
stk_status stk_wavelet_noise_table(int32_t levels, double* e);

/* ---- display stretch: exact image statistics, the auto-stretch rule, the curve and the conversion to 8 or 16 bits: an
 * EXTENSION beyond the reference ---------------------------------------------------------------------------------------
 * The last step of every recipe: a finished stack is linear f32 with its sky at 1 - 3 % of full scale, so it is measured
 * (stk_image_stats), a black point and a midtones balance are set from the sky level and its spread (stk_stretch_auto), and a
 * non-linear curve and the output conversion are applied in one launch (stk_stretch). stk_auto_stretch is the three in one
 * call. Everything on the device is f32 and each operation is rounded on its own (no contraction); every fmaf below is one.
 * The host helpers work in f64, each operation rounded on its own too.
 * Inputs: an stk_image_f32 d with 1, 3 or 4 channels, host or device, any row stride that is a multiple of 4 bytes;
 *   cc = min(channels, 3) colour channels. The statistics optionally take a one-channel f32 mask plane M (width x height, its
 *   own row stride in bytes, 0 = tightly packed; host or device memory), as stk_deconvolve takes it.
 * 1. Statistics (stk_image_stats), per colour channel c. A sample counts iff it is finite and (there is no mask or
 *    M(q) > 0). Its value is v, with -0.0f counted as +0.0f (decided on the bits). Of the N samples that count:
 *      count = N; min; max; median = the lower median, the ((N + 1) / 2)-th smallest;
 *      mad = the lower median of fabsf(v - median), an f32 subtraction;
 *      q[i] for up to four quantiles p_i in 0 .. 1: the k-th smallest, k = min(N, max(1, (int64)ceil(p_i * N))) in f64.
 *    All of them exact: a radix selection on order-preserving 32-bit keys, integer counts, so nothing depends on the order
 *    of anything. N = 0, the alpha channel and the entries of q that were not asked for: zeros.
 * 2. The auto rule (stk_stretch_auto; host code, no context, f64), per colour channel from its record, with the constants
 *    of stk_stretch_auto_params:
 *      c0 = max(min, median + (shadows_clip * 1.4826) * mad);
 *      w = white (white_mode 0), max (1) or q[0] (2); if w <= c0 then w = c0 + 1;
 *      x0 = (median - c0) / (w - c0);
 *      m = ((target - 1) * x0) / ((2 * target - 1) * x0 - target), clamped to [1e-6, 1 - 1e-6]; x0 == 0: m = 0.5.
 *    (mtf(m, x) = t iff m = mtf(t, x): the midtone that sends the sky's median to the target.) linked != 0: median, mad, min
 *    and w are replaced by their means over the colour channels (summed in channel order, divided by cc) before the rule,
 *    so every colour channel gets the same three values. black = (float)c0, white = (float)w, midtone = (float)m; the
 *    entries from cc on are 0, 1 and 0.5. The record written is otherwise curve MTF, colour 0, out_depth F32, out_scale 1.
 * 3. The stretch (stk_stretch), per pixel, for the colour channels c < cc, with r_c = white_c - black_c,
 *    mm1_c = midtone_c - 1 and k_c = 2 midtone_c - 1 in f32 on the host:
 *      x_c = fminf(fmaxf((v_c - black_c) / r_c, 0), 1)      (the IEEE fmaxf: a NaN becomes 0; +inf 1; -inf 0)
 *      the curve f_c(x):
 *        STK_STRETCH_LINEAR: x.
 *        STK_STRETCH_MTF:    fminf(fmaxf((mm1_c x) / fmaf(k_c, x, -midtone_c), 0), 1).
 *        STK_STRETCH_TABLE:  K = knots, T the table of K + 1 floats, one for all channels: t = x (float)K;
 *                            i = min((int)t, K - 1); fr = t - (float)i; fmaf(T[i+1] - T[i], fr, T[i]).
 *      colour == 0 or channels == 1: y_c = f_c(x_c).
 *      colour == 1: L = ((x_0 + x_1) + x_2) / 3.0f; g = f_0(L); s = L > 0 ? g / L : 0; y_c = fminf(x_c s, 1): every channel
 *        is scaled by what the curve does to the luminance, so hue and saturation survive (what an asinh stretch is for).
 *      output: STK_DEPTH_F32: y_c out_scale. STK_DEPTH_U8 / U16: rintf(y_c 255.0f) / rintf(y_c 65535.0f), half to even
 *        (out_scale is not read).
 *      alpha (channels == 4): y_3 = fminf(fmaxf(v_3, 0), 1) through the same output step: no black point and no curve.
 * Checks (anything else is STK_INVALID_PARAMS): width * height < 2^31; at most four quantiles, each finite and in 0 .. 1;
 *   black_c and white_c finite with white_c > black_c (c < cc); midtone_c in (0, 1) under MTF (c < cc); knots 2 .. 65536 and
 *   every table value finite and in 0 .. 1 under TABLE; out_scale finite; known enums; reserved 0; out has the input's width,
 *   height, channels and location, and the depth of the parameters; shadows_clip <= 0; target_background in (0, 1); white
 *   finite; white_quantile in 0 .. 1; linked 0 or 1; white_mode 0 .. 2; the records given to the rule finite.
 * In place: with STK_DEPTH_F32, `out` may be exactly the input (same pointer, same row stride). Any other overlap of the
 *   output with the input in the same memory space is refused.
 * No result depends on scheduling, on the tiling or on what the context held before; a padded or misaligned image gives
 *   the bits of its tight copy; host and device images give the same bits. Only pixel bytes are written.
 * Not here: histogram equalisation and CLAHE, the inverted rule for bright backgrounds (median > 0.5), per-channel tables,
 *   white balance from star colours, star masks, a histogram output, shard and files forms, 8-bit input. A multi-device
 *   context uses its first device. */
enum { STK_STRETCH_LINEAR = 0, STK_STRETCH_MTF = 1, STK_STRETCH_TABLE = 2 };
enum { STK_CURVE_ASINH = 0, STK_CURVE_GAMMA = 1, STK_CURVE_SRGB = 2 };
typedef struct {
    int64_t count;            /* N: the samples of the channel that count */
    float   min, max;
    float   median, mad;      /* lower medians */
    float   q[4];             /* the quantiles asked for, in the caller's order */
} stk_image_stat;
typedef struct {
    int32_t curve;            /* STK_STRETCH_* */
    int32_t colour;           /* 0: per channel; 1: colour-preserving (3 or 4 channels; with 1 channel it is per channel) */
    int32_t out_depth;        /* STK_DEPTH_U8 / U16 / F32 */
    int32_t reserved;         /* 0 */
    float   black[4];         /* finite; the entry of alpha is not read */
    float   white[4];         /* finite, > black */
    float   midtone[4];       /* in (0, 1), read under STK_STRETCH_MTF; 0.5 is the identity */
    float   out_scale;        /* finite; STK_DEPTH_F32 only; default 1 */
} stk_stretch_params;
typedef struct {
    double  shadows_clip;     /* <= 0, in robust sigmas below the median; default -2.8 */
    double  target_background;/* in (0, 1); default 0.25 */
    double  white;            /* finite; the white point of white_mode 0; default 1 */
    double  white_quantile;   /* 0 .. 1; the quantile stk_auto_stretch measures as q[0] under white_mode 2; default 0.999 */
    int32_t linked;           /* 0 (default): per channel, which neutralises the background; 1: one rule for all */
    int32_t white_mode;       /* 0 (default): `white`; 1: the channel's max; 2: the channel's q[0] */
} stk_stretch_auto_params;
/* The image a stretch writes: as stk_image_f32, with a depth. row_stride_bytes: 0 = tightly packed, else at least
 * width * channels * (depth / 8) and a multiple of depth / 8; neither it nor data needs any other alignment. */
typedef struct {
    void*   data;
    int32_t width, height, channels;
    int32_t depth;            /* STK_DEPTH_U8 / U16 / F32 */
    int32_t location;         /* STK_HOST | STK_DEVICE */
    size_t  row_stride_bytes;
} stk_image_out;
/* Step 1. stats: 4 records, one per channel; those from min(channels, 3) on are zeros. quantiles_or_null: n_quantiles
 * values (0 .. 4). stk_timing.finalize_ms is the launches alone; prep_ms the first pass (the counts, min and max and the
 * first digit), warp_ms the second round of the values' selection (one histogram launch and one pick), align_ms the second
 * round of the MAD's. */
stk_status stk_image_stats(stk_ctx* ctx, const stk_image_f32* in, const float* mask_or_null, size_t mask_stride_bytes,
                           int32_t mask_location, const double* quantiles_or_null, int32_t n_quantiles, stk_image_stat* stats);
/* Step 3. table_or_null: knots + 1 floats in host memory, read under STK_STRETCH_TABLE only. finalize_ms is the launch. */
stk_status stk_stretch(stk_ctx* ctx, const stk_image_f32* in, const stk_stretch_params* params, const float* table_or_null,
                       int32_t knots, stk_image_out* out);
/* Step 2 (host code, no context). stats: 4 records as stk_image_stats writes them; channels 1, 3 or 4; params_or_null:
 * null = the defaults. */
stk_status stk_stretch_auto(const stk_image_stat* stats, int32_t channels, const stk_stretch_auto_params* params_or_null,
                            stk_stretch_params* out);
/* A table for STK_STRETCH_TABLE (host code, no context, f64): table: knots + 1 floats, T[k] at x = (double)k / knots:
 * STK_CURVE_ASINH: (float)(asinh(param x) / asinh(param)), param = beta > 0 (10 .. 1000 are usual);
 * STK_CURVE_GAMMA: (float)pow(x, 1 / param), param = gamma > 0;
 * STK_CURVE_SRGB:  x <= 0.0031308 ? 12.92 x : 1.055 pow(x, 1 / 2.4) - 0.055 (param is not read).
 * T[0] = 0 and T[knots] = 1 exactly. knots 2 .. 65536. */
stk_status stk_stretch_table(int32_t kind, double param, int32_t knots, float* table);
/* Steps 1 - 3 in one call: the statistics of `in` (with the mask; the quantile white_quantile under white_mode 2, else
 * none), the rule, then the stretch with the rule's black, white and midtone and this call's curve, colour, out->depth and
 * out_scale. Bit for bit the three parts. stats_out_or_null: 4 records; params_out_or_null: the parameters as used. */
stk_status stk_auto_stretch(stk_ctx* ctx, const stk_image_f32* in, const float* mask_or_null, size_t mask_stride_bytes,
                            int32_t mask_location, const stk_stretch_auto_params* auto_params_or_null, int32_t curve, int32_t colour,
                            float out_scale, const float* table_or_null, int32_t knots, stk_image_out* out,
                            stk_image_stat* stats_out_or_null, stk_stretch_params* params_out_or_null);

/* One frame's whole ECC preparation as ecc_match runs it per frame: cvt_color(BGR2GRAY) (utils.rs:136-142) followed
 * by findTransformECC's own GaussianBlur of the float image (lib.rs:769-777) in one fused pass. `out` is a tightly
 * packed width x height f32 plane in the frame's location. BGR frames, 8-bit or f32. */
stk_status stk_grey_blur_f32(stk_ctx* ctx, const stk_frames* frame /* n==1 */, int32_t ksize, float* out);
/* GaussianBlur(float(grey), g x g, sigma 0, REFLECT_101) as findTransformECC's setup does. */
stk_status stk_gaussian_blur_f32(stk_ctx* ctx, const void* grey, int32_t depth, int32_t width,
                                 int32_t height, int32_t location, int32_t ksize, float* out);
/* video::find_transform_ecc(template, input, warp, motion, criteria, no mask, gauss) lib.rs:769-777.
 * template/input: single-channel u8 (or f32) width x height, tightly packed.
 * warp: 9 floats row-major in/out (2x3 motions use the first 6). rho/iterations optional. */
stk_status stk_find_transform_ecc(stk_ctx* ctx, const void* templ, const void* input,
                                  int32_t depth, int32_t width, int32_t height, int32_t location,
                                  const stk_ecc_params* params, float* warp, double* rho,
                                  int32_t* iterations);
/* Test hooks: what the last ECC preparation on this context left for the iteration kernels. Neither changes what a call
 * launches. Usable after any stk_ecc_match* / stk_hybrid_match* / stk_find_transform_ecc call that got as far as its
 * iterations, whether or not a frame's ECC then failed (the iteration kernels only read these buffers); on a context that
 * has prepared nothing both return STK_INVALID_PARAMS. A multi-device context answers for its first device's shard.
 * stk_ecc_prepared_geometry: size of the planes ECC ran on (the scaled-down size under scale_down_width), the number of
 * moving-frame templates and the width of the zero border around the frame-0 planes.
 * stk_ecc_prepared: drains the context's streams and copies one plane to host memory, tightly packed:
 *   what = STK_PREP_TEMPLATE   template `index` (moving frame index + 1): height x width floats
 *   what = STK_PREP_I / STK_PREP_GX / STK_PREP_GY   blurred frame 0 and its central-difference gradients, WITH the zero
 *          border: (height + 2 pad) x (width + 2 pad) floats
 *   what = STK_PREP_GXY / STK_PREP_IGG   the interleaved (gx, gy) and (I, gx, gy) copies, with the border: 2 and 3 floats per pixel
 * (`index` is ignored for the frame-0 planes.) capacity_floats below the plane's size: STK_INVALID_PARAMS. */
enum { STK_PREP_TEMPLATE = 0, STK_PREP_I = 1, STK_PREP_GX = 2, STK_PREP_GY = 3, STK_PREP_GXY = 4, STK_PREP_IGG = 5 };
stk_status stk_ecc_prepared_geometry(const stk_ctx* ctx, int32_t* width, int32_t* height, int32_t* n_templates, int32_t* pad);
stk_status stk_ecc_prepared(stk_ctx* ctx, int32_t what, int32_t index, float* out_host, size_t capacity_floats);
/* imgproc::warp_perspective / warp_affine (INTER_LINEAR, no WARP_INVERSE_MAP: M is inverted)
 * of convert(frame, 1/255)  fused with  acc += warped   (lib.rs:290-316, 780-814).
 * M: 9 doubles row-major (affine: last row 0 0 1). acc: device or host f32 w*h*c.
 * If accumulate == 0 the warped image overwrites acc. alpha is the convert scale. */
stk_status stk_warp_accumulate(stk_ctx* ctx, const stk_frames* frame /* n==1 */, const double* M,
                               int32_t is_affine, int32_t border_mode, const double* border_value,
                               double alpha, int32_t accumulate, stk_image_f32* acc);

/* scale_image (utils.rs:186-214) on an 8-bit grey image: aspect-preserving resize(INTER_AREA) so that the
 * SMALLER dimension becomes scale_down: new_w = (int)(w * f), new_h = (int)(h * f), f = scale_down / min(w, h). out must hold
 * new_w * new_h bytes — more than width * height when scale_down exceeds the smaller dimension (the image is then enlarged,
 * as the reference does for a landscape frame with height < scale_down < width: INTER_AREA's bilinear emulation). */
stk_status stk_scale_image_grey(stk_ctx* ctx, const uint8_t* grey, int32_t width, int32_t height, int32_t location,
                                float scale_down, uint8_t* out, int32_t* new_width, int32_t* new_height);
/* The same on a 32FC1 grey (the grey of a float stack, e.g. float TIFF: ecc_match_scaling_down shrinks whatever depth cvtColor
 * gave it, lib.rs:896, 921; 16-bit greys never get that far — findTransformECC and ORB reject them first). */
stk_status stk_scale_image_grey_f32(stk_ctx* ctx, const float* grey, int32_t width, int32_t height, int32_t location,
                                    float scale_down, float* out, int32_t* new_width, int32_t* new_height);

/* ORB::create_def + detect_and_compute, utils.rs:174-183. keypoints: rows of 7 floats
 * {x, y, size, angle, response, octave, class_id}; descriptors: rows of 32 bytes. */
stk_status stk_orb_detect_and_compute(stk_ctx* ctx, const uint8_t* grey, int32_t width,
                                      int32_t height, int32_t location, int32_t max_keypoints,
                                      float* keypoints, uint8_t* descriptors, int32_t* n_keypoints);
/* BFMatcher(NORM_HAMMING).knn_match(query, k=2) lib.rs:208-219. out rows {train0, dist0, train1, dist1}
 * (-1 where the train set has fewer than 2 rows). Host pointers. */
stk_status stk_bf_knn2_hamming(stk_ctx* ctx, const uint8_t* query, int32_t n_query,
                               const uint8_t* train, int32_t n_train, int32_t* out);
/* calib3d::find_homography(src_pts, dst_pts, mask, method, thr) lib.rs:267-276. Points are host
 * float pairs. H: 9 doubles; *found = 0 when OpenCV would return an empty Mat. */
stk_status stk_find_homography(stk_ctx* ctx, const float* src_pts, const float* dst_pts, int32_t n,
                               int32_t method, double ransac_reproj_threshold, double* H,
                               uint8_t* inlier_mask_or_null, int32_t* found);

/* stk_find_homography for `count` independent problems in one call: the batch the keypoint path and star registration
 * hand to the engine (every round's models of every problem in one launch, every problem's refinement in one launch).
 * Problem i of a batch returns the bits that problem returns alone. Host pointers; points are n x 2 float pairs. */
typedef struct {
    const float* src_pts;
    const float* dst_pts;
    int32_t n;
    uint8_t* inlier_mask_or_null;   /* n bytes: 1 inlier, 0 outlier; all 0 when nothing is found or rc != 0 */
} stk_hg_problem;
typedef struct {
    int32_t rc;                     /* 0: see found; 3: arguments findHomography rejects (n < 4, unknown method); 7: RHO */
    int32_t found;                  /* 0 when OpenCV would return an empty Mat */
    double  H[9];                   /* row-major, H[8] == 1 when found, else zeros */
    int32_t n_inliers;              /* points the final fit ran over (0 when nothing is found) */
    int32_t models_evaluated;       /* 4-point models scored for this problem: 0 for method 0, n == 4 and a problem
                                     * without an admissible sample. RANSAC: up to the end of the round (32, 288, 2000
                                     * models) in which its adaptive iteration count was reached; LMEDS: its fixed count */
} stk_hg_outcome;
/* Per-problem errors are reported in outcomes[i].rc and do not fail the call. count <= 0: STK_OK, nothing written. A null
 * problems or outcomes, or a problem with n > 0 and a null point list: STK_INVALID_PARAMS. A problem of more than 4096
 * points: STK_NOT_IMPLEMENTED for the whole call. ransac_reproj_threshold <= 0 means 3, as in findHomography. */
stk_status stk_find_homography_batch(stk_ctx* ctx, const stk_hg_problem* problems, int32_t count, int32_t method,
                                     double ransac_reproj_threshold, stk_hg_outcome* outcomes);

#ifdef __cplusplus
}
#endif
#endif /* STACKER_H */
