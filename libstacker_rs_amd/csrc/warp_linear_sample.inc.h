// warp_linear_sample.inc.h — a FRAGMENT of a kernel body, included after warp_coords.inc.h: the bilinear sample of every
// channel of table entry `fr` at (ix + ax, iy + ay), border mode and value included. The linear generic kernel's whole
// sample, and the cubic kernels' sample wherever their footprint test fails: one text, so they agree bit for bit.
// The including scope provides exactly these names:
//   T, CN          the sample type and the channel count
//   a, fr, src     the WarpArgs, the table entry and its frame as const T*
//   mode           the border mode
//   ix, iy, ax, ay, finite, w00, w01, w10, w11     warp_coords.inc.h's results (or their like: the classic weights are read
//                  only where STK_SUBPIX != 0)
//   STK_SUBPIX     the subpixel mode, as for warp_coords.inc.h
//   cs             the state. Its type decides what it is handed besides the samples: cs.entry(kappa) if it declares
//                  wants_kappa, cs.coords(..) if wants_coords (FoldTraits, warp_body.h)
//   STK_SAMPLE(c, v)   what becomes of channel c's sample v: a hook of cs, or the mean's running sum
        int x0 = border_interp(ix, a.sw, mode), x1 = border_interp(ix + 1, a.sw, mode);
        int y0 = border_interp(iy, a.sh, mode), y1 = border_interp(iy + 1, a.sh, mode);
        if (!finite) { x0 = x1 = y0 = y1 = (mode == STK_BORDER_CONSTANT) ? -1 : 0; }
        const bool v00 = (x0 >= 0) & (y0 >= 0), v01 = (x1 >= 0) & (y0 >= 0);
        const bool v10 = (x0 >= 0) & (y1 >= 0), v11 = (x1 >= 0) & (y1 >= 0);
        // clamped addresses keep every load in bounds; out-of-image taps are replaced afterwards
        const int cx0 = max(x0, 0), cx1 = max(x1, 0), cy0 = max(y0, 0), cy1 = max(y1, 0);
        const T* r0 = src + (size_t)cy0 * a.src_stride;
        const T* r1 = src + (size_t)cy1 * a.src_stride;
        if constexpr (decltype(cs)::wants_kappa) {
            // kappa from the taps that are inside the frame (the BORDER_CONSTANT validity, whatever the fold's border mode)
            const bool ix0 = (unsigned)ix < (unsigned)a.sw, ix1 = (unsigned)(ix + 1) < (unsigned)a.sw;
            const bool iy0 = (unsigned)iy < (unsigned)a.sh, iy1 = (unsigned)(iy + 1) < (unsigned)a.sh;
            cs.entry(fold_kappa(ix0 & iy0, ix1 & iy0, ix0 & iy1, ix1 & iy1, STK_SUBPIX != 0, ax, ay, w00, w01, w10, w11));
        }
        // the local mode samples its weight plane at the same coordinates
        if constexpr (decltype(cs)::wants_coords) cs.coords(ix, iy, ax, ay, finite, STK_SUBPIX != 0, w00, w01, w10, w11, a.sw, a.sh);
#pragma unroll
        for (int c = 0; c < CN; c++) {
            const float p00 = v00 ? (float)r0[cx0 * CN + c] * a.alpha : a.bv[c];
            const float p01 = v01 ? (float)r0[cx1 * CN + c] * a.alpha : a.bv[c];
            const float p10 = v10 ? (float)r1[cx0 * CN + c] * a.alpha : a.bv[c];
            const float p11 = v11 ? (float)r1[cx1 * CN + c] * a.alpha : a.bv[c];
            float v;
            if (STK_SUBPIX == 0) {
                const float t0 = __builtin_fmaf(ax, p01 - p00, p00);
                const float t1 = __builtin_fmaf(ax, p11 - p10, p10);
                v = __builtin_fmaf(ay, t1 - t0, t0);
            } else {
                v = p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11;
            }
            STK_SAMPLE(c, v);
        }
