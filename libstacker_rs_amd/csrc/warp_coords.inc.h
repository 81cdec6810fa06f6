// warp_coords.inc.h — a FRAGMENT of a kernel body, included inside the frame loop of the generic fold kernels (warp_body.h,
// warp_cubic_body.h) and of the kernels that only need the coordinates: the source coordinates of destination pixel
// (px, py) = (fx, fy) under table entry `fr`. Leaves ix, iy (floor), ax, ay (fractions), `finite`, and under the classic
// path the four weights w00 .. w11. The including scope provides a, fr, fx, fy, px, py (the last two are read only where
// STK_SUBPIX != 0) and STK_SUBPIX, its subpixel mode (a.subpixel_bits, or the constant 0). One text for every kernel that
// samples: the cubic fold's coordinates are the linear fold's by construction.
        int ix, iy;
        float ax = 0, ay = 0;
        float w00 = 0, w01 = 0, w10 = 0, w11 = 0;
        bool finite = true;
        if (STK_SUBPIX == 0) {
            // OpenCV >= 4.11 kernels: f32 matrix, fma chains, true division, floor, lerp by fma
            float X = __builtin_fmaf(fr->M[0], fx, __builtin_fmaf(fr->M[1], fy, fr->M[2]));
            float Y = __builtin_fmaf(fr->M[3], fx, __builtin_fmaf(fr->M[4], fy, fr->M[5]));
            if (!a.is_affine) {
                const float W = __builtin_fmaf(fr->M[6], fx, __builtin_fmaf(fr->M[7], fy, fr->M[8]));
                X = X / W; Y = Y / W;
            }
            finite = (__builtin_fabsf(X) < 1e9f) & (__builtin_fabsf(Y) < 1e9f);   // false for NaN / inf
            const float flx = __builtin_floorf(X), fly = __builtin_floorf(Y);
            ix = finite ? (int)flx : -100000; iy = finite ? (int)fly : -100000;
            ax = finite ? X - flx : 0.0f; ay = finite ? Y - fly : 0.0f;
        } else {
            // classic remap path: 1/32-pixel quantised coordinates, 4-weight table
            int Xi, Yi;
            const double* M = fr->Md;
            if (a.is_affine) {
                const int adx = sat_int_d(M[0] * px * 1024), bdx = sat_int_d(M[3] * px * 1024);
                const int X0 = sat_int_d((M[1] * py + M[2]) * 1024) + 16;
                const int Y0 = sat_int_d((M[4] * py + M[5]) * 1024) + 16;
                Xi = (X0 + adx) >> 5; Yi = (Y0 + bdx) >> 5;
            } else {
                double W = M[6] * px + M[7] * py + M[8];
                W = W != 0 ? 32.0 / W : 0;
                const double Xd = fmax(-2147483648.0, fmin(2147483647.0, (M[0] * px + M[1] * py + M[2]) * W));
                const double Yd = fmax(-2147483648.0, fmin(2147483647.0, (M[3] * px + M[4] * py + M[5]) * W));
                Xi = sat_int_d(Xd); Yi = sat_int_d(Yd);
            }
            ix = Xi >> 5; iy = Yi >> 5;
            const float qx = (float)(Xi & 31) * (1.f / 32), qy = (float)(Yi & 31) * (1.f / 32);
            const float ux = 1.f - qx, uy = 1.f - qy;
            w00 = uy * ux; w01 = uy * qx; w10 = qy * ux; w11 = qy * qx;
        }
