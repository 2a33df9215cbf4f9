// dwt53_l0pix_fwd_body.inc -- the statements of one workgroup of the packed-RGBA8 level-0 forward transform (see dwt53_l0pix.inc),
// included TEXTUALLY by dwt53_fwd_rgba8_wg_kernel (its own static LDS array) and by dwt53_fwd_rgba8_wg_body (dynamic LDS of
// dwt53_mega_fwd_kernel): as a function call the kernel lost two registers to the inliner's different schedule and spilled.
// Names it expects in scope: NW, NT (template parameters), MAL (a compile-time bool: Mallat routing of the stores, see store_row), S16 (a
// compile-time bool: the rows of X_1 as int16, see store_row; never with MAL), slot
// (v4i [NW][6][64] in LDS), job (DwtJob), planes, pix, out, nxt, dc_shift, pix_stride.

    constexpr int NR = NW - 1;                     // regular waves = pair-rows per workgroup
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const DwtPlane P = planes[job.plane];
    const int w = P.w, h = P.h, halfH = (h + 1) >> 1, halfW = w >> 1;
    const int c = lane * 8;
    const bool active = c < w;
    const bool last_lane = c + 8 >= w;
    const int q0 = job.prow0;
    const bool helper = wv == NR;
    const int q = q0 + wv;                         // regular waves: my pair-row
    const bool live = !helper && q < halfH;
    const int64_t y0 = P.src_off[0] / P.src_stride;
#ifndef J2K_L0_YCC
    const uint32_t *base = pix + y0 * pix_stride + (P.src_off[0] - y0 * P.src_stride) + (active ? c : 0);
    auto rowp = [&](int r) { return reinterpret_cast<const uint4 *>(base + (int64_t)min(max(r, 0), h - 1) * pix_stride); };
#else
    // YCbCr source (dwt53_fwd_ycc_wg_kernel, SRC = 1 + ratio; Rect.Min even and >= 0, so Go's offsets are plain shifts of the
    // frame position): 8 Y bytes and the 4 (4:2:x) or 8 (4:4:4) Cb / Cr bytes of chroma row y >> VS per row, all loads first,
    // then the colours in registers as the packed pixels hrow takes (image_color.h)
    constexpr int HS = SRC == 1 + J2K_YCBCR_444 ? 0 : 1, VS = SRC == 1 + J2K_YCBCR_420 ? 1 : 0;
    const int64_t gx = (P.src_off[0] - y0 * P.src_stride) + (active ? c : 0);      // frame column of my first pixel
    struct YccRaw { uint2 y, cb, cr; };
    auto yload = [&](int r) {
        const int64_t fy = y0 + min(max(r, 0), h - 1), cy = fy >> VS;
        YccRaw o;
        o.y = *reinterpret_cast<const uint2 *>(ycc.y + fy * ycc.ystride + gx);
        if constexpr (HS == 0) {
            o.cb = *reinterpret_cast<const uint2 *>(ycc.cb + cy * ycc.cstride + gx);
            o.cr = *reinterpret_cast<const uint2 *>(ycc.cr + cy * ycc.cstride + gx);
        } else {
            o.cb = make_uint2(*reinterpret_cast<const uint32_t *>(ycc.cb + cy * ycc.cstride + (gx >> 1)), 0u);
            o.cr = make_uint2(*reinterpret_cast<const uint32_t *>(ycc.cr + cy * ycc.cstride + (gx >> 1)), 0u);
        }
        return o;
    };
    auto ycvt = [&](const YccRaw &o, uint4 &a, uint4 &b) {
        uint32_t px[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int ci = i >> HS;
            const int Y = (int)(((i < 4 ? o.y.x : o.y.y) >> (8 * (i & 3))) & 0xFF);
            const int Cb = (int)(((ci < 4 ? o.cb.x : o.cb.y) >> (8 * (ci & 3))) & 0xFF);
            const int Cr = (int)(((ci < 4 ? o.cr.x : o.cr.y) >> (8 * (ci & 3))) & 0xFF);
            px[i] = ycbcr_rgba8(Y, Cb, Cr);
        }
        a = make_uint4(px[0], px[1], px[2], px[3]);
        b = make_uint4(px[4], px[5], px[6], px[7]);
    };
#endif

    // one row, all three components: unpack, RCT on raw bytes, horizontal 5-3 across the wave -> v[k*2] = lo, v[k*2+1] = hi
    auto hrow = [&](const uint4 &a, const uint4 &b, v4i (&v)[6]) {
        const uint32_t px[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            int x[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int R = (int)(px[i] & 0xFF), G = (int)((px[i] >> 8) & 0xFF), B = (int)((px[i] >> 16) & 0xFF);
                x[i] = (k == 0) ? (R + 2 * G + B) >> 2 : (k == 1 ? B - G : R - G);
            }
            int er = __builtin_amdgcn_update_dpp(x[6], x[0], 0x130, 0xf, 0xf, false);   // lane 63 keeps x[6]
            er = last_lane ? x[6] : er;                                                  // mirror at the row end (dwt.go:89-95)
            int d[4];
#pragma unroll
            for (int j = 0; j < 4; j++) d[j] = x[2 * j + 1] - ((x[2 * j] + (j < 3 ? x[2 * j + 2] : er)) >> 1);
            const int dl = __builtin_amdgcn_update_dpp(d[0], d[3], 0x138, 0xf, 0xf, false);   // lane 0 mirrors d[0] (dwt.go:99)
#pragma unroll
            for (int j = 0; j < 4; j++) v[2 * k][j] = x[2 * j] + (((j > 0 ? d[j - 1] : dl) + d[j] + 2) >> 2);
            v[2 * k + 1] = (v4i){d[0], d[1], d[2], d[3]};
        }
    };
    // n_next = (w/2) * h_next is a multiple of w/2, so "this half-row lies past the prefix that feeds level 1" is the same
    // for every lane: wave-uniform branches (a per-lane select would also make the compiler drop the nt flag)
    // MAL (a Mallat plan, DwtPlane::coef_stride): the routing of fwd_store_row<MAL> -- LL (the low half of a low-pass row, while there is a
    // next level) to its dense (w/2) x ceil(h/2) scratch, every other half-row to the plane at row * coef_stride + column; uniform as well
    auto store_row = [&](int ro, const v4i (&v)[6], int ysub) {
        if (!active) return;
        if constexpr (MAL) {
            const bool ll = P.n_next != 0 && ro < halfH;
            const int offP = ro * P.coef_stride + lane * 4, offL = ll ? ro * halfW + lane * 4 : offP;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const v4i vl = (k == 0) ? v[0] - ysub : v[2 * k];
                if (ll) *reinterpret_cast<v4i *>(nxt + P.nxt_off[k] + offL) = vl;
                else st_final<NT>(reinterpret_cast<v4i *>(out + P.out_off[k] + offL), vl);
                st_final<NT>(reinterpret_cast<v4i *>(out + P.out_off[k] + offP + halfW), v[2 * k + 1]);
            }
            return;
        }
        const int idxL = ro * w + lane * 4, idxH = idxL + halfW;
        const bool finL = ro * w >= P.n_next, finH = ro * w + halfW >= P.n_next;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const v4i vl = (k == 0) ? v[0] - ysub : v[2 * k];
            // S16 (dwt53_fwd_rgba8_wg16_kernel): a half-row below n_next -- a row of X_1, read back by the deep launch alone -- goes out
            // as four int16 per lane in the first half of its int32-sized slot (st_scr16: the bound, and why nothing is lost)
            if (finL) {
                v4i *bl = reinterpret_cast<v4i *>(out + P.out_off[k] + idxL);
                st_final<NT>(bl, vl);
            } else if constexpr (S16) {
                st_scr16(nxt + P.nxt_off[k] + idxL - lane * 2, vl);
            } else {
                *reinterpret_cast<v4i *>(nxt + P.nxt_off[k] + idxL) = vl;
            }
            if (finH) {
                v4i *bh = reinterpret_cast<v4i *>(out + P.out_off[k] + idxH);
                st_final<NT>(bh, v[2 * k + 1]);
            } else if constexpr (S16) {
                st_scr16(nxt + P.nxt_off[k] + idxH - lane * 2, v[2 * k + 1]);
            } else {
                *reinterpret_cast<v4i *>(nxt + P.nxt_off[k] + idxH) = v[2 * k + 1];
            }
        }
    };

    v4i E[6], O[6];
    if (helper) {
        // rows 2*q0-2, 2*q0-1 (pair-row above the band) and 2*(q0+NR) (even row below it)
#ifndef J2K_L0_YCC
        const uint4 *p0 = rowp(2 * q0 - 2), *p1 = rowp(2 * q0 - 1), *p2 = rowp(2 * (q0 + NR));
        const uint4 a0 = p0[0], b0 = p0[1], a1 = p1[0], b1 = p1[1], a2 = p2[0], b2 = p2[1];
#else
        const YccRaw r0 = yload(2 * q0 - 2), r1 = yload(2 * q0 - 1), r2 = yload(2 * (q0 + NR));
        uint4 a0, b0, a1, b1, a2, b2;
        ycvt(r0, a0, b0); ycvt(r1, a1, b1); ycvt(r2, a2, b2);
#endif
        v4i B[6];
        hrow(a2, b2, B);
#pragma unroll
        for (int v = 0; v < 6; v++) slot[NR][v][lane] = B[v];
        hrow(a0, b0, E);
        hrow(a1, b1, O);
    } else if (live) {
#ifndef J2K_L0_YCC
        const uint4 *p0 = rowp(2 * q), *p1 = rowp(2 * q + 1);
        const uint4 a0 = p0[0], b0 = p0[1], a1 = p1[0], b1 = p1[1];
#else
        const YccRaw r0 = yload(2 * q), r1 = yload(2 * q + 1);
        uint4 a0, b0, a1, b1;
        ycvt(r0, a0, b0); ycvt(r1, a1, b1);
#endif
        hrow(a0, b0, E);
#pragma unroll
        for (int v = 0; v < 6; v++) slot[wv][v][lane] = E[v];
        hrow(a1, b1, O);
    }
    __syncthreads();
    const bool has_odd = 2 * q + 1 < h, has_next = 2 * q + 2 < h;
    if (helper) {
        // d of the pair-row above the band: needs E of the band's first pair-row (slot 0), then recycles that slot
#pragma unroll
        for (int v = 0; v < 6; v++) {
            const v4i En = slot[0][v][lane];
            slot[0][v][lane] = O[v] - ((E[v] + En) >> 1);
        }
    } else if (live && has_odd) {
        if (has_next) {
#pragma unroll
            for (int v = 0; v < 6; v++) {
                const v4i En = slot[wv + 1][v][lane];
                O[v] = O[v] - ((E[v] + En) >> 1);        // O becomes d
            }
        } else {
#pragma unroll
            for (int v = 0; v < 6; v++) O[v] = O[v] - E[v];
        }
        if (wv + 1 < NR) {
#pragma unroll
            for (int v = 0; v < 6; v++) slot[wv + 1][v][lane] = O[v];
        }
    }
    __syncthreads();
    if (live) {
        v4i Dp[6];
#pragma unroll
        for (int v = 0; v < 6; v++) Dp[v] = slot[wv][v][lane];
        if (!has_odd) {                                  // odd height, last even row: its d mirrors d[n-2] (dwt.go:112-114)
#pragma unroll
            for (int v = 0; v < 6; v++) O[v] = Dp[v];
        }
        if (q == 0) {                                    // d[-1] mirrors d[0] (dwt.go:99)
#pragma unroll
            for (int v = 0; v < 6; v++) Dp[v] = O[v];
        }
#pragma unroll
        for (int v = 0; v < 6; v++) E[v] = E[v] + ((Dp[v] + O[v] + 2) >> 2);
        store_row(q, E, dc_shift);
        if (has_odd) store_row(halfH + q, O, 0);
    }
