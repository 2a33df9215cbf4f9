// dwt53_plane_wg.inc -- one level of the 5-3 transform of SINGLE-COMPONENT planes in workgroup form (included by dwt53.hip,
// inside namespace j2k).  Same idea as dwt53_l0pix.inc -- a wave = one pair-row, all its loads in flight at once, vertical
// neighbours through LDS, no marching -- for the planes the packed-RGBA8 kernels do not cover: every level > 0 (always single
// components: dwt.go:524-531 transforms the contiguous prefix of each component on its own), level 0 of one-component frames
// (int32 planes or packed Gray16 pixels, encoder.go:94-105), any width: a plane wider than 512 columns is cut into strips of
// 512, and a strip's first / last lane fetch the two samples to their left / the one to their right themselves (the
// horizontal 5-3 of a pair looks one even sample to the right, dwt.go:84-95, and one high-pass value to the left, :99-110).
// The marching kernels these replace are latency-bound on such planes (a 1024 x 1024 level: 8.8 us for 8 MB): few long
// waves, load -> use -> store per step.  Arithmetic wraps like Go's int32 (coefficients of deeper levels are arbitrary).
//
// Geometry contract (checked by the plan): w % 8 == 0, w >= 16, h >= 2, 16-byte aligned rows.  Everything else keeps the
// general kernels.

typedef unsigned int u4w __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4i wadd4(const v4i &a, const v4i &b) { return (v4i)((u4w)a + (u4w)b); }
__device__ __forceinline__ v4i wsub4(const v4i &a, const v4i &b) { return (v4i)((u4w)a - (u4w)b); }

// NC: 1 = a single component (any level); 3 = level 0 of an RGB triple with DC shift + forward RCT (mct.go:28-40, 96-101) ahead of
// the lifting -- the planar twin of dwt53_fwd_rgba8_wg_kernel, wrap-exact for any precision.
// SRC: where level 0 reads its samples (encoder.extractImageData, encoder.go:79-179, without the int32 staging frame):
//   0 = int32 planes (source row stride P.src_stride);
//   1 = image.Gray16.Pix (one 16-bit sample per pixel, high byte first);      2 = image.Gray.Pix (one byte per pixel);
//   3 = a byte of a four-byte pixel (image.RGBA / NRGBA: channel = the plane's component index -- NRGBA's alpha, or any
//       component of a frame coded without the colour transform);
//   4 = a 16-bit sample of an eight-byte pixel (image.RGBA64 / NRGBA64, high byte first); with NC = 3 channels 0, 1, 2.
// pix_stride = the frame's row stride in PIXELS, comp_elems = W * H of the frame (src_off = component * comp_elems + y0 * W + x0).
// MULTI: the plane has more than one 512-column strip.
// MAL: a level of a Mallat plan (DwtPlane::coef_stride): half-rows are routed as fwd_store_row<MAL> / inv_load_row<MAL> route them -- LL (the
// low half of a low-pass row, while n_next != 0) <-> the dense (w/2) x ceil(h/2) scratch of the next level, every other half-row <-> the
// coefficient plane at row * coef_stride + column.  Wave-uniform per half-row like the prefix test; coef_stride % 4 == 0 (the plan's check).
template <int SRC> struct PixSrc { static constexpr int PB = SRC == 1 ? 2 : SRC == 2 ? 1 : SRC == 3 ? 4 : 8, SB = (SRC == 1 || SRC == 4) ? 2 : 1; };
__device__ __forceinline__ uint32_t bswap16(uint32_t v) { return ((v & 0xFF) << 8) | ((v >> 8) & 0xFF); }
template <int NW, int NC, int SRC, bool MULTI, int WPE, bool MAL = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt53_fwd_plane_wg_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes,
                               const void *__restrict__ src, int32_t *__restrict__ out, int32_t *__restrict__ nxt, int dc_shift,
                               int pix_stride, int64_t comp_elems) {
    static_assert(NC == 1 || (NC == 3 && (SRC == 0 || SRC == 4)), "pixel triples: RGBA64 here, RGBA8 in dwt53_l0pix.inc");
    constexpr int NR = NW - 1;                     // regular waves = pair-rows per workgroup; the last wave is the helper
    constexpr int NV = 2 * NC;                     // vectors per row: L part, H part of every component
    __shared__ v4i slot[NW][NV][64];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;                     // padding entry of the XCD-aware job order
    const DwtPlane P = planes[job.plane];
    const int w = P.w, h = P.h, halfH = (h + 1) >> 1, halfW = w >> 1;
    const int c = job.col0 + lane * 8;
    const bool active = c < w;
    const bool row_end = c + 8 >= w;               // my last pair is the row's last: its right neighbour mirrors (dwt.go:89-95)
    const int cc = active ? c : job.col0;          // idle lanes load a valid address
    const int q0 = job.prow0;
    const bool helper = wv == NR;
    const int q = q0 + wv;
    const bool live = !helper && q < halfH;

    // packed pixels: which channel this plane is and where its tile starts in the frame
    int comp = 0;
    const uint8_t *pix0 = nullptr;
    if constexpr (SRC != 0) {
        comp = (int)(P.src_off[0] / comp_elems);                        // (NC = 3: the triple starts at component 0)
        const int64_t rem = P.src_off[0] - comp * comp_elems, y0 = rem / P.src_stride, x0 = rem - y0 * P.src_stride;
        pix0 = reinterpret_cast<const uint8_t *>(src) + (y0 * (int64_t)pix_stride + x0) * PixSrc<SRC>::PB;
    }
    struct Row { unsigned x[NC][8]; unsigned xm2[NC], xm1[NC], xp8[NC]; };
    auto load_row = [&](int r, Row &R) {
        r = min(max(r, 0), h - 1);
        if constexpr (SRC == 0) {
#pragma unroll
            for (int k = 0; k < NC; k++) {
                const int32_t *p = reinterpret_cast<const int32_t *>(src) + P.src_off[k] + (int64_t)r * P.src_stride;
                const int4 a = *reinterpret_cast<const int4 *>(p + cc), b = *reinterpret_cast<const int4 *>(p + cc + 4);
                R.x[k][0] = a.x; R.x[k][1] = a.y; R.x[k][2] = a.z; R.x[k][3] = a.w; R.x[k][4] = b.x; R.x[k][5] = b.y; R.x[k][6] = b.z; R.x[k][7] = b.w;
                R.xm2[k] = R.xm1[k] = R.xp8[k] = 0;
                if constexpr (MULTI) {
                    if (lane == 0 && c > 0) { R.xm2[k] = p[c - 2]; R.xm1[k] = p[c - 1]; }
                    if (lane == 63 && !row_end) R.xp8[k] = p[c + 8];
                }
            }
        } else {
            constexpr int PB = PixSrc<SRC>::PB;
            const uint8_t *p = pix0 + (int64_t)r * pix_stride * PB;     // the tile's row r
            uint32_t dw[2 * PB];                                        // my eight pixels
            if constexpr (PB == 1) { const uint2 a = *reinterpret_cast<const uint2 *>(p + cc); dw[0] = a.x; dw[1] = a.y; }
            else {
#pragma unroll
                for (int i = 0; i < PB / 2; i++) {
                    const uint4 a = *reinterpret_cast<const uint4 *>(p + (int64_t)cc * PB + 16 * i);
                    dw[4 * i] = a.x; dw[4 * i + 1] = a.y; dw[4 * i + 2] = a.z; dw[4 * i + 3] = a.w;
                }
            }
            // sample of channel ch of pixel i of those eight
            auto smp = [&](int i, int ch) -> unsigned {
                if constexpr (SRC == 2) return (dw[i >> 2] >> (8 * (i & 3))) & 0xFF;
                else if constexpr (SRC == 1) return bswap16(dw[i >> 1] >> (16 * (i & 1)));
                else if constexpr (SRC == 3) return (dw[i] >> (8 * ch)) & 0xFF;
                else return bswap16(((ch & 2) ? dw[2 * i + 1] : dw[2 * i]) >> (16 * (ch & 1)));      // (no dynamic index: the array stays in registers)
            };
            auto px = [&](int col, int ch) -> unsigned {                // one sample by itself (strip boundaries)
                const uint8_t *q = p + (int64_t)col * PB + ch * PixSrc<SRC>::SB;
                if constexpr (PixSrc<SRC>::SB == 1) return q[0]; else return (unsigned)q[0] << 8 | q[1];
            };
#pragma unroll
            for (int k = 0; k < NC; k++) {
                const int ch = NC == 3 ? k : comp;
#pragma unroll
                for (int i = 0; i < 8; i++) R.x[k][i] = smp(i, ch);
                R.xm2[k] = R.xm1[k] = R.xp8[k] = 0;
                if constexpr (MULTI) {
                    if (lane == 0 && c > 0) { R.xm2[k] = px(c - 2, ch); R.xm1[k] = px(c - 1, ch); }
                    if (lane == 63 && !row_end) R.xp8[k] = px(c + 8, ch);
                }
            }
        }
        // DC shift (mct.go:96-101; dc_shift = 0 above level 0), then the forward RCT of a triple (mct.go:28-40)
        auto pre = [&](unsigned (&v)[NC]) {
#pragma unroll
            for (int k = 0; k < NC; k++) v[k] -= (unsigned)dc_shift;
            if constexpr (NC == 3) {
                const unsigned r_ = v[0], g_ = v[1], b_ = v[2];
                v[0] = (unsigned)((int)(r_ + 2u * g_ + b_) >> 2);
                v[1] = b_ - g_;
                v[2] = r_ - g_;
            }
        };
#pragma unroll
        for (int i = 0; i < 8; i++) {
            unsigned v[NC];
#pragma unroll
            for (int k = 0; k < NC; k++) v[k] = R.x[k][i];
            pre(v);
#pragma unroll
            for (int k = 0; k < NC; k++) R.x[k][i] = v[k];
        }
        if constexpr (MULTI) { pre(R.xm2); pre(R.xm1); pre(R.xp8); }
    };
    // the horizontal 5-3 of one row across the wave: v[2k] = L part, v[2k + 1] = H part of component k
    auto hrow = [&](const Row &R, v4i (&v)[NV]) {
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const unsigned (&x)[8] = R.x[k];
            unsigned er = (unsigned)__builtin_amdgcn_update_dpp((int)x[6], (int)x[0], 0x130, 0xf, 0xf, false);   // x[0] of lane + 1
            if (MULTI && lane == 63) er = R.xp8[k];
            unsigned d[4];
#pragma unroll
            for (int j = 0; j < 4; j++) d[j] = x[2 * j + 1] - (unsigned)((int)(x[2 * j] + (j < 3 ? x[2 * j + 2] : er)) >> 1);
            if (row_end) d[3] = x[7] - x[6];       // the row's last odd sample: data[n-1] -= data[n-2] (dwt.go:93-95), exact under wraparound
            unsigned dl = (unsigned)__builtin_amdgcn_update_dpp((int)d[0], (int)d[3], 0x138, 0xf, 0xf, false);    // d[3] of lane - 1; lane 0: d[0]
            if (MULTI && lane == 0 && c > 0) dl = R.xm1[k] - (unsigned)((int)(R.xm2[k] + x[0]) >> 1);            // last high-pass value of the strip to the left
#pragma unroll
            for (int j = 0; j < 4; j++) v[2 * k][j] = (int)(x[2 * j] + (unsigned)((int)((j > 0 ? d[j - 1] : dl) + d[j] + 2u) >> 2));
            v[2 * k + 1] = (v4i){(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
        }
    };
    // n_next = (w/2) * h_next is a multiple of w/2: "this half-row lies past the prefix that feeds the next level" is wave-uniform
    auto store_row = [&](int ro, const v4i (&v)[NV]) {
        if (!active) return;
        if constexpr (MAL) {
            const bool ll = P.n_next != 0 && ro < halfH;
            const int64_t offP = (int64_t)ro * P.coef_stride + (c >> 1), offL = ll ? (int64_t)ro * halfW + (c >> 1) : offP;
#pragma unroll
            for (int k = 0; k < NC; k++) {
                if (ll) *reinterpret_cast<v4i *>(nxt + P.nxt_off[k] + offL) = v[2 * k];
                else st_final<1>(reinterpret_cast<v4i *>(out + P.out_off[k] + offL), v[2 * k]);
                st_final<1>(reinterpret_cast<v4i *>(out + P.out_off[k] + offP + halfW), v[2 * k + 1]);
            }
            return;
        }
        const int64_t idxL = (int64_t)ro * w + (c >> 1), idxH = idxL + halfW;
        const bool finL = (int64_t)ro * w >= P.n_next, finH = (int64_t)ro * w + halfW >= P.n_next;
#pragma unroll
        for (int k = 0; k < NC; k++) {
            if (finL) st_final<1>(reinterpret_cast<v4i *>(out + P.out_off[k] + idxL), v[2 * k]);
            else *reinterpret_cast<v4i *>(nxt + P.nxt_off[k] + idxL) = v[2 * k];
            if (finH) st_final<1>(reinterpret_cast<v4i *>(out + P.out_off[k] + idxH), v[2 * k + 1]);
            else *reinterpret_cast<v4i *>(nxt + P.nxt_off[k] + idxH) = v[2 * k + 1];
        }
    };
    const v4i two = {2, 2, 2, 2};

    v4i E[NV], O[NV];
    if (helper) {
        // rows 2*q0-2, 2*q0-1 (pair-row above the band) and 2*(q0+NR) (even row below it)
        {
            Row n;
            load_row(2 * (q0 + NR), n);
            v4i N[NV];
            hrow(n, N);
#pragma unroll
            for (int v = 0; v < NV; v++) slot[NR][v][lane] = N[v];
        }
        Row a, b;
        load_row(2 * q0 - 2, a); load_row(2 * q0 - 1, b);
        hrow(a, E);
        hrow(b, O);
    } else if (live) {
        Row a, b;
        load_row(2 * q, a); load_row(2 * q + 1, b);
        hrow(a, E);
#pragma unroll
        for (int v = 0; v < NV; v++) slot[wv][v][lane] = E[v];
        hrow(b, O);
    }
    __syncthreads();
    const bool has_odd = 2 * q + 1 < h, has_next = 2 * q + 2 < h;
    if (helper) {
        // d of the pair-row above the band: needs E of the band's first pair-row (slot 0), then recycles that slot
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const v4i En = slot[0][v][lane];
            slot[0][v][lane] = wsub4(O[v], wadd4(E[v], En) >> 1);
        }
    } else if (live && has_odd) {
#pragma unroll
        for (int v = 0; v < NV; v++) {
            if (has_next) O[v] = wsub4(O[v], wadd4(E[v], slot[wv + 1][v][lane]) >> 1);      // O becomes d
            else O[v] = wsub4(O[v], E[v]);
        }
        if (wv + 1 < NR) {
#pragma unroll
            for (int v = 0; v < NV; v++) slot[wv + 1][v][lane] = O[v];
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int v = 0; v < NV; v++) {
            v4i Dp = slot[wv][v][lane];
            if (!has_odd) O[v] = Dp;                             // odd height, last even row: its d mirrors d[n-2] (dwt.go:112-114)
            if (q == 0) Dp = O[v];                               // d[-1] mirrors d[0] (dwt.go:99)
            E[v] = wadd4(E[v], wadd4(wadd4(Dp, O[v]), two) >> 2);
        }
        store_row(q, E);
        if (has_odd) store_row(halfH + q, O);
    }
}

// ================================================================================================================
// Inverse counterpart: one level of ReconstructMultiLevel53 (dwt.go:534-548) = Inverse2D53 (dwt.go:410-429: columns first,
// then rows) for single-component planes; at the final level + mct.DCLevelShiftInverse (mct.go:113-118) and, DST = 1,
// decoder.createImage's 16-bit gray branch straight to packed Gray16 pixels (decoder.go:434-451).
// Wave i owns pair-row q = q0 + i: loads its low-pass row s_q and high-pass row d_q (elements below n_next from the coarser
// level's output `prev`, the rest from the coefficient plane), exchanges d, then e, through LDS exactly as
// dwt53_inv_rgba8_wg_kernel does, and runs the horizontal inverse on rows e_q, o_q across the wave.  In a plane of several
// strips the horizontal step of a strip's first pair needs the high-pass value to its left and that of its last pair the
// reconstructed even sample to its right (= low- and high-pass value there): the boundary lanes carry those three extra
// columns through the whole vertical pipeline as a third vector.
// ================================================================================================================
// NC = 3: level 0 of an RGB triple, inverse RCT (mct.go:56-66) + DC shift to three int32 planes (the planar twin of
// dwt53_inv_rgba8_wg_kernel).
template <int NW, int NC, int DST, bool MULTI, int WPE, bool MAL = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt53_inv_plane_wg_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes,
                               const int32_t *__restrict__ coef, const int32_t *__restrict__ prev, void *__restrict__ dst,
                               int dc_shift, int final_level, int pix_stride, int64_t comp_elems, const int *__restrict__ guard) {
    if (guard && *guard) return;             // (the frame decoder: a stream that was refused leaves the caller's frame alone)
    static_assert(NC == 1 || (NC == 3 && (DST == 0 || DST == 4)), "pixel triples: RGBA64 here, RGBA8 in dwt53_l0pix.inc");
    constexpr int NR = NW - 1;
    constexpr int NV = (MULTI ? 3 : 2) * NC;       // vectors per row: per component L part, H part [, boundary extras {h[-1], l[+4], h[+4], -}]
    constexpr int XV = 2 * NC;                     // index of the first extras vector
    __shared__ v4i slot[NW][NV][64];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    const DwtPlane P = planes[job.plane];
    const int w = P.w, h = P.h, halfH = (h + 1) >> 1, halfW = w >> 1, nhigh = h - halfH;
    const int c = job.col0 + lane * 8;
    const bool active = c < w;
    const bool row_end = c + 8 >= w;
    const int p4 = (active ? c : job.col0) >> 1;   // my four elements of a half-row
    const int q0 = job.prow0;
    const bool helper = wv == NR;
    const int q = q0 + wv;
    const bool live = !helper && q < halfH;
    const v4i two = {2, 2, 2, 2};
    // row `ro` of the level matrix; elements below n_next come from prev (uniform per half-row: n_next % (w/2) == 0)
    auto load_row = [&](int ro, v4i (&v)[NV]) {
        const int64_t rowL = (int64_t)ro * w, rowH = rowL + halfW;
        const bool ll = MAL && P.n_next != 0 && ro < halfH;                 // MAL: bl, bh = where the two half-rows start
        const int64_t rowP = MAL ? (int64_t)ro * P.coef_stride : 0;
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const int32_t *bl = MAL ? (ll ? prev + P.nxt_off[k] + (int64_t)ro * halfW : coef + P.src_off[k] + rowP)
                                    : (rowL >= P.n_next ? coef + P.src_off[k] : prev + P.nxt_off[k]) + rowL;
            const int32_t *bh = MAL ? coef + P.src_off[k] + rowP + halfW
                                    : (rowH >= P.n_next ? coef + P.src_off[k] : prev + P.nxt_off[k]) + rowH;
            v[2 * k] = *reinterpret_cast<const v4i *>(bl + p4);
            v[2 * k + 1] = *reinterpret_cast<const v4i *>(bh + p4);
            if constexpr (MULTI) {
                v4i x = {0, 0, 0, 0};
                if (lane == 0 && c > 0) x[0] = bh[p4 - 1];
                if (lane == 63 && !row_end) { x[1] = bl[p4 + 4]; x[2] = bh[p4 + 4]; }
                v[XV + k] = x;
            }
        }
    };
    v4i S[NV], D[NV];
    if (helper) {
        // d of the pair-row above the band -> slot[0]; s, d of the pair-row below it stay in registers for phase 2
        {
            v4i Da[NV];
            load_row(halfH + min(max(q0 - 1, 0), max(nhigh - 1, 0)), Da);
#pragma unroll
            for (int v = 0; v < NV; v++) slot[0][v][lane] = Da[v];
        }
        asm volatile("" ::: "memory");
        load_row(min(q0 + NR, halfH - 1), S);
        load_row(halfH + min(q0 + NR, max(nhigh - 1, 0)), D);
    } else if (live) {
        load_row(q, S);
        load_row(halfH + min(q, max(nhigh - 1, 0)), D);      // odd height: the last pair-row has no d row (clamped, unused)
#pragma unroll
        for (int v = 0; v < NV; v++) slot[wv + 1][v][lane] = D[v];
    }
    __syncthreads();
    // undo update (dwt.go:132-138): e_q = s_q - ((d_{q-1} + d_q + 2) >> 2); d_{-1} := d_0; no d_q (odd height, last row) := d_{q-1}
    const int qq = helper ? q0 + NR : q;
    if ((helper && qq < halfH) || live) {
        const int sl = helper ? NR : wv;
        const bool has_d = qq < nhigh;
#pragma unroll
        for (int v = 0; v < NV; v++) {
            v4i Dp = slot[sl][v][lane];
            const v4i Dc = has_d ? D[v] : Dp;
            if (qq == 0) Dp = Dc;
            S[v] = wsub4(S[v], wadd4(wadd4(Dp, Dc), two) >> 2);      // S becomes e
            slot[sl][v][lane] = S[v];
        }
    }
    __syncthreads();
    if (!live) return;
    {
        // undo predict (dwt.go:141-146): o_q = d_q + ((e_q + e_{q+1}) >> 1); no e_{q+1}: o_q = d_q + e_q
        const bool has_next = q + 1 < halfH;
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const v4i En = has_next ? slot[wv + 1][v][lane] : S[v];
            D[v] = wadd4(D[v], has_next ? wadd4(S[v], En) >> 1 : S[v]);   // D becomes o
        }
    }
    // horizontal inverse of one row (dwt.go:122-147 across the wave) [+ inverse RCT] + DC shift at the final level, stored
    // as int32 or Gray16
    auto finish_row = [&](int r, const v4i (&v)[NV]) {
        unsigned x[NC][8];
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const v4i lo = v[2 * k], hi = v[2 * k + 1];
            unsigned dleft = (unsigned)__builtin_amdgcn_update_dpp(hi[0], hi[3], 0x138, 0xf, 0xf, false);   // lane 0 keeps d[0]: d[-1] := d[0]
            if (MULTI && lane == 0 && c > 0) dleft = (unsigned)v[MULTI ? XV + k : 0][0];
            unsigned e[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                e[j] = (unsigned)lo[j] - (unsigned)((int)((j > 0 ? (unsigned)hi[j - 1] : dleft) + (unsigned)hi[j] + 2u) >> 2);
            unsigned eright = (unsigned)__builtin_amdgcn_update_dpp((int)e[3], (int)e[0], 0x130, 0xf, 0xf, false);
            if (MULTI && lane == 63 && !row_end)        // the even sample that opens the strip to the right
                eright = (unsigned)v[MULTI ? XV + k : 0][1] - (unsigned)((int)((unsigned)hi[3] + (unsigned)v[MULTI ? XV + k : 0][2] + 2u) >> 2);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned en = j < 3 ? e[j + 1] : eright;
                unsigned pred = (unsigned)((int)(e[j] + en) >> 1);
                if (j == 3 && row_end) pred = e[3];                      // last odd sample of an even-length row: += data[n-2]
                x[k][2 * j] = e[j];
                x[k][2 * j + 1] = (unsigned)hi[j] + pred;
            }
        }
        if constexpr (NC == 3) {                                         // mct.go:56-66
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const unsigned y_ = x[0][i], u_ = x[1][i], v_ = x[2][i];
                const unsigned g_ = y_ - (unsigned)((int)(u_ + v_) >> 2);
                x[0][i] = v_ + g_; x[1][i] = g_; x[2][i] = u_ + g_;
            }
        }
        if (!active) return;
        if constexpr (DST != 0) {
            // decoder.createImage (decoder.go:417-588) at the format's own precision, without the int32 frame in between:
            // 8 bit: clamp to 0..255; 16 bit: clamp to 0..65535, then the reference's rescale v * 65535 / 65535 in int32 (it wraps
            // for v >= 32769) and uint16() of that, high byte first.  DST as SRC of the forward kernel; NC = 3 writes whole
            // RGBA64 pixels with alpha 65535 (decoder.go:504-528), a single component of a four-channel pixel only its own bytes
            // (the triple's launch comes first: decoder.go:531-585 takes alpha from component 3).
            constexpr int PB = PixSrc<DST>::PB;
            const int comp = (int)(P.out_off[0] / comp_elems);
            const int64_t rem = P.out_off[0] - comp * comp_elems, y0 = rem / P.out_stride, x0 = rem - y0 * P.out_stride;
            uint8_t *p = reinterpret_cast<uint8_t *>(dst) + ((y0 + r) * (int64_t)pix_stride + x0 + c) * PB;
            auto pix8 = [&](unsigned v) -> uint32_t { return (uint32_t)min(max((int)(v + (unsigned)dc_shift), 0), 255); };
            auto pix16 = [&](unsigned v) -> uint32_t {                  // (bytes already swapped)
                const int a0 = min(max((int)(v + (unsigned)dc_shift), 0), 65535);
                return bswap16((uint32_t)((int)((uint32_t)a0 * 65535u) / 65535) & 0xFFFFu);
            };
            if constexpr (DST == 1) {
                uint32_t dw[4];
#pragma unroll
                for (int i = 0; i < 4; i++) dw[i] = pix16(x[0][2 * i]) | pix16(x[0][2 * i + 1]) << 16;
                const v4i o = {(int)dw[0], (int)dw[1], (int)dw[2], (int)dw[3]};
                __builtin_nontemporal_store(o, reinterpret_cast<v4i *>(p));
            } else if constexpr (DST == 2) {
                uint2 o;
                o.x = pix8(x[0][0]) | pix8(x[0][1]) << 8 | pix8(x[0][2]) << 16 | pix8(x[0][3]) << 24;
                o.y = pix8(x[0][4]) | pix8(x[0][5]) << 8 | pix8(x[0][6]) << 16 | pix8(x[0][7]) << 24;
                *reinterpret_cast<uint2 *>(p) = o;
            } else if constexpr (NC == 1) {
                // one channel of four: read my eight pixels, put my samples in, write them back whole (16-byte accesses; eight
                // strided one- or two-byte stores per lane cost twice the time).  NOT atomic: correct only while no other plane of the
                // same launch writes the same pixels -- the host takes this kernel for ONE single-component plane per pixel, the alpha
                // plane beside an MCT triple whose launch ran before (pix_fusable, j2k_stages.cpp).
                v4i o[PB / 2];
#pragma unroll
                for (int i = 0; i < PB / 2; i++) o[i] = *reinterpret_cast<const v4i *>(p + 16 * i);
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    if constexpr (DST == 3) {
                        const uint32_t sh = 8u * (uint32_t)comp;
                        o[i >> 2][i & 3] = (int)(((uint32_t)o[i >> 2][i & 3] & ~(0xFFu << sh)) | pix8(x[0][i]) << sh);
                    } else {
                        const uint32_t sh = 16u * ((uint32_t)comp & 1u), v = pix16(x[0][i]);
                        const uint32_t lo = (uint32_t)o[i >> 1][2 * (i & 1)], hi = (uint32_t)o[i >> 1][2 * (i & 1) + 1];
                        o[i >> 1][2 * (i & 1)] = (int)((comp & 2) ? lo : ((lo & ~(0xFFFFu << sh)) | v << sh));
                        o[i >> 1][2 * (i & 1) + 1] = (int)((comp & 2) ? ((hi & ~(0xFFFFu << sh)) | v << sh) : hi);
                    }
                }
#pragma unroll
                for (int i = 0; i < PB / 2; i++) *reinterpret_cast<v4i *>(p + 16 * i) = o[i];
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {                           // two pixels per 16-byte store
                    const v4i o = {(int)(pix16(x[0][2 * i]) | pix16(x[1][2 * i]) << 16), (int)(pix16(x[2][2 * i]) | 0xFFFF0000u),
                                   (int)(pix16(x[0][2 * i + 1]) | pix16(x[1][2 * i + 1]) << 16), (int)(pix16(x[2][2 * i + 1]) | 0xFFFF0000u)};
                    *reinterpret_cast<v4i *>(p + 16 * i) = o;
                }
            }
        } else {
            const int stride = final_level ? P.out_stride : w;
#pragma unroll
            for (int k = 0; k < NC; k++) {
                int32_t *p = reinterpret_cast<int32_t *>(dst) + P.out_off[k] + (int64_t)r * stride + c;
                const unsigned dcu = (unsigned)dc_shift;
                *reinterpret_cast<v4i *>(p) = (v4i){(int)(x[k][0] + dcu), (int)(x[k][1] + dcu), (int)(x[k][2] + dcu), (int)(x[k][3] + dcu)};
                *reinterpret_cast<v4i *>(p + 4) = (v4i){(int)(x[k][4] + dcu), (int)(x[k][5] + dcu), (int)(x[k][6] + dcu), (int)(x[k][7] + dcu)};
            }
        }
    };
    finish_row(2 * q, S);
    if (2 * q + 1 < h) finish_row(2 * q + 1, D);
}
