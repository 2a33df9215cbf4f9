// dwt97_l0wg_inv.inc -- level 0 of the lossy inverse path for an RGB triple, workgroup form (included by dwt97.hip).
//
// Replaces, fused: the int32 -> float64 copy of tcd.ApplyInverseDWT (tcd.go:428-431), dwt.Inverse2D97 as level 0 of
// ReconstructMultiLevel97 (dwt.go:212-262, 453-473, 566-573), its int32(v + 0.5) (tcd.go:433-435), the decoder's inverse
// ICT with the same rounding (decoder.go:326-339, mct.go:43-53) and mct.DCLevelShiftInverse (mct.go:113-118).
//
// The forward kernel's structure (dwt97_l0wg.inc) run backwards:
//   * one workgroup = one <= 512-column tile x a band of NR = NW - 3 pair-rows, ALL THREE components (the inverse ICT needs
//     them together at the end), one component after the other through the same LDS slots; wave i owns pair-row
//     t = q0 - 1 + i: low row t and high row halfH + t of the level's dense matrix, 8 columns per lane as its two halves
//     (4 + 4).  The loads stay raw until their use and component k + 1's are
//     issued while component k runs (holding all three at once costs a wave per SIMD);
//   * the inverse runs the vertical steps first.  They alternate between the pair-row above (delta, beta) and the one below
//     (gamma, alpha): four LDS exchanges of one row per component, each slot recycled by its only reader:
//       slot[i+1] <- d2_t | barrier | wave i: s1_t = K s2_t - d (d2_t-1 + d2_t)   (d2_t-1 from slot[i]);   slot[i]   <- s1_t
//                           barrier | wave i: d1_t = d2_t - g (s1_t + s1_t+1)     (s1_t+1 from slot[i+1]); slot[i+1] <- d1_t
//                           barrier | wave i: e_t  = s1_t - b (d1_t-1 + d1_t)     (d1_t-1 from slot[i]);   slot[i]   <- e_t
//                           barrier | wave i: o_t  = d1_t - a (e_t + e_t+1)       (e_t+1 from slot[i+1])
//     An output pair-row needs one pair-row above (plus the high row of the one above that, which wave 0 loads itself and
//     parks in LDS before the first barrier) and two below: NW = NR + 3, the outer three waves store nothing;
//   * then per component the horizontal inverse across the wave (DPP, hinv97<8>) on rows 2t and 2t + 1 and int32(v + 0.5);
//     the three components' integers stay in registers for the inverse ICT, whose int32(v + 0.5) + DC shift is stored as
//     two 16-byte pieces per lane, row and component.
//   * Go's int32(float64) (go_int32: 0x80000000 for values past the positive end, where the hardware convert saturates) is kept exact without paying for it per
//     value: the wave converts with v_cvt_i32_f64 and collects "some lane was out of range" in a scalar mask; a wave that saw
//     one (no real image does) redoes that batch of conversions with go_int32.
// Sources: elements below n_next of the dense matrix are the coarser level's float64 output (`prev`), the rest int32
// coefficients; n_next = halfW * halfH is a multiple of halfW, so a half-row is one or the other.
// step (j2k_plan_set_dequantize): every int32 coefficient is multiplied by it right after its conversion and before the K97 / K97I
// scaling -- dwt.Dequantize (dwt.go:514-520) in front of ReconstructMultiLevel97 -- at its two loads: half_values(false, ...) and the
// separate high row above the band that wave 0 parks in xslot.  Values from `prev` were multiplied when the coarser level read them.
// 1.0 = off (x * 1.0 is exact: tcd.ApplyInverseDWT as written); a kernel argument, not a template parameter, because it costs these
// kernels two SGPRs and nothing else (docs/KERNEL_NOTES.md, the resource tables).
// Geometry contract (checked by the plan): int32 coefficients and frame, three components with ICT, every plane
// 16 <= w <= 512, w % 8 == 0, h >= 2, offsets and strides multiples of 4 elements.

// PIX (round 4): the frame is packed 8-bit RGBA pixels (decoder.createImage for three components at precision 8, decoder.go:470-500: clamp
// to 0..255, alpha 255), pix_stride = its row stride in pixels -- two 16-byte stores per row instead of six.
template <int NW, int WPE, bool PIX>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt97_inv_rgb_wg_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes,
                             const int32_t *__restrict__ coef, const double *__restrict__ prev, int32_t *__restrict__ dst, int dc_shift, int pix_stride,
                             const int *__restrict__ guard, double step) {
    if (guard && *guard) return;             // (the frame decoder: a stream that was refused leaves the caller's frame alone)
    typedef double v2d __attribute__((ext_vector_type(2)));
    __shared__ v2d slot[NW][4][64];                      // 8 doubles per lane as four 16-byte pieces, lane-contiguous
    __shared__ v2d xslot[3][4][64];                      // d2 of the pair-row above wave 0, per component
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;                           // padding entry of the XCD-aware job order
    const DwtPlane P = planes[job.plane];
    const int w = P.w, h = P.h, halfH = (h + 1) >> 1, halfW = w >> 1;
    const int c = lane * 8;
    const bool active = c < w;
    const int q0 = job.prow0;
    const int t = q0 - 1 + wv;                           // my pair-row
    const bool live = t >= 0 && t < halfH;
    const bool hi_ex = live && 2 * t + 1 < h;            // my high row exists (false only for the last pair of an odd height)
    const bool nx = live && t + 1 < halfH && wv < NW - 1;   // the pair-row below exists (and a wave holds it)
    const int p0 = active ? lane * 4 : 0;

    // ---- loads: raw, converted at their use; component k + 1's are issued while component k runs ------------------------
    // one half-row (4 values per lane) of the level's dense matrix: float64 from the coarser level's output (two 16-byte
    // pieces) or int32 coefficients (one)
    const bool pl = t * w < P.n_next, ph = t * w + halfW < P.n_next;
    int Lr[3][16];                                       // low row t: [0..7] low half, [8..15] high half (int32: the first 4 of each)
    int Hr[3][8];                                        // high row halfH + t (never below n_next: halfH * w >= n_next)
    const int rh = halfH + min(max(t, 0), h - halfH - 1);   // clamped into the plane; hi_ex discards it when it does not exist
    auto ld4 = [&](const void *p, int *d) {
        const v4i a = *reinterpret_cast<const v4i *>(p);
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
    };
    auto issue = [&](int k) {
        ld4(coef + P.src_off[k] + rh * w + p0, &Hr[k][0]);
        ld4(coef + P.src_off[k] + rh * w + halfW + p0, &Hr[k][4]);
        if (pl) {
            ld4(prev + P.nxt_off[k] + t * w + p0, &Lr[k][0]); ld4(prev + P.nxt_off[k] + t * w + p0 + 2, &Lr[k][4]);
        } else {
            ld4(coef + P.src_off[k] + t * w + p0, &Lr[k][0]);
        }
        if (ph) {
            ld4(prev + P.nxt_off[k] + t * w + halfW + p0, &Lr[k][8]); ld4(prev + P.nxt_off[k] + t * w + halfW + p0 + 2, &Lr[k][12]);
        } else {
            ld4(coef + P.src_off[k] + t * w + halfW + p0, &Lr[k][8]);
        }
    };
    auto half_values = [&](bool from_prev, const int *a, double (&v)[4]) {
        if (from_prev) {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = __hiloint2double(a[2 * j + 1], a[2 * j]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = (double)a[j] * step;                                        // tcd.go:429-431, dwt.go:517
        }
    };
    if (live) {
        const bool extra = wv == 0 && t >= 1;             // the high row of the pair-row above the band: d2_t-1 for wave 0
        v4i Xl[3], Xh[3];
        if (extra) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int idx = (halfH + t - 1) * w;
                Xl[k] = *reinterpret_cast<const v4i *>(coef + P.src_off[k] + idx + p0);
                Xh[k] = *reinterpret_cast<const v4i *>(coef + P.src_off[k] + idx + halfW + p0);
            }
        }
        issue(0);
        if (extra) {                                       // parked in LDS (read back by wave 0 only): no registers held
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const v4i a = Xl[k], b = Xh[k];
                xslot[k][0][lane] = (v2d){(double)a.x * step * K97I, (double)a.y * step * K97I}; xslot[k][1][lane] = (v2d){(double)a.z * step * K97I, (double)a.w * step * K97I};
                xslot[k][2][lane] = (v2d){(double)b.x * step * K97I, (double)b.y * step * K97I}; xslot[k][3][lane] = (v2d){(double)b.z * step * K97I, (double)b.w * step * K97I};
            }
        }
    }

    auto put = [&](int s, const double (&lo)[4], const double (&hi)[4]) {
        slot[s][0][lane] = (v2d){lo[0], lo[1]}; slot[s][1][lane] = (v2d){lo[2], lo[3]};
        slot[s][2][lane] = (v2d){hi[0], hi[1]}; slot[s][3][lane] = (v2d){hi[2], hi[3]};
    };
    auto get = [&](const v2d (*s)[64], double (&lo)[4], double (&hi)[4]) {
        const v2d a = s[0][lane], b = s[1][lane], c2 = s[2][lane], d = s[3][lane];
        lo[0] = a.x; lo[1] = a.y; lo[2] = b.x; lo[3] = b.y; hi[0] = c2.x; hi[1] = c2.y; hi[2] = d.x; hi[3] = d.y;
    };
    // int32(v) of the reference for a batch of values: fast convert + "was any lane out of range"
    auto cvt8 = [&](const double (&x)[8], int (&v)[8]) {
        unsigned long long bad = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            bad |= __builtin_amdgcn_ballot_w64(!(x[i] < 2147483648.0));        // (the negative end saturates to the same value)
            v[i] = (int)x[i];
        }
        if (bad) {
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = go_int32(x[i]);
        }
    };

    // dwt.go:212-262 across the wave, + 0.5 (tcd.go:433); w is even and a multiple of 8 here: the only edges are column 0
    // (lane 0) and the last pair of the row (last lane)
    const bool last_lane = c + 8 >= w;
    auto hrow_inv = [&](const double (&lo)[4], const double (&hi)[4], double (&x)[8]) {
        double d[4], s_[4];
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = hi[j] * K97I;
        const double d2_l = dleft(d[3]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double dp = (j > 0) ? d[j - 1] : (lane == 0 ? d[0] : d2_l);
            s_[j] = lo[j] * K97 - D97 * (dp + d[j]);
        }
        const double s1_r = dright(s_[0]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double sn = (j < 3) ? s_[j + 1] : (last_lane ? s_[3] : s1_r);
            d[j] = d[j] - G97 * (s_[j] + sn);                                       // d becomes d1
        }
        const double d1_l = dleft(d[3]);
        {
            double dp = (lane == 0) ? d[0] : d1_l;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s_[j] = s_[j] - B97 * (dp + d[j]);                                  // s becomes e
                dp = d[j];
            }
        }
        const double e_r = dright(s_[0]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double en = (j < 3) ? s_[j + 1] : (last_lane ? s_[3] : e_r);
            x[2 * j] = s_[j] + 0.5;
            x[2 * j + 1] = (d[j] - A97 * (s_[j] + en)) + 0.5;
        }
    };

    int ve[3][8], vo[3][8];                              // rows 2t and 2t + 1 after int32(v + 0.5), per component
#pragma unroll
    for (int k = 0; k < 3; k++) {
        // The edge rules (mirrors at the first / last pair-row) are wave-uniform; as selects they would cost two v_cndmask per
        // value and step.  Instead the wave that needs a mirror writes its own row into the slot it is about to read (the
        // neighbour that would have written it does not exist), so every wave runs the same arithmetic on what it reads.
        double Dl[4], Dh[4], Sl[4], Sh[4], Rl[4], Rh[4], Ll[4], Lh[4];
        const int dn = (wv + 1 < NW) ? wv + 1 : wv;        // the slot below (the last wave's results are never used)
        if (live) {
            if (k + 1 < 3) issue(k + 1);
            half_values(false, &Hr[k][0], Dl);
            half_values(false, &Hr[k][4], Dh);
            half_values(pl, &Lr[k][0], Ll);
            half_values(ph, &Lr[k][8], Lh);
#pragma unroll
            for (int j = 0; j < 4; j++) { Dl[j] = Dl[j] * K97I; Dh[j] = Dh[j] * K97I; }
            if (hi_ex && wv < NW - 1) put(wv + 1, Dl, Dh);
            if (t == 0) put(wv, Dl, Dh);                   // d2[-1] := d2[0]
        }
        __syncthreads();
        // undo delta: s1 = K s2 - d (d2[t-1] + d2); no high row (odd height, last pair): d2 := d2[t-1]
        if (live) {
            const v2d (*up)[64] = (wv == 0 && t >= 1) ? xslot[k] : slot[wv];
            get(up, Rl, Rh);
            if (!hi_ex) get(up, Dl, Dh);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                Sl[j] = Ll[j] * K97 - D97 * (Rl[j] + Dl[j]);
                Sh[j] = Lh[j] * K97 - D97 * (Rh[j] + Dh[j]);
            }
            put(wv, Sl, Sh);
            if (!nx && wv < NW - 1) put(wv + 1, Sl, Sh);   // s1 past the end mirrors s1
        }
        __syncthreads();
        // undo gamma: d1 = d2 - g (s1 + s1[t+1]); no high row: d1 := d1[t-1] (below)
        if (live) {
            get(slot[dn], Rl, Rh);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                Dl[j] = Dl[j] - G97 * (Sl[j] + Rl[j]);                             // D becomes d1
                Dh[j] = Dh[j] - G97 * (Sh[j] + Rh[j]);
            }
            if (hi_ex && wv < NW - 1) put(wv + 1, Dl, Dh);
            if (t == 0) put(wv, Dl, Dh);                   // d1[-1] := d1[0]
        }
        __syncthreads();
        // undo beta: e = s1 - b (d1[t-1] + d1)       (wave 0 has no d1[t-1]: its e is never used)
        if (live) {
            get(slot[wv], Rl, Rh);
            if (!hi_ex) get(slot[wv], Dl, Dh);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                Sl[j] = Sl[j] - B97 * (Rl[j] + Dl[j]);                             // S becomes e
                Sh[j] = Sh[j] - B97 * (Rh[j] + Dh[j]);
            }
            put(wv, Sl, Sh);
            if (!nx && wv < NW - 1) put(wv + 1, Sl, Sh);   // e past the end mirrors e
        }
        __syncthreads();
        // undo alpha: o = d1 - a (e + e[t+1])
        if (live && wv >= 1 && wv <= NW - 3) {
            get(slot[wv + 1], Rl, Rh);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                Dl[j] = Dl[j] - A97 * (Sl[j] + Rl[j]);                             // D becomes o
                Dh[j] = Dh[j] - A97 * (Sh[j] + Rh[j]);
            }
            // rows: horizontal inverse (dwt.go:212-262 across the wave) and tcd.go:433-435
            double x[8];
            hrow_inv(Sl, Sh, x);
            cvt8(x, ve[k]);
            if (hi_ex) {
                hrow_inv(Dl, Dh, x);
                cvt8(x, vo[k]);
            }
        }
    }
    if (!live || wv < 1 || wv > NW - 3 || !active) return;          // the outer three waves of the band store nothing
    // decoder.go:326-339 + mct.go:43-53, then mct.go:113-118
    auto finish = [&](int ro, const int (&v)[3][8]) {
        double r_[8], g_[8], b_[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const double y = (double)v[0][i], cb = (double)v[1][i], cr = (double)v[2][i];
            r_[i] = (y + 1.402 * cr) + 0.5;
            g_[i] = (y - 0.34413 * cb - 0.71414 * cr) + 0.5;
            b_[i] = (y + 1.772 * cb) + 0.5;
        }
        int o[3][8];
        cvt8(r_, o[0]); cvt8(g_, o[1]); cvt8(b_, o[2]);
        if constexpr (PIX) {
            const int64_t y0 = P.out_off[0] / P.out_stride, x0 = P.out_off[0] - y0 * P.out_stride;
            uint32_t px[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t rr = (uint32_t)min(max((int)((unsigned)o[0][i] + (unsigned)dc_shift), 0), 255), gg = (uint32_t)min(max((int)((unsigned)o[1][i] + (unsigned)dc_shift), 0), 255),
                               bb = (uint32_t)min(max((int)((unsigned)o[2][i] + (unsigned)dc_shift), 0), 255);
                px[i] = rr | gg << 8 | bb << 16 | 0xFF000000u;
            }
            v4i *p = reinterpret_cast<v4i *>(reinterpret_cast<uint32_t *>(dst) + (y0 + ro) * (int64_t)pix_stride + x0 + c);
            p[0] = (v4i){(int)px[0], (int)px[1], (int)px[2], (int)px[3]};
            p[1] = (v4i){(int)px[4], (int)px[5], (int)px[6], (int)px[7]};
            return;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v4i *p = reinterpret_cast<v4i *>(dst + P.out_off[k] + (int64_t)ro * P.out_stride + c);
            p[0] = (v4i){(int)((unsigned)o[k][0] + (unsigned)dc_shift), (int)((unsigned)o[k][1] + (unsigned)dc_shift),
                         (int)((unsigned)o[k][2] + (unsigned)dc_shift), (int)((unsigned)o[k][3] + (unsigned)dc_shift)};
            p[1] = (v4i){(int)((unsigned)o[k][4] + (unsigned)dc_shift), (int)((unsigned)o[k][5] + (unsigned)dc_shift),
                         (int)((unsigned)o[k][6] + (unsigned)dc_shift), (int)((unsigned)o[k][7] + (unsigned)dc_shift)};
        }
    };
    finish(2 * t, ve);
    if (hi_ex) finish(2 * t + 1, vo);
}

// The same for ONE plane of a deeper level (dwt.go:566-573: level l's output is the float64 prefix level l - 1 reads): int32
// coefficients + the coarser level's float64 prefix in, a dense float64 matrix out; no colour transform, no rounding.  One
// component means 60-odd VGPRs and seven waves per SIMD; planes narrower than 512 columns use the first w / 8 lanes.
// Round 4: CF64 -- the coefficients are float64 (the unit calls dwt.Inverse2D97 / ReconstructMultiLevel97, dwt.go:453-473, 561-573);
// DSTI32 -- level 0 of ONE component of an int32 frame: int32(v + 0.5) (tcd.go:433-435) and the DC shift (mct.go:113-118) at the
// store, rows out_stride apart.  step: as above, in load_half's int32 branch only (CF64 has no quantiser and is passed 1.0).
template <int NW, int WPE, bool CF64, bool DSTI32>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt97_inv_plane_wg_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes,
                               const void *__restrict__ coef_, const double *__restrict__ prev, void *__restrict__ dst_, int dc_shift, int frame_rows, int pix_stride,
                               const int *__restrict__ guard, double step) {
    if (guard && *guard) return;             // (the frame decoder: a stream that was refused leaves the caller's frame alone)
    const int32_t *coef = reinterpret_cast<const int32_t *>(coef_);
    const double *coeff = reinterpret_cast<const double *>(coef_);
    double *dst = reinterpret_cast<double *>(dst_);
    typedef double v2d __attribute__((ext_vector_type(2)));
    __shared__ v2d slot[NW][4][64];
    __shared__ v2d xslot[4][64];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    const DwtPlane P = planes[job.plane];
    const int w = P.w, h = P.h, halfH = (h + 1) >> 1, halfW = w >> 1;
    const int c = lane * 8;
    const bool active = c < w;
    const int t = job.prow0 - 1 + wv;
    const bool live = t >= 0 && t < halfH;
    const bool hi_ex = live && 2 * t + 1 < h;
    const bool nx = live && t + 1 < halfH && wv < NW - 1;
    const int p0 = active ? lane * 4 : 0;
    const bool last_lane = c + 8 >= w;
    // float64 coefficients (the unit calls) can make x + x overflow at a mirrored edge: the reference's (2 * c) * x there (lift97); wave-uniform
    // for the rows: the row read from the slot is this wave's own above the first pair-row / for a missing odd row, and below the last pair-row
    const bool m_up = CF64 && (t == 0 || !hi_ex), m_dn = CF64 && t + 1 >= halfH;
    auto put = [&](int s, const double (&lo)[4], const double (&hi)[4]) {
        slot[s][0][lane] = (v2d){lo[0], lo[1]}; slot[s][1][lane] = (v2d){lo[2], lo[3]};
        slot[s][2][lane] = (v2d){hi[0], hi[1]}; slot[s][3][lane] = (v2d){hi[2], hi[3]};
    };
    auto get = [&](const v2d (*s)[64], double (&lo)[4], double (&hi)[4]) {
        const v2d a = s[0][lane], b = s[1][lane], c2 = s[2][lane], d = s[3][lane];
        lo[0] = a.x; lo[1] = a.y; lo[2] = b.x; lo[3] = b.y; hi[0] = c2.x; hi[1] = c2.y; hi[2] = d.x; hi[3] = d.y;
    };
    auto load_half = [&](int idx, double (&v)[4]) {      // float64 from the coarser level's output, or int32 coefficients (tcd.go:429-431)
        if (idx < P.n_next) {
            const v2d *p = reinterpret_cast<const v2d *>(prev + P.nxt_off[0] + idx + p0);
            const v2d a = p[0], b = p[1];
            v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
        } else if constexpr (CF64) {
            const v2d *p = reinterpret_cast<const v2d *>(coeff + P.src_off[0] + idx + p0);
            const v2d a = p[0], b = p[1];
            v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
        } else {
            const v4i a = *reinterpret_cast<const v4i *>(coef + P.src_off[0] + idx + p0);
            v[0] = (double)a.x * step; v[1] = (double)a.y * step; v[2] = (double)a.z * step; v[3] = (double)a.w * step;   // dwt.go:517
        }
    };
    double Dl[4], Dh[4], Sl[4], Sh[4], Rl[4], Rh[4], Ll[4], Lh[4];
    const int dn = (wv + 1 < NW) ? wv + 1 : wv;
    if (live) {
        const int rh = halfH + min(t, h - halfH - 1);    // clamped into the plane; hi_ex discards it when it does not exist
        if (wv == 0 && t >= 1) {                         // d2 of the pair-row above the band, for wave 0 itself
            double Xl[4], Xh[4];
            load_half((halfH + t - 1) * w, Xl); load_half((halfH + t - 1) * w + halfW, Xh);
#pragma unroll
            for (int j = 0; j < 4; j++) { Xl[j] = Xl[j] * K97I; Xh[j] = Xh[j] * K97I; }
            xslot[0][lane] = (v2d){Xl[0], Xl[1]}; xslot[1][lane] = (v2d){Xl[2], Xl[3]};
            xslot[2][lane] = (v2d){Xh[0], Xh[1]}; xslot[3][lane] = (v2d){Xh[2], Xh[3]};
        }
        load_half(rh * w, Dl); load_half(rh * w + halfW, Dh);
        load_half(t * w, Ll); load_half(t * w + halfW, Lh);
#pragma unroll
        for (int j = 0; j < 4; j++) { Dl[j] = Dl[j] * K97I; Dh[j] = Dh[j] * K97I; }
        if (hi_ex && wv < NW - 1) put(wv + 1, Dl, Dh);
        if (t == 0) put(wv, Dl, Dh);
    }
    __syncthreads();
    if (live) {
        const v2d (*up)[64] = (wv == 0 && t >= 1) ? xslot : slot[wv];
        get(up, Rl, Rh);
        if (!hi_ex) get(up, Dl, Dh);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            Sl[j] = Ll[j] * K97 - lift97(D97, Dl[j], Rl[j], m_up);
            Sh[j] = Lh[j] * K97 - lift97(D97, Dh[j], Rh[j], m_up);
        }
        put(wv, Sl, Sh);
        if (!nx && wv < NW - 1) put(wv + 1, Sl, Sh);
    }
    __syncthreads();
    if (live) {
        get(slot[dn], Rl, Rh);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            Dl[j] = Dl[j] - lift97(G97, Sl[j], Rl[j], m_dn);
            Dh[j] = Dh[j] - lift97(G97, Sh[j], Rh[j], m_dn);
        }
        if (hi_ex && wv < NW - 1) put(wv + 1, Dl, Dh);
        if (t == 0) put(wv, Dl, Dh);
    }
    __syncthreads();
    if (live) {
        get(slot[wv], Rl, Rh);
        if (!hi_ex) get(slot[wv], Dl, Dh);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            Sl[j] = Sl[j] - lift97(B97, Dl[j], Rl[j], m_up);
            Sh[j] = Sh[j] - lift97(B97, Dh[j], Rh[j], m_up);
        }
        put(wv, Sl, Sh);
        if (!nx && wv < NW - 1) put(wv + 1, Sl, Sh);
    }
    __syncthreads();
    if (!live || wv < 1 || wv > NW - 3) return;
    get(slot[wv + 1], Rl, Rh);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        Dl[j] = Dl[j] - lift97(A97, Sl[j], Rl[j], m_dn);
        Dh[j] = Dh[j] - lift97(A97, Sh[j], Rh[j], m_dn);
    }
    // dwt.go:212-262 across the wave (w even, a multiple of 8: the edges are lane 0 and the last lane)
    auto hrow_out = [&](const double (&lo)[4], const double (&hi)[4], int ro) {
        double d[4], s_[4], x[8];
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = hi[j] * K97I;
        const double d2_l = dleft(d[3]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double dp = (j > 0) ? d[j - 1] : (lane == 0 ? d[0] : d2_l);
            s_[j] = lo[j] * K97 - lift97(D97, d[j], dp, CF64 && j == 0 && lane == 0);
        }
        const double s1_r = dright(s_[0]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double sn = (j < 3) ? s_[j + 1] : (last_lane ? s_[3] : s1_r);
            d[j] = d[j] - lift97(G97, s_[j], sn, CF64 && j == 3 && last_lane);
        }
        const double d1_l = dleft(d[3]);
        {
            double dp = (lane == 0) ? d[0] : d1_l;
#pragma unroll
            for (int j = 0; j < 4; j++) { s_[j] = s_[j] - lift97(B97, d[j], dp, CF64 && j == 0 && lane == 0); dp = d[j]; }
        }
        const double e_r = dright(s_[0]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double en = (j < 3) ? s_[j + 1] : (last_lane ? s_[3] : e_r);
            x[2 * j] = s_[j];
            x[2 * j + 1] = d[j] - lift97(A97, s_[j], en, CF64 && j == 3 && last_lane);
        }
        if (active) {
            if constexpr (DSTI32) {
                int q[8];
#pragma unroll
                for (int i = 0; i < 8; i++) q[i] = (int)((unsigned)go_int32(x[i] + 0.5) + (unsigned)dc_shift);
                if (pix_stride > 0) {                    // image.Gray.Pix (decoder.createImage, one component at precision 8: clamp to 0..255, decoder.go:428-447)
                    const int64_t y0 = P.out_off[0] / P.out_stride, x0 = P.out_off[0] - y0 * P.out_stride;
                    uint2 o = {0, 0};
#pragma unroll
                    for (int i = 0; i < 8; i++) { const uint32_t v = (uint32_t)min(max(q[i], 0), 255) << (8 * (i & 3)); if (i < 4) o.x |= v; else o.y |= v; }
                    *reinterpret_cast<uint2 *>(reinterpret_cast<uint8_t *>(dst_) + (y0 + ro) * (int64_t)pix_stride + x0 + c) = o;
                } else {
                    v4i *p = reinterpret_cast<v4i *>(reinterpret_cast<int32_t *>(dst_) + P.out_off[0] + (int64_t)ro * P.out_stride + c);
                    p[0] = (v4i){q[0], q[1], q[2], q[3]}; p[1] = (v4i){q[4], q[5], q[6], q[7]};
                }
            } else {
                v2d *p = reinterpret_cast<v2d *>(dst + P.out_off[0] + (int64_t)ro * (frame_rows ? P.out_stride : w) + c);    // a frame's rows / the dense scratch matrix
                p[0] = (v2d){x[0], x[1]}; p[1] = (v2d){x[2], x[3]}; p[2] = (v2d){x[4], x[5]}; p[3] = (v2d){x[6], x[7]};
            }
        }
    };
    hrow_out(Sl, Sh, 2 * t);
    if (hi_ex) hrow_out(Dl, Dh, 2 * t + 1);
}
