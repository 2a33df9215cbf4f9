// dwt97_l0wg.inc -- level 0 of the lossy forward path for an RGB triple of int32 planes, workgroup form (included by dwt97.hip).
//
// Replaces, fused: mct.DCLevelShiftForward (mct.go:96-101), the int32 -> float64 copies + mct.ForwardICT + round half away
// (encoder.go:227-244), dwt.Forward2D97 as level 0 of DecomposeMultiLevel97 (dwt.go:161-210, 432-451, 551-558) and, on the
// final coefficients, the encoder's quantisation int32(v / step +- 0.5) (encoder.go:265-276) or tcd's int32(v +- 0.5)
// (tcd.go:520-532).
//
// Same idea as dwt53_l0pix.inc, adapted to four lifting steps in float64:
//   * one workgroup = one COMPONENT of one <= 512-column tile plane x a band of pair-rows; wave i owns pair-row t = q0 - 2 + i,
//     loads its two source rows of all three planes (six 16-byte loads per row, every load of the wave in flight at once),
//     applies DC shift + ICT + rounding for ITS component only and the horizontal 9-7 across the wave (DPP);
//   * the four vertical steps alternate between needing the pair-row below (alpha, gamma) and the one above (beta, delta):
//     four LDS exchanges of one row (8 doubles per lane, 4 KB per wave), each slot recycled by its only reader:
//       slot[i]   <- e_t | barrier | wave i: d1_t = o_t + a (e_t + e_t+1)      (e_t+1 from slot[i+1]); slot[i+1] <- d1_t
//                         barrier | wave i: s1_t = e_t + b (d1_t-1 + d1_t)     (d1_t-1 from slot[i]);  slot[i]   <- s1_t
//                         barrier | wave i: d2_t = d1_t + g (s1_t + s1_t+1)    (s1_t+1 from slot[i+1]); slot[i+1] <- d2_t
//                         barrier | wave i: s2_t = s1_t + d (d2_t-1 + d2_t)    (d2_t-1 from slot[i]);  store s2 k97Inv, d2 k97
//     A band of NR output pair-rows needs two pair-rows above and one below (plus one more even row, which the last wave
//     transforms itself): NW = NR + 3 waves, the outer three store nothing -- the 7 halo rows of the marching kernel, but
//     recomputed per band instead of carried, in exchange for ~38 000 short waves with no loop-carried memory latency;
//   * the three components of a band are three workgroups that read the same six source rows per wave: the job order puts
//     them on one XCD (L2 hits); the read side is 12 of 27 bytes per pixel;
//   * v / step for the constant step = 1.0 / Quality is evaluated as q0 = v * r, q = fma(fma(-q0, step, v), r, q0) with
//     r = RN(1 / step): three instructions instead of the ~14 of the IEEE divide expansion, and -- by Markstein's theorem, r
//     being the correctly rounded reciprocal and q0 within an ulp of the quotient -- the same correctly rounded result the
//     reference's division gives (checked against the oracle's true division on every coefficient of their frames by
//     tests/test_gpu_lossy97_oracle.py -- every workgroup width, Quality 1, 2, 3, 75, 100, 101, 4097, 8191, samples inside and
//     outside the precision -- and tests/test_gpu_dwt97.py, and by tests/test_markstein_division.py on 10^7 values per
//     Quality on the CPU).
// Bit-exactness otherwise as dwt97.hip: no contraction (-ffp-contract=off; the two fma above are explicit and exact by
// construction), the reference's literal constants and operand association.
// Geometry contract (checked by the plan): int32 source, three components with ICT, every plane 16 <= w <= 512, w % 8 == 0,
// h >= 2.  Everything else takes the general kernel.

// Go's int32(float64) (amd64: CVTTSD2SL -- truncation, 0x80000000 for NaN and whatever does not fit) from the hardware convert, which
// saturates instead: the two differ only past the positive end, one compare + select.  The plan proves every value converted
// here to be inside int32 when the samples lie inside the declared precision (precision <= 16, Quality < 8192) -- but
// j2k_plan_forward takes arbitrary int32 planes, and for those the select is what keeps this kernel on the reference's answer
// (ADVICE r2; tests/test_gpu_knobs.py::test_lossy_level0_samples_outside_the_precision).  Measured alternatives on a 4K frame:
// no check 67.4 us; a wave-level range test of the samples with an exact redo 78.7 us; the redo as a second code path 151 us
// (registers: 60 spilled); this select 68.8 us.
__device__ __forceinline__ int cvt_go(double x) { return x < 2147483648.0 ? (int)x : (int)0x80000000; }
// int32(v +- 0.5) of the reference: truncation toward zero after adding half with v's sign (v >= 0 is false only for negative
// v: -0.0 takes +0.5 like the reference, result 0 either way)
__device__ __forceinline__ int round_half_away_inrange(double v) {
    const double half = __hiloint2double((__double2hiint(v) & 0x80000000) | 0x3FE00000, 0);    // copysign(0.5, v)
    return cvt_go(v + half);
}

// SRC 0: int32 RGB triple, one component per workgroup (DC shift + ICT + rounding in the row load).  SRC 1: one float64 plane (the
// deeper levels, whose input is the scratch prefix of the level above: dwt.go:551-558; with QUANT = none also the float64 unit calls
// dwt.Forward2D97 / DecomposeMultiLevel97, dwt.go:432-451, 551-558) -- same workgroup, the row load is four 16-byte loads of doubles;
// planes narrower than 512 columns use the first w / 8 lanes.  SRC 2 (round 4): level 0 of ONE int32 component -- a gray frame, or the
// components of a frame without the colour transform: DC shift and the conversion in the row load (encoder.go:228-233, 259-262).
// SRC 3 (round 4): as SRC 0 with the triple read out of packed 8-bit RGBA pixels (image.RGBA.Pix, encoder.go:108-122: alpha ignored) --
// `src` is the pixel frame, pix_stride its row stride in pixels; two 16-byte loads per row instead of six.  This is the reference's
// DEFAULT path: DefaultOptions() is lossy at Quality 75 (jpeg2000.go:305-316).
template <int NW, int QUANT, int WPE, int SRC>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt97_fwd_rgb_wg_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes,
                             const int32_t *__restrict__ src, const double *__restrict__ srcf, int32_t *__restrict__ out_i32,
                             double *__restrict__ out_f64, double *__restrict__ nxt, int dc_shift, double step, double rstep, int pix_stride) {
    typedef double v2d __attribute__((ext_vector_type(2)));
    __shared__ v2d slot[NW + 1][4][64];                  // 8 doubles per lane as four 16-byte pieces, lane-contiguous
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;                           // padding entry of the XCD-aware job order
    const DwtPlane P = planes[job.plane];
    const int k = job.col0;                              // this workgroup's component
    // (indexed straight from the table: a run-time index into the local copy would make it an LDS-promoted array)
    const int64_t out_off_k = planes[job.plane].out_off[k], nxt_off_k = planes[job.plane].nxt_off[k];
    const int w = P.w, h = P.h, halfH = (h + 1) >> 1, halfW = w >> 1;
    const int c = lane * 8;
    const bool active = c < w;
    const bool last_lane = c + 8 >= w;
    // arbitrary float64 samples (the unit calls) can make x + x overflow at a mirrored edge where the reference's (2 * c) * x stays
    // finite: lift97's second form there; samples that come from int32 are far below that, and keep one form for every position
    constexpr bool EDGE = (SRC == 1);
    const int q0 = job.prow0;
    const int t = q0 - 2 + wv;                           // my pair-row
    const bool live = t >= 0 && t < halfH;
    const bool o_ex = live && 2 * t + 1 < h, en_ex = live && 2 * t + 2 < h;
    const int cc = active ? c : 0;
    // row k of the ICT matrix (mct.go:16-18) as wave-uniform coefficients: a - m*b is a + (-m)*b bit for bit, so one
    // expression serves the three components without a branch per pixel
    const double c_r = (k == 0) ? 0.299 : (k == 1) ? -0.16875 : 0.5;
    const double c_g = (k == 0) ? 0.587 : (k == 1) ? -0.33126 : -0.41869;
    const double c_b = (k == 0) ? 0.114 : (k == 1) ? 0.5 : -0.08131;

    // one source row -> this component after DC shift + ICT + rounding -> horizontal 9-7: lo[4], hi[4]
    auto hrow = [&](int r, double (&lo)[4], double (&hi)[4]) {
        r = min(max(r, 0), h - 1);
        double x[8];
        if constexpr (SRC == 1) {
            const v2d *p = reinterpret_cast<const v2d *>(srcf + P.src_off[0] + (int64_t)r * P.src_stride + cc);
            const v2d a = p[0], b = p[1], c2 = p[2], d = p[3];
            x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y; x[4] = c2.x; x[5] = c2.y; x[6] = d.x; x[7] = d.y;
        } else if constexpr (SRC == 2) {
            int raw[8];
            if (pix_stride > 0) {                        // image.Gray.Pix: a byte per pixel (encoder.go:84-93), pix_stride = the frame's row stride in pixels
                const int64_t y0 = P.src_off[0] / P.src_stride, x0 = P.src_off[0] - y0 * P.src_stride;
                const uint2 a = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint8_t *>(src) + (y0 + r) * (int64_t)pix_stride + x0 + cc);
#pragma unroll
                for (int i = 0; i < 8; i++) raw[i] = (int)(((i < 4 ? a.x : a.y) >> (8 * (i & 3))) & 0xFF);
            } else {
                const int4 *p = reinterpret_cast<const int4 *>(src + P.src_off[0] + (int64_t)r * P.src_stride + cc);
                const int4 a = p[0], b = p[1];
                raw[0] = a.x; raw[1] = a.y; raw[2] = a.z; raw[3] = a.w; raw[4] = b.x; raw[5] = b.y; raw[6] = b.z; raw[7] = b.w;
            }
#pragma unroll
            for (int i = 0; i < 8; i++) x[i] = (double)(int)((unsigned)raw[i] - (unsigned)dc_shift);     // mct.go:96-101, then float64(v)
        } else if constexpr (SRC == 3) {
            const int64_t y0 = P.src_off[0] / P.src_stride, x0 = P.src_off[0] - y0 * P.src_stride;        // the tile's origin (component 0 of the frame)
            const uint4 *p = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint32_t *>(src) + (y0 + r) * (int64_t)pix_stride + x0 + cc);
            const uint4 a = p[0], b = p[1];
            const uint32_t dw[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const double r_ = (double)((int)(dw[i] & 0xFF) - dc_shift), g_ = (double)((int)((dw[i] >> 8) & 0xFF) - dc_shift),
                             b_ = (double)((int)((dw[i] >> 16) & 0xFF) - dc_shift);
                const double y = c_r * r_ + c_g * g_ + c_b * b_;
                x[i] = (double)round_half_away_inrange(y);
            }
        } else {
            int raw[3][8];
#pragma unroll
            for (int kk = 0; kk < 3; kk++) {
                const int4 *p = reinterpret_cast<const int4 *>(src + P.src_off[kk] + (int64_t)r * P.src_stride + cc);
                const int4 a = p[0], b = p[1];
                raw[kk][0] = a.x; raw[kk][1] = a.y; raw[kk][2] = a.z; raw[kk][3] = a.w;
                raw[kk][4] = b.x; raw[kk][5] = b.y; raw[kk][6] = b.z; raw[kk][7] = b.w;
            }
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const double r_ = (double)(int)((unsigned)raw[0][i] - (unsigned)dc_shift), g_ = (double)(int)((unsigned)raw[1][i] - (unsigned)dc_shift),
                             b_ = (double)(int)((unsigned)raw[2][i] - (unsigned)dc_shift);
                const double y = c_r * r_ + c_g * g_ + c_b * b_;
                x[i] = (double)round_half_away_inrange(y);
            }
        }
        // dwt.go:161-210 across the wave; w is even and >= 16 here: the only edges are column 0 and the last pair of the row
        double d1[4], s1[4], d2[4];
        const double e_r = dright(x[0]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double en = (j < 3) ? x[2 * j + 2] : (last_lane ? x[6] : e_r);
            d1[j] = x[2 * j + 1] + lift97(A97, x[2 * j], en, EDGE && j == 3 && last_lane);
        }
        const double d1_l = dleft(d1[3]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double dp = (j > 0) ? d1[j - 1] : (lane == 0 ? d1[0] : d1_l);
            s1[j] = x[2 * j] + lift97(B97, d1[j], dp, EDGE && j == 0 && lane == 0);
        }
        const double s1_r = dright(s1[0]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double sn = (j < 3) ? s1[j + 1] : (last_lane ? s1[3] : s1_r);
            d2[j] = d1[j] + lift97(G97, s1[j], sn, EDGE && j == 3 && last_lane);
        }
        const double d2_l = dleft(d2[3]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double dp = (j > 0) ? d2[j - 1] : (lane == 0 ? d2[0] : d2_l);
            lo[j] = (s1[j] + lift97(D97, d2[j], dp, EDGE && j == 0 && lane == 0)) * K97I;
            hi[j] = d2[j] * K97;
        }
    };
    auto put = [&](int s, const double (&lo)[4], const double (&hi)[4]) {
        slot[s][0][lane] = (v2d){lo[0], lo[1]}; slot[s][1][lane] = (v2d){lo[2], lo[3]};
        slot[s][2][lane] = (v2d){hi[0], hi[1]}; slot[s][3][lane] = (v2d){hi[2], hi[3]};
    };
    auto get = [&](int s, double (&lo)[4], double (&hi)[4]) {
        const v2d a = slot[s][0][lane], b = slot[s][1][lane], c2 = slot[s][2][lane], d = slot[s][3][lane];
        lo[0] = a.x; lo[1] = a.y; lo[2] = b.x; lo[3] = b.y; hi[0] = c2.x; hi[1] = c2.y; hi[2] = d.x; hi[3] = d.y;
    };

    // The edge rules (mirrors at the first / last pair-row) are wave-uniform; as selects they would cost two v_cndmask per value
    // and step.  Instead the wave that needs a mirror writes its own row into the slot it is about to read (the neighbour that
    // would have written it does not exist), so every wave runs the same arithmetic on what it reads.  slot[NW] is the last
    // wave's "row below".
    double El[4], Eh[4], Ol[4], Oh[4], Nl[4], Nh[4];
    const bool nx = live && t + 1 < halfH && wv < NW - 1;    // the pair-row below exists and a wave holds it
    // (wave-uniform) the row read from the slot is this wave's own: the mirror above the first pair-row / of a missing odd row, below the last row
    const bool m_up = EDGE && (t == 0 || !o_ex), m_dn1 = EDGE && !en_ex, m_dn3 = EDGE && t + 1 >= halfH;
    if (live) {
        hrow(2 * t, El, Eh);
        put(wv, El, Eh);
        hrow(2 * t + 1, Ol, Oh);
        if (wv == NW - 1) {                                   // the last wave transforms the even row below itself
            if (en_ex) { hrow(2 * t + 2, Nl, Nh); put(NW, Nl, Nh); }
            else put(NW, El, Eh);
        } else if (!en_ex) put(wv + 1, El, Eh);               // no next even row: e_next := e
    }
    __syncthreads();
    // step 1 (alpha): d1 = o + a (e + e_next); no odd row (odd height, last): d1 := d1[t-1] (below)
    if (live) {
        get(wv + 1, Nl, Nh);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            Ol[j] = Ol[j] + lift97(A97, El[j], Nl[j], m_dn1);                // O becomes d1
            Oh[j] = Oh[j] + lift97(A97, Eh[j], Nh[j], m_dn1);
        }
        if (wv < NW - 1 && o_ex) put(wv + 1, Ol, Oh);
        if (t == 0) put(wv, Ol, Oh);                          // d1[-1] := d1[0]
    }
    __syncthreads();
    // step 2 (beta): s1 = e + b (d1[t-1] + d1)        (wave 0 of a band below the top has no d1[t-1]: its s1 is never used)
    if (live) {
        double Pl[4], Ph[4];
        get(wv, Pl, Ph);
        if (!o_ex) get(wv, Ol, Oh);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            El[j] = El[j] + lift97(B97, Ol[j], Pl[j], m_up);                 // E becomes s1
            Eh[j] = Eh[j] + lift97(B97, Oh[j], Ph[j], m_up);
        }
        put(wv, El, Eh);
        if (!nx && wv < NW - 1) put(wv + 1, El, Eh);          // s1 past the end mirrors s1 (dwt.go:189-197)
    }
    __syncthreads();
    // step 3 (gamma): d2 = d1 + g (s1 + s1[t+1])      (the last wave has no s1[t+1]: its d2 is never used)
    if (live) {
        get(wv + 1, Nl, Nh);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            Ol[j] = Ol[j] + lift97(G97, El[j], Nl[j], m_dn3);                // O becomes d2
            Oh[j] = Oh[j] + lift97(G97, Eh[j], Nh[j], m_dn3);
        }
        if (wv < NW - 1 && o_ex) put(wv + 1, Ol, Oh);
        if (t == 0) put(wv, Ol, Oh);                          // d2[-1] := d2[0]
    }
    __syncthreads();
    if (!live || wv < 2 || wv >= NW - 1 || !active) return;       // the outer three waves of the band store nothing
    {
        // step 4 (delta): s2 = s1 + d (d2[t-1] + d2); no odd row: d2 := d2[t-1]
        double Pl[4], Ph[4];
        get(wv, Pl, Ph);
        if (!o_ex) get(wv, Ol, Oh);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            El[j] = (El[j] + lift97(D97, Ol[j], Pl[j], m_up)) * K97I;
            Eh[j] = (Eh[j] + lift97(D97, Oh[j], Ph[j], m_up)) * K97I;
            Ol[j] = Ol[j] * K97;
            Oh[j] = Oh[j] * K97;
        }
    }
    // stores: the prefix that feeds level 1 stays float64 in scratch; everything else is final (quantised int32, or f64)
    auto quant = [&](double v) -> int {
        if constexpr (SRC != 0) {
            // deeper levels, single components: the plan's bound on level 0 (values inside int32) is not claimed for them -- the general kernel's
            // exact forms (IEEE division, Go's out-of-range conversion); these planes are a quarter of the frame and less
            if constexpr (QUANT == Q_ENCODER_) return v >= 0 ? go_int32(v / step + 0.5) : go_int32(v / step - 0.5);
            else return round_half_away(v);
        } else if constexpr (QUANT == Q_ENCODER_) {
            const double q0_ = v * rstep;
            const double q = __builtin_fma(__builtin_fma(-q0_, step, v), rstep, q0_);      // == v / step, correctly rounded
            // encoder.go:270-275: the sign test is on v, the half is added to the quotient (same sign: step > 0)
            const double half = __hiloint2double((__double2hiint(v) & 0x80000000) | 0x3FE00000, 0);
            return cvt_go(q + half);
        } else {
            return round_half_away_inrange(v);                                               // tcd.go:526-531
        }
    };
    auto store_half = [&](int64_t idx, bool fin, const double (&v)[4]) {
        if (!fin) {
            v2d *p = reinterpret_cast<v2d *>(nxt + nxt_off_k + idx);
            p[0] = (v2d){v[0], v[1]}; p[1] = (v2d){v[2], v[3]};
        } else if constexpr (QUANT == Q_NONE_) {
            v2d *p = reinterpret_cast<v2d *>(out_f64 + out_off_k + idx);
            p[0] = (v2d){v[0], v[1]}; p[1] = (v2d){v[2], v[3]};
        } else {
            const v4i q = {quant(v[0]), quant(v[1]), quant(v[2]), quant(v[3])};
            __builtin_nontemporal_store(q, reinterpret_cast<v4i *>(out_i32 + out_off_k + idx));
        }
    };
    auto store_row = [&](int ro, const double (&lo)[4], const double (&hi)[4]) {
        const int64_t idxL = (int64_t)ro * w + lane * 4;
        store_half(idxL, ro * w >= P.n_next, lo);
        store_half(idxL + halfW, ro * w + halfW >= P.n_next, hi);
    };
    store_row(t, El, Eh);
    if (o_ex) store_row(halfH + t, Ol, Oh);
}
