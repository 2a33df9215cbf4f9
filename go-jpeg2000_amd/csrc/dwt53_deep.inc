// dwt53_deep.inc -- every decomposition level below level 0 of the 5-3 transform in ONE launch per direction (included by
// dwt53.hip inside namespace j2k, after the tail kernels whose LDS level routines it reuses).
//
// Replaces the level >= 1 iterations of dwt.DecomposeMultiLevel53 / ReconstructMultiLevel53 (dwt.go:524-548), each of them
// one Forward2D53 / Inverse2D53 (dwt.go:356-429) on the contiguous prefix of the component's array.
//
// Why one launch: round 2 ran level 1 as its own bandwidth kernel (C2: 49.8 MB, 9.8 us) and levels 2..4 as a one-workgroup-
// per-plane LDS kernel (15.6 MB, 11.2 us: launch + one dependent chain of load -> three levels -> store) -- 21 us for a third
// of the transform's bytes, half of it waiting on a launch boundary.  The reference's layout makes the split unnecessary:
// level l+1 reads the first ceil(w/2)*ceil(h/2) ELEMENTS of level l's output as a dense matrix, i.e. (w even) the first
// ceil(h/2)/2 low-pass ROWS -- which depend only on the top half of level l's input.  So per plane
//   * one DEEP workgroup takes pair-rows 0 .. T-1 (T = ceil(ceil(h/2)/2)) of level l0 straight from memory, keeps the low-pass
//     rows in LDS as the level l0+1 matrix and runs every further level there (tail_fwd_level), and
//   * FLAT workgroups take the remaining pair-rows of level l0 (all of their output is final),
// all in the same grid, deep workgroups first so that their dependent chain starts at once and the flat ones fill the other
// CUs meanwhile.  The inverse is the mirror image: the deep workgroup rebuilds levels L-1 .. l0+1 in LDS (tail_inv_level),
// then the top half of level l0 from LDS low-pass rows + high-pass rows from memory, while the flat workgroups rebuild the
// bottom half, which needs nothing from the coarser levels.
//
// A wave = DEEP_PER consecutive pair-rows x 4 columns per lane (one 16-byte load per row, 256 columns per wave), every load
// of the wave in flight at once, horizontal lifting by DPP across the wave (hfwd<4> / hinv<4>), the vertical neighbours of
// the wave's first / last pair-row through two LDS slots (forward: E of the pair-row below, d of the pair-row above; inverse:
// e of the pair-row below).  The first / last wave of a job loads the job's halo rows itself.
// Geometry contract (checked by the plan): at level l0 every plane has 8 <= w <= 256, w % 4 == 0, 2 <= h <= 256 (so T <= 64 =
// 16 waves x 4 pair-rows and the level l0+1 matrix is at most 128 x 128 = 64 KB of LDS), 16-byte aligned prefixes.
// Arithmetic wraps like Go's int32 (coefficients of a decoder's input are arbitrary).

#define DEEP_WAVES 16
#define DEEP_PER 4
#define DEEP_SLOT_INTS (2 * DEEP_WAVES * 64 * 4)     /* slotE + slotD, one v4i per lane per wave */

// dev builds (tools/variant.sh stamp dwt53.hip -DJ2K_DEEP_STAMP): wave 0 of every workgroup records the constant-rate clock
// (100 MHz) at the phase boundaries; tools/deep_stamps.py prints the spans
#ifdef J2K_DEEP_STAMP
__device__ unsigned long long g_deep_stamp[2][1024][8];
__device__ unsigned long long g_deep_wstamp[256][16][4];      // forward, first LDS level: per wave {begin, end, after barrier}
#define DEEP_STAMP(dir, k) do { if (threadIdx.x == 0 && blockIdx.x < 1024) g_deep_stamp[dir][blockIdx.x][k] = wall_clock64(); } while (0)
#else
#define DEEP_STAMP(dir, k) do { } while (0)
#endif

typedef int deep_v2i __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) deep_v2i lds_v2i_t;
typedef __attribute__((address_space(1))) deep_v2i glb_v2i_t;
#ifdef J2K_DEEP_NOSTORE_L0
__device__ __forceinline__ void deep_st2(int32_t *p, int a, int b) { }                                                // dev timing variant: results are wrong
#else
__device__ __forceinline__ void deep_st2(int32_t *p, int a, int b) { *(glb_v2i_t *)p = (deep_v2i){a, b}; }          // memory
#endif
__device__ __forceinline__ void deep_st2_lds(int32_t *p, int a, int b) { *(lds_v2i_t *)p = (deep_v2i){a, b}; }

// job.col0: 0 = flat, 1 = deep (continues into the LDS levels), 3 = mid.  job.prow0 / job.nprow & 0xffff: the pair-rows of level
// l0 it COMPUTES (at most DEEP_WAVES * DEEP_PER).  job.nprow & DEEP_HAS_MID: the plane's top half is split once more --
// level l0+1 has T = ceil(ceil(h/2)/2) pair-rows (pair-row u = the two halves of level l0's low-pass row s_u) and only its first
// T1 = ceil(T/2) feed level l0+2, so
//   deep: level l0 pair-rows [0, T1+1) -> LDS rows 0 .. 2 T1 + 1 of the level l0+1 matrix, level l0+1 pair-rows [0, T1), then
//         every further level;   mid: level l0 pair-rows [T1-1, T) -> LDS rows 2 T1 - 2 .., level l0+1 pair-rows [T1, T), all
//         final;   flat: level l0 pair-rows [T, ceil(h/2)).
// Two pair-rows of level l0 are computed twice (T1-1 and T1); every output element is still written once (the high-pass rows of
// level l0 by the workgroup that owns them: deep t < T1, mid t >= T1).  This halves the deep workgroup's chain -- its load from
// memory (a CU takes in ~30 GB/s: 4.2 us for 130 KB), its level-l0 arithmetic and the largest LDS level (3-4 us of issue on one CU).
#define DEEP_HAS_MID 0x10000
#define DEEP_COMPACT 0x20000      /* inverse: the LDS levels' coefficients staged as compact runs (see dwt53_deep_inv_body) */
extern __shared__ __attribute__((aligned(16))) int32_t deep_lds[];
// A row of X_{l0} that dwt53_fwd_rgba8_wg16_kernel stored (st_scr16, dwt53_l0pix.inc): int16 in the first half of the row's int32-sized
// slot, four per lane in one 8-byte load, sign-extended.  Lanes past the row end load column 0 and are zeroed, as in load_cols.
typedef short deep_v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) deep_v4s glb_v4s_t;
__device__ __forceinline__ void deep_load_cols16(const int32_t *__restrict__ row, int c, int w, int (&x)[4]) {
    const bool in = c < w;
    const deep_v4s t = *(const glb_v4s_t *)(reinterpret_cast<const int16_t *>(row) + (in ? c : 0));
    x[0] = in ? (int)t.x : 0; x[1] = in ? (int)t.y : 0; x[2] = in ? (int)t.z : 0; x[3] = in ? (int)t.w : 0;
}
// S16: the level-l0 input rows are 16-bit (dwt53_deep_fwd16_kernel); everything behind the load is the same
template <bool S16 = false>
__device__ __forceinline__ void dwt53_deep_fwd_body(const DwtJob job, const TailPlane *__restrict__ planes,
                                                    const int32_t *__restrict__ scr, int32_t *__restrict__ coef) {
    const TailPlane P = planes[job.plane];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    v4i *slotE = reinterpret_cast<v4i *>(deep_lds), *slotD = slotE + DEEP_WAVES * 64;
    int w = P.w, h = P.h;
    const int halfW = w >> 1, halfH = (h + 1) >> 1;
    const int n_next = (P.nlev > 1) ? halfW * halfH : 0;
    const int kind = job.col0 & 0xff;
    const bool has_mid = (job.nprow & DEEP_HAS_MID) != 0;
    const int T = (halfH + 1) >> 1, T1 = (T + 1) >> 1;           // pair-rows of level l0+1; those of them that feed level l0+2
    // LDS: the rows of the level l0+1 matrix this workgroup holds start at row r0 of that matrix (bufA is addressed with the
    // matrix's own linear index through a biased pointer)
    const int r0 = (kind == 3) ? 2 * (T1 - 1) : 0;
    const int a_ints = has_mid ? (2 * T1 + 2) * halfW : n_next;
    // bufB (the level l0+2 matrix, written by level l0+1) lies over the exchange slots of level l0, which are dead by then: with
    // slots + bufA <= 80 KB two workgroups share a CU (deep + mid + flat jobs outnumber the CUs)
    int32_t *bufA = deep_lds + DEEP_SLOT_INTS, *bufB = deep_lds;
    int32_t *bufAb = bufA - r0 * halfW;
    const int ds_lo = (kind == 3) ? T1 : 0, ds_hi = (kind == 1 && has_mid) ? T1 : 0x7fffffff;     // whose high-pass rows of level l0 are mine
    const int32_t *src = scr + P.scr_off;
    int32_t *gout = coef + P.coef_off;
    const int c = lane * 4;
    const bool active = c < w;
    const int q_end = min(job.prow0 + (job.nprow & 0xffff), halfH);
    const int qa = job.prow0 + wave * DEEP_PER;
    const bool first = wave == 0 && job.prow0 > 0;                 // needs d of the pair-row above the job
    const bool lastw = qa < q_end && qa + DEEP_PER >= q_end;       // holds the job's last pair-row: loads the even row below it
    auto ldrow = [&](int r, int (&x)[4]) {
        if constexpr (S16) deep_load_cols16(src + (int64_t)min(max(r, 0), h - 1) * w, c, w, x);
        else load_cols<4, true>(src + (int64_t)min(max(r, 0), h - 1) * w, c, w, x);
    };
    DEEP_STAMP(0, 0);
    {
        int xe[DEEP_PER][4], xo[DEEP_PER][4], xa[4] = {0, 0, 0, 0}, xb[4] = {0, 0, 0, 0}, xn[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < DEEP_PER; i++) { ldrow(2 * (qa + i), xe[i]); ldrow(2 * (qa + i) + 1, xo[i]); }
        if (first) { ldrow(2 * qa - 2, xa); ldrow(2 * qa - 1, xb); }
        if (lastw) ldrow(2 * q_end, xn);
        int El[DEEP_PER][2], Eh[DEEP_PER][2], Ol[DEEP_PER][2], Oh[DEEP_PER][2];
#pragma unroll
        for (int i = 0; i < DEEP_PER; i++) { hfwd<4, true>(xe[i], c, w, El[i], Eh[i]); hfwd<4, true>(xo[i], c, w, Ol[i], Oh[i]); }
        slotE[wave * 64 + lane] = (v4i){El[0][0], El[0][1], Eh[0][0], Eh[0][1]};
        int Xl[2] = {0, 0}, Xh[2] = {0, 0};                        // E of the even row below the wave's last pair-row
        if (lastw) hfwd<4, true>(xn, c, w, Xl, Xh);
        int Pl[2] = {0, 0}, Ph[2] = {0, 0};                        // d of the pair-row above the wave's first
        if (first) {
            int Al[2], Ah[2], Bl[2], Bh[2];
            hfwd<4, true>(xa, c, w, Al, Ah); hfwd<4, true>(xb, c, w, Bl, Bh);
#pragma unroll
            for (int j = 0; j < 2; j++) { Pl[j] = wsub(Bl[j], avg1(Al[j], El[0][j])); Ph[j] = wsub(Bh[j], avg1(Ah[j], Eh[0][j])); }
        }
        __syncthreads();
        DEEP_STAMP(0, 1);
        if (!lastw && wave + 1 < DEEP_WAVES) {
            const v4i t = slotE[(wave + 1) * 64 + lane];
            Xl[0] = t.x; Xl[1] = t.y; Xh[0] = t.z; Xh[1] = t.w;
        }
        // predict (dwt.go:84-95 down the columns): d_q = o_q - ((e_q + e_{q+1}) >> 1); no row below: d_q = o_q - e_q
#pragma unroll
        for (int i = 0; i < DEEP_PER; i++) {
            const int q = qa + i;
            const bool has_next = 2 * q + 2 < h;
            const bool inner = (i + 1 < DEEP_PER) && (q + 1 < q_end);
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int nl = inner ? El[(i + 1) % DEEP_PER][j] : Xl[j], nh = inner ? Eh[(i + 1) % DEEP_PER][j] : Xh[j];
                Ol[i][j] = wsub(Ol[i][j], has_next ? avg1(El[i][j], nl) : El[i][j]);       // O becomes d
                Oh[i][j] = wsub(Oh[i][j], has_next ? avg1(Eh[i][j], nh) : Eh[i][j]);
            }
        }
        slotD[wave * 64 + lane] = (v4i){Ol[DEEP_PER - 1][0], Ol[DEEP_PER - 1][1], Oh[DEEP_PER - 1][0], Oh[DEEP_PER - 1][1]};
        lds_barrier();
        if (!first && wave > 0) {
            const v4i t = slotD[(wave - 1) * 64 + lane];
            Pl[0] = t.x; Pl[1] = t.y; Ph[0] = t.z; Ph[1] = t.w;
        }
        // update (dwt.go:99-114): s_q = e_q + ((d_{q-1} + d_q + 2) >> 2); d_{-1} := d_0; no odd row (odd h, last row): d_q := d_{q-1}
#pragma unroll
        for (int i = 0; i < DEEP_PER; i++) {
            const int q = qa + i;
            if (q >= q_end) break;
            const bool has_odd = 2 * q + 1 < h;
            int sl[2], sh[2];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                int dpl = Pl[j], dph = Ph[j];
                const int dcl = has_odd ? Ol[i][j] : dpl, dch = has_odd ? Oh[i][j] : dph;
                if (q == 0) { dpl = dcl; dph = dch; }
                sl[j] = wadd(El[i][j], avg2(dpl, dcl));
                sh[j] = wadd(Eh[i][j], avg2(dph, dch));
                Pl[j] = Ol[i][j]; Ph[j] = Oh[i][j];
            }
            if (active) {
                const int idxL = q * w + lane * 2, idxH = idxL + halfW;
                if (q * w < n_next) deep_st2_lds(bufAb + idxL, sl[0], sl[1]); else deep_st2(gout + idxL, sl[0], sl[1]);
                if (q * w + halfW < n_next) deep_st2_lds(bufAb + idxH, sh[0], sh[1]); else deep_st2(gout + idxH, sh[0], sh[1]);
                if (has_odd && q >= ds_lo && q < ds_hi) {
                    const int idxD = (halfH + q) * w + lane * 2;
                    deep_st2(gout + idxD, Ol[i][0], Ol[i][1]);
                    deep_st2(gout + idxD + halfW, Oh[i][0], Oh[i][1]);
                }
            }
        }
    }
    DEEP_STAMP(0, 2);
    if (kind == 0) return;                     // flat job: all of its output was final (uniform for the workgroup)
    lds_barrier();
    w = halfW; h = halfH;
    if (P.nlev > 1) {
        // level l0+1 on the rows held in LDS: its pair-rows [0, T1) (deep with a mid beside it), [T1, T) (mid), or all of them
        const int wn = (w + 1) >> 1, hn = (h + 1) >> 1;
        const int nn = (P.nlev == 2) ? 0 : wn * hn;
        const int ua = (kind == 3) ? T1 : 0, ub = (kind == 1 && has_mid) ? T1 : T;
#ifdef J2K_DEEP_STAMP
        if (lane == 0 && blockIdx.x < 256) g_deep_wstamp[blockIdx.x][wave][0] = wall_clock64();
#endif
        tail_fwd_level(bufAb, bufB, gout, w, h, nn, wave, lane, ua, ub);
#ifdef J2K_DEEP_STAMP
        if (lane == 0 && blockIdx.x < 256) g_deep_wstamp[blockIdx.x][wave][1] = wall_clock64();
#endif
        if (kind == 3) return;                 // mid job: everything it produced at level l0+1 was final
        lds_barrier();
        DEEP_STAMP(0, 3);
        w = wn; h = hn;
    }
    int32_t *cur = bufB, *nxt = bufA;
    for (int l = 2; l < P.nlev; l++) {
        const int wn = (w + 1) >> 1, hn = (h + 1) >> 1;
        const int nn = (l == P.nlev - 1) ? 0 : wn * hn;
        tail_fwd_level(cur, nxt, gout, w, h, nn, wave, lane);
        lds_barrier();
        DEEP_STAMP(0, 2 + l);
        int32_t *t = cur; cur = nxt; nxt = t;
        w = wn; h = hn;
    }
}

// (8 waves per SIMD = two workgroups per CU: deep + mid + flat jobs outnumber the CUs, and at one workgroup per CU the surplus
//  starts when the first finish -- stamps: the last flat job began 8 us into a 15 us kernel)
__global__ __launch_bounds__(64 * DEEP_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void dwt53_deep_fwd_kernel(const DwtJob *__restrict__ jobs, const TailPlane *__restrict__ planes,
                                                                         const int32_t *__restrict__ scr, int32_t *__restrict__ coef) {
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    dwt53_deep_fwd_body(job, planes, scr, coef);
}
// ... behind dwt53_fwd_rgba8_wg16_kernel: the rows of X_{l0} are int16 (deep_load_cols16)
__global__ __launch_bounds__(64 * DEEP_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void dwt53_deep_fwd16_kernel(const DwtJob *__restrict__ jobs, const TailPlane *__restrict__ planes,
                                                                           const int32_t *__restrict__ scr, int32_t *__restrict__ coef) {
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    dwt53_deep_fwd_body<true>(job, planes, scr, coef);
}

// S16 (dwt53_deep_inv16_kernel; option l0_scr16 bit 1): a wave that stores a row of X_{l0} -- it holds the whole row, four columns per lane --
// votes on "every value of the row fits int16".  If so the row goes out as int16 in the first half of its int32-sized slot (8 bytes per
// lane), else as int32 as ever; either way lane 0 writes the row's format byte (1 = int16) to fmt[(scr_off + row * w) >> 3] -- rows start
// at least 8 elements apart (w >= 8), so no two rows share a byte -- with an ordinary byte store.  Every row is stored once per call by one
// wave, so the table is rewritten whole on every call.  Exact for every input: a narrow row is one whose sign extension gives it back.
template <bool S16 = false>
__device__ __forceinline__ void dwt53_deep_inv_body(const DwtJob job, const TailPlane *__restrict__ planes,
                                                    const int32_t *__restrict__ coef, int32_t *__restrict__ scr, uint8_t *__restrict__ fmt = nullptr) {
    const TailPlane P = planes[job.plane];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int w = P.w, h = P.h;
    const int halfW = w >> 1, halfH = (h + 1) >> 1, nhigh = h - halfH;
    const int n_next = (P.nlev > 1) ? halfW * halfH : 0;
    const int kind = job.col0 & 0xff;
    const bool has_mid = (job.nprow & DEEP_HAS_MID) != 0;
    const int T = (halfH + 1) >> 1, T1 = (T + 1) >> 1;           // pair-rows of level l0+1; those of them whose input comes from level l0+2
    // Roles (see the forward kernel): deep rebuilds levels L-1 .. l0+2, then pair-rows [0, T1+1) of level l0+1 (one more than its
    // own level-l0 rows need: e of the pair-row below), then pair-rows [0, T1) of level l0; mid rebuilds pair-rows [T1, T) of level
    // l0+1 -- whose inputs are all final coefficients -- and pair-rows [T1, T) of level l0; flat the rest of level l0.  With a mid
    // job there are no flat jobs: the deep and the mid job each take half of the plane's bottom rows of level l0 FIRST, while
    // their staging loads are in flight (job.col0 bits 8..15 = how many pair-rows, bits 16..23 = the first one's distance from T)
    // -- the launch's LDS size allows one workgroup per CU, so a third job per plane would have to wait for a CU.
    // LDS: bufA = the rows of X_{l0+1} this workgroup rebuilds (addressed with the matrix's own linear index through a biased
    // pointer) | bufB = X_{l0+2} | bufC = the staged coefficients of the LDS levels, at their own linear index; the exchange
    // slots of level l0 reuse bufC (dead by then: the level loop ends with a barrier)
    const int r0 = (kind == 3) ? 2 * T1 : 0;
    const int a_ints = has_mid ? (2 * T1 + 2) * halfW : n_next;
    // Round 4, DEEP_COMPACT (deep + mid + flat jobs): the staged coefficients no longer sit at their own linear index (a 64 KB image of
    // the level l0+1 matrix with a hole in the middle) but in the places that are free when they are needed, so that a workgroup needs
    // <= 80 KB and TWO share a CU (the mid and flat jobs no longer wait for a CU):
    //   coefficients of levels >= l0+2 (indices below nn = |X_{l0+2}|)  -> the top end of bufA, which level l0+1 overwrites only after they are dead
    //   low-pass rows of level l0+1 beyond them (deep: rows nn / halfW .. T1+1; mid: rows T1 .. T-1)  -> region X behind bufB (mid: at X itself)
    //   high-pass rows of level l0+1 (deep: pair-rows 0 .. T1+1; mid: T1-1 ..)                        -> region RB
    // pc_deep / pc_lo / pc_hi are those three places as BIASED pointers (indexed with the coefficient's own linear index); the level
    // routines read low-pass and high-pass rows through separate bases.  Level l0's exchange slots reuse region X.
    const bool compact = (job.nprow & DEEP_COMPACT) != 0;
    const int nn1 = (P.nlev > 2) ? ((halfW + 1) >> 1) * ((halfH + 1) >> 1) : 0;
    int32_t *bufA = deep_lds;
    const int a4 = (a_ints + 3) & ~3, n2_4 = ((((halfW + 1) >> 1) * ((halfH + 1) >> 1)) + 3) & ~3;
    int32_t *bufB = bufA + a4;
    int32_t *bufC = bufB + n2_4;
    const int32_t *pc_deep = bufC, *pc_lo = bufC, *pc_hi = bufC;
    v4i *slotE = reinterpret_cast<v4i *>(bufC);
    if (compact) {
        const int lowtail = max(min(T1 + 2, T) * halfW - nn1, 0), lowmid = (T - T1) * halfW;
        const int xsize = (max(max(n2_4 + lowtail, lowmid), DEEP_WAVES * 64 * 4) + 3) & ~3;
        int32_t *X = bufB, *RB = X + xsize;
        slotE = reinterpret_cast<v4i *>(X);
        if (kind == 1) { pc_deep = bufA + (a_ints - nn1); pc_lo = X + n2_4 - nn1; pc_hi = RB - T * halfW; }
        else { pc_lo = X - T1 * halfW; pc_hi = RB - (T + T1 - 1) * halfW; }
        bufC = nullptr;
    }
    if (kind == 0) slotE = reinterpret_cast<v4i *>(deep_lds);      // a flat job has nothing but the exchange slots (the launch's LDS may be smaller than bufA + bufB)
    int32_t *bufAb = bufA - r0 * halfW;
    const int32_t *gcoef = coef + P.coef_off;
    int32_t *dst = scr + P.scr_off;
    const int c = lane * 4;
    const bool active = c < w;
    const int l2 = active ? lane * 2 : 0;                          // idle lanes load a valid address
    // The coefficients of the LDS levels are two runs of rows of the level l0+1 matrix (halfW wide, halfH rows: low-pass rows
    // 0 .. T-1, high-pass rows T ..): everything for a deep job without a mid beside it; low-pass rows [0, T1+2) and high-pass
    // rows of pair-rows [0, T1+2) for a deep job with one; low-pass rows [T1, T) and high-pass rows of pair-rows [T1-1, ..) for
    // the mid job.  Requested first (one sweep of the whole workgroup, up to four 16-byte loads per thread).
    const bool lds_levels = kind != 0 && P.nlev > 1;
    int ra0 = 0, ra1 = halfH, rb0 = 0, rb1 = 0;                    // row runs [ra0, ra1) and [rb0, rb1) of the level l0+1 matrix
    if (has_mid && kind == 1) { ra1 = min(T1 + 2, T); rb0 = T; rb1 = min(T + T1 + 2, halfH); }
    if (kind == 3) { ra0 = T1; ra1 = T; rb0 = T + T1 - 1; rb1 = halfH; }
    constexpr int NSTG = 4;
    int4 stg[NSTG];
    const int na4 = (ra1 - ra0) * halfW / 4, nb4 = (rb1 - rb0) * halfW / 4;
    const bool stg_vec = (halfW & 3) == 0 && na4 + nb4 <= NSTG * 64 * DEEP_WAVES;
    auto stg_idx4 = [&](int i) { return i < na4 ? ra0 * halfW / 4 + i : rb0 * halfW / 4 + (i - na4); };      // int4 index in the plane
    if (lds_levels && stg_vec) {
#pragma unroll
        for (int k = 0; k < NSTG; k++) {
            const int i = threadIdx.x + k * 64 * DEEP_WAVES;
            stg[k] = (i < na4 + nb4) ? reinterpret_cast<const int4 *>(gcoef)[stg_idx4(i)] : make_int4(0, 0, 0, 0);
        }
    }
    auto ldg2 = [&](int64_t idx, int (&v)[2]) { const deep_v2i t = *(const glb_v2i_t *)(gcoef + idx + l2); v[0] = t.x; v[1] = t.y; };
    auto ld_d = [&](int q, int (&lo)[2], int (&hi)[2]) {
        const int64_t row = (int64_t)(halfH + min(max(q, 0), nhigh - 1)) * w;
        ldg2(row, lo); ldg2(row + halfW, hi);
    };
    // low-pass rows: elements below n_next come from the coarser level's result (LDS), the rest from the coefficient plane;
    // uniform per half-row (n_next is a multiple of w / 2)
    auto ld_s = [&](int q, int (&lo)[2], int (&hi)[2]) {
        const int row = min(max(q, 0), halfH - 1) * w;
        if (row < n_next) { const deep_v2i t = *(const lds_v2i_t *)(bufAb + row + l2); lo[0] = t.x; lo[1] = t.y; }
        else ldg2(row, lo);
        if (row + halfW < n_next) { const deep_v2i t = *(const lds_v2i_t *)(bufAb + row + halfW + l2); hi[0] = t.x; hi[1] = t.y; }
        else ldg2(row + halfW, hi);
    };
    // undo update (dwt.go:132-138): e_q = s_q - ((d_{q-1} + d_q + 2) >> 2); d_{-1} := d_0; no d_q (odd h, last row): d_q := d_{q-1}
    auto undo_update = [&](int q, int (&sl)[2], int (&sh)[2], const int (&pl)[2], const int (&ph)[2], const int (&dl)[2], const int (&dh)[2]) {
        const bool has_d = q < nhigh;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            int al = pl[j], ah = ph[j];
            const int bl = has_d ? dl[j] : al, bh = has_d ? dh[j] : ah;
            if (q == 0) { al = bl; ah = bh; }
            sl[j] = wsub(sl[j], avg2(al, bl));
            sh[j] = wsub(sh[j], avg2(ah, bh));
        }
    };
    // pair-rows [p0, p0 + np) of level l0: every row they need requested at once, the vertical steps with one LDS exchange (e of
    // the pair-row below), then the horizontal inverse of each row
    [[maybe_unused]] auto st_row = [&](int r, const int (&x)[4]) {      // (S16 only: the int32 form keeps its own statements below)
        {
            const bool wide = active && ((x[0] != (int)(short)x[0]) | (x[1] != (int)(short)x[1]) | (x[2] != (int)(short)x[2]) | (x[3] != (int)(short)x[3]));
            const bool narrow = __builtin_amdgcn_ballot_w64(wide) == 0;       // wave-uniform
            if (narrow) {
                if (active) {
                    const unsigned lo = __builtin_amdgcn_perm((unsigned)x[1], (unsigned)x[0], 0x05040100u), hi = __builtin_amdgcn_perm((unsigned)x[3], (unsigned)x[2], 0x05040100u);
                    *(glb_v2i_t *)(reinterpret_cast<int16_t *>(dst + (int64_t)r * w) + c) = (deep_v2i){(int)lo, (int)hi};
                }
            } else if (active) *reinterpret_cast<int4 *>(dst + (int64_t)r * w + c) = make_int4(x[0], x[1], x[2], x[3]);
            if (lane == 0) fmt[(P.scr_off + (int64_t)r * w) >> 3] = narrow ? 1 : 0;
        }
    };
    auto level0_rows = [&](int p0, int np) {
        const int q_end = min(p0 + np, halfH);
        const int qa = p0 + wave * DEEP_PER;
        const bool lastw = qa < q_end && qa + DEEP_PER >= q_end;       // computes e of the pair-row below the range itself
        int Dl[DEEP_PER][2], Dh[DEEP_PER][2], Pl[2], Ph[2], Nl[2] = {0, 0}, Nh[2] = {0, 0};
#pragma unroll
        for (int i = 0; i < DEEP_PER; i++) ld_d(qa + i, Dl[i], Dh[i]);
        ld_d(qa - 1, Pl, Ph);
        if (lastw) ld_d(q_end, Nl, Nh);
        int Sl[DEEP_PER][2], Sh[DEEP_PER][2], Ml[2] = {0, 0}, Mh[2] = {0, 0};
#pragma unroll
        for (int i = 0; i < DEEP_PER; i++) ld_s(qa + i, Sl[i], Sh[i]);
        if (lastw) ld_s(q_end, Ml, Mh);
#pragma unroll
        for (int i = 0; i < DEEP_PER; i++) {
            if (i == 0) undo_update(qa, Sl[0], Sh[0], Pl, Ph, Dl[0], Dh[0]);
            else undo_update(qa + i, Sl[i], Sh[i], Dl[i - 1], Dh[i - 1], Dl[i], Dh[i]);      // S becomes e
        }
        if (lastw) {
            const int il = q_end - 1 - qa;           // the range's last pair-row, held by this wave
            int pl[2], ph[2];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                pl[j] = Dl[0][j]; ph[j] = Dh[0][j];
#pragma unroll
                for (int i = 1; i < DEEP_PER; i++) if (i == il) { pl[j] = Dl[i][j]; ph[j] = Dh[i][j]; }
            }
            undo_update(q_end, Ml, Mh, pl, ph, Nl, Nh);
        }
        slotE[wave * 64 + lane] = (v4i){Sl[0][0], Sl[0][1], Sh[0][0], Sh[0][1]};
        lds_barrier();
        if (!lastw && wave + 1 < DEEP_WAVES) {
            const v4i t = slotE[(wave + 1) * 64 + lane];
            Ml[0] = t.x; Ml[1] = t.y; Mh[0] = t.z; Mh[1] = t.w;
        }
        // undo predict (dwt.go:141-146): o_q = d_q + ((e_q + e_{q+1}) >> 1); no e_{q+1}: o_q = d_q + e_q; then the rows
#pragma unroll
        for (int i = 0; i < DEEP_PER; i++) {
            const int q = qa + i;
            if (q >= q_end) break;
            const bool has_next = q + 1 < halfH;
            const bool inner = (i + 1 < DEEP_PER) && (q + 1 < q_end);
            int x[4];
            hinv<4>(Sl[i], Sh[i], c, w, x);
            if constexpr (S16) st_row(2 * q, x);
            else if (active) *reinterpret_cast<int4 *>(dst + (int64_t)(2 * q) * w + c) = make_int4(x[0], x[1], x[2], x[3]);
            if (2 * q + 1 < h) {
                int ol[2], oh[2];
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int nl = inner ? Sl[(i + 1) % DEEP_PER][j] : Ml[j], nh = inner ? Sh[(i + 1) % DEEP_PER][j] : Mh[j];
                    ol[j] = wadd(Dl[i][j], has_next ? avg1(Sl[i][j], nl) : Sl[i][j]);
                    oh[j] = wadd(Dh[i][j], has_next ? avg1(Sh[i][j], nh) : Sh[i][j]);
                }
                hinv<4>(ol, oh, c, w, x);
                if constexpr (S16) st_row(2 * q + 1, x);
                else if (active) *reinterpret_cast<int4 *>(dst + (int64_t)(2 * q + 1) * w + c) = make_int4(x[0], x[1], x[2], x[3]);
            }
        }
    };
    DEEP_STAMP(1, 0);
    const int fl_n = (job.col0 >> 8) & 0xff, fl_0 = T + ((job.col0 >> 16) & 0xff);
    if (fl_n > 0) {
        level0_rows(fl_0, fl_n);               // rows that depend on no coarser level: in the shadow of the staging loads
        lds_barrier();                         // (their exchange slots lie in bufC, which the staged coefficients are about to fill)
    }
    if (lds_levels) {
        // levels L-1 .. l0+1 inside LDS as dwt53_tail_inv_kernel runs them, with their coefficients staged into LDS first: a
        // level that fetched its own coefficients paid a memory round trip per level (stamps: 3.2 / 2.6 / 4.0 us for levels of
        // 32 / 64 / 128 columns)
        auto dim = [](int v, int l) { for (int i = 0; i < l; i++) v = (v + 1) >> 1; return v; };
        if (stg_vec) {
#pragma unroll
            for (int k = 0; k < NSTG; k++) {
                const int i = threadIdx.x + k * 64 * DEEP_WAVES;
                if (i < na4 + nb4) {
                    const int e = 4 * stg_idx4(i);                 // the piece's linear index in the plane; runs and nn are multiples of 4
                    const int32_t *base = e < nn1 ? pc_deep : (i < na4 ? pc_lo : pc_hi);
                    *(__attribute__((address_space(3))) v4i *)(const_cast<int32_t *>(base) + e) = (v4i){stg[k].x, stg[k].y, stg[k].z, stg[k].w};
                }
            }
        } else {
            for (int i = threadIdx.x; i < (ra1 - ra0) * halfW; i += 64 * DEEP_WAVES) {
                const int e = ra0 * halfW + i;
                const_cast<int32_t *>(e < nn1 ? pc_deep : pc_lo)[e] = gcoef[e];
            }
            for (int i = threadIdx.x; i < (rb1 - rb0) * halfW; i += 64 * DEEP_WAVES) const_cast<int32_t *>(pc_hi)[rb0 * halfW + i] = gcoef[rb0 * halfW + i];
        }
        __syncthreads();
        for (int l = P.nlev - 1; l >= 2 && kind == 1; l--) {
            const int wl = dim(w, l), hl = dim(h, l);
            const int nn = (l == P.nlev - 1) ? 0 : ((wl + 1) >> 1) * ((hl + 1) >> 1);
            const int32_t *prev = ((l + 1) & 1) ? bufA : bufB;
            int32_t *d2 = (l & 1) ? bufA : bufB;
            tail_inv_level(prev, pc_deep, d2, wl, hl, nn, wave, lane, true, true);
            lds_barrier();
            DEEP_STAMP(1, l);
        }
        {
            // level l0+1: its pair-rows [0, T1+1) (deep with a mid beside it), [T1, T) (mid), or all of them
            const int nn = (P.nlev == 2) ? 0 : ((halfW + 1) >> 1) * ((halfH + 1) >> 1);
            const int ua = (kind == 3) ? T1 : 0, ub = (kind == 1 && has_mid) ? min(T1 + 1, T) : T;
            tail_inv_level(bufB, pc_lo, pc_hi, bufAb, halfW, halfH, nn, wave, lane, true, true, ua, ub);
            lds_barrier();
            DEEP_STAMP(1, 1);
        }
    }
    level0_rows(job.prow0, job.nprow & 0xffff);
    DEEP_STAMP(1, 7);
}

__global__ __launch_bounds__(64 * DEEP_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void dwt53_deep_inv_kernel(const DwtJob *__restrict__ jobs, const TailPlane *__restrict__ planes,
                                                                         const int32_t *__restrict__ coef, int32_t *__restrict__ scr) {
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    dwt53_deep_inv_body(job, planes, coef, scr);
}
// ... in front of dwt53_inv_rgba8_wg16_kernel: rows of X_{l0} that fit are stored as int16, fmt says which (the body's st_row)
__global__ __launch_bounds__(64 * DEEP_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void dwt53_deep_inv16_kernel(const DwtJob *__restrict__ jobs, const TailPlane *__restrict__ planes,
                                                                           const int32_t *__restrict__ coef, int32_t *__restrict__ scr, uint8_t *__restrict__ fmt) {
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    dwt53_deep_inv_body<true>(job, planes, coef, scr, fmt);
}

// ================================================================================================================
// The deep levels and HALF OF LEVEL 0 in one launch (packed RGBA8 frames).  The deep workgroups' chain (memory -> level 1 ->
// three LDS levels) keeps 120 CUs busy at a fraction of their bandwidth for ~13 us, and it depends only on the low-pass rows of
// the TOP half of every level-0 plane (the prefix that is level 1's input).  The bottom half of level 0 -- 66 MB of pure
// streaming whose output is all final -- depends on nothing the deep levels produce or consume.  So the forward transform is
//     launch A: level 0, top bands (dwt53_fwd_rgba8_wg_kernel: the rows whose low-pass halves feed level 1)
//     launch B: this kernel -- deep + flat workgroups (levels >= 1, as dwt53_deep_fwd_kernel) AND the level-0 bottom bands,
//               16 waves = 15 pair-rows per workgroup on the same dynamic LDS (job.col0 == 2)
// and the inverse is the mirror image: launch A' = deep levels + level-0 bottom bands (which read no coarser-level output),
// launch B' = level-0 top bands.  Same bytes, same kernels' arithmetic; the bandwidth-bound half of level 0 runs in the
// shadow of the latency-bound chain instead of after / before it.
// ================================================================================================================
__global__ __launch_bounds__(64 * DEEP_WAVES) void dwt53_mega_fwd_kernel(const DwtJob *__restrict__ jobs, const TailPlane *__restrict__ tplanes,
                                                                         const DwtPlane *__restrict__ l0planes, const int32_t *__restrict__ scr,
                                                                         int32_t *__restrict__ coef, const uint32_t *__restrict__ pix,
                                                                         int32_t *__restrict__ nxt0, int dc_shift, int pix_stride) {
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    if ((job.col0 & 0xff) == 2) {
        dwt53_fwd_rgba8_wg_body<DEEP_WAVES, 1>(*reinterpret_cast<v4i (*)[DEEP_WAVES][6][64]>(deep_lds), job, l0planes, pix, coef, nxt0, dc_shift, pix_stride);
        return;
    }
    dwt53_deep_fwd_body(job, tplanes, scr, coef);
}
__global__ __launch_bounds__(64 * DEEP_WAVES) void dwt53_mega_inv_kernel(const DwtJob *__restrict__ jobs, const TailPlane *__restrict__ tplanes,
                                                                         const DwtPlane *__restrict__ l0planes, const int32_t *__restrict__ coef,
                                                                         int32_t *__restrict__ scr, const int32_t *__restrict__ prev0,
                                                                         uint32_t *__restrict__ pix, int dc_shift, int pix_stride) {
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    if ((job.col0 & 0xff) == 2) {
        dwt53_inv_rgba8_wg_body<DEEP_WAVES, false>(*reinterpret_cast<v4i (*)[DEEP_WAVES][6][64]>(deep_lds), job, l0planes, coef, prev0, pix, dc_shift, pix_stride);
        return;
    }
    dwt53_deep_inv_body(job, tplanes, coef, scr);
}

#ifdef J2K_DEEP_STAMP
extern "C" int j2k_dev_deep_stamps(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_deep_stamp), sizeof(g_deep_stamp)); }
extern "C" int j2k_dev_deep_wstamps(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_deep_wstamp), sizeof(g_deep_wstamp)); }
#endif

hipError_t launch_dwt53_deep_fwd(hipStream_t s, const DwtJob *jobs, int njobs, const TailPlane *planes, size_t lds_bytes, const int32_t *scr,
                                 int32_t *coef, hipEvent_t ev0, hipEvent_t ev1, int scr16) {
    if (njobs <= 0) return hipSuccess;
    if (scr16) {               // the level-0 launch of this call stored the rows of `scr` as int16 (dwt53_fwd_rgba8_wg16_kernel)
        static bool attr16_done = false;
        if (!attr16_done) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dwt53_deep_fwd16_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
            if (e != hipSuccess) return e;
            attr16_done = true;
        }
        hipExtLaunchKernelGGL(dwt53_deep_fwd16_kernel, dim3(njobs), dim3(64 * DEEP_WAVES), lds_bytes, s, ev0, ev1, 0, jobs, planes, scr, coef);
        return hipGetLastError();
    }
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dwt53_deep_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    hipExtLaunchKernelGGL(dwt53_deep_fwd_kernel, dim3(njobs), dim3(64 * DEEP_WAVES), lds_bytes, s, ev0, ev1, 0, jobs, planes, scr, coef);
    return hipGetLastError();
}
hipError_t launch_dwt53_deep_inv(hipStream_t s, const DwtJob *jobs, int njobs, const TailPlane *planes, size_t lds_bytes, const int32_t *coef,
                                 int32_t *scr, hipEvent_t ev0, hipEvent_t ev1, uint8_t *scr16_fmt) {
    if (njobs <= 0) return hipSuccess;
    if (scr16_fmt) {           // the level-0 launch of this call is dwt53_inv_rgba8_wg16_kernel: rows that fit go out as int16, scr16_fmt says which
        static bool attr16_done = false;
        if (!attr16_done) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dwt53_deep_inv16_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
            if (e != hipSuccess) return e;
            attr16_done = true;
        }
        hipExtLaunchKernelGGL(dwt53_deep_inv16_kernel, dim3(njobs), dim3(64 * DEEP_WAVES), lds_bytes, s, ev0, ev1, 0, jobs, planes, coef, scr, scr16_fmt);
        return hipGetLastError();
    }
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dwt53_deep_inv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    hipExtLaunchKernelGGL(dwt53_deep_inv_kernel, dim3(njobs), dim3(64 * DEEP_WAVES), lds_bytes, s, ev0, ev1, 0, jobs, planes, coef, scr);
    return hipGetLastError();
}

#define DEEP_L0_LDS_BYTES (DEEP_WAVES * 6 * 64 * 16)      /* the level-0 role's exchange slots */
hipError_t launch_dwt53_mega_fwd(hipStream_t s, const DwtJob *jobs, int njobs, const TailPlane *tplanes, const DwtPlane *l0planes, size_t lds_bytes,
                                 const int32_t *scr, int32_t *coef, const uint32_t *pix, int32_t *nxt0, int dc_shift, int pix_stride,
                                 hipEvent_t ev0, hipEvent_t ev1) {
    if (njobs <= 0) return hipSuccess;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dwt53_mega_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    lds_bytes = std::max(lds_bytes, (size_t)DEEP_L0_LDS_BYTES);
    hipExtLaunchKernelGGL(dwt53_mega_fwd_kernel, dim3(njobs), dim3(64 * DEEP_WAVES), lds_bytes, s, ev0, ev1, 0, jobs, tplanes, l0planes, scr, coef, pix, nxt0,
                          dc_shift, pix_stride);
    return hipGetLastError();
}
hipError_t launch_dwt53_mega_inv(hipStream_t s, const DwtJob *jobs, int njobs, const TailPlane *tplanes, const DwtPlane *l0planes, size_t lds_bytes,
                                 const int32_t *coef, int32_t *scr, const int32_t *prev0, uint32_t *pix, int dc_shift, int pix_stride,
                                 hipEvent_t ev0, hipEvent_t ev1) {
    if (njobs <= 0) return hipSuccess;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dwt53_mega_inv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    lds_bytes = std::max(lds_bytes, (size_t)DEEP_L0_LDS_BYTES);
    hipExtLaunchKernelGGL(dwt53_mega_inv_kernel, dim3(njobs), dim3(64 * DEEP_WAVES), lds_bytes, s, ev0, ev1, 0, jobs, tplanes, l0planes, coef, scr, prev0, pix,
                          dc_shift, pix_stride);
    return hipGetLastError();
}
