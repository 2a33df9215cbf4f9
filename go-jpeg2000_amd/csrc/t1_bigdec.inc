// t1_bigdec.inc -- T1.Decode (t1.go:1261-1410) for code-blocks above 64 x 64, up to 256 x 256: the reference's DEFAULT block size
// (encoder.go:606-607: 1 << (6 + 2)).  Included by t1.hip.
//
// Round 2/3 decoded these blocks with byte flags in LDS, the scans by all lanes and every decision on lane 0 of a divergent
// wavefront: 170 ns per decision, 135-170 ms for a 256 x 256 block of noise.  A block is ONE serial MQ chain whatever is done, so
// what counts is the instruction stream of that chain.  Here the whole decoder is WAVE-UNIFORM: one wavefront per block, every
// lane executes the same thing, so the compiler keeps the state machine on the scalar unit (s_ff1 / s_bitset / s_lshr_b64 on
// 64-bit row masks in SGPRs, real scalar branches, no exec-mask bookkeeping), at ~2.2 ns per dependent instruction
// (tools/probe/salu_lat.hip).  The vector unit is the memory of the chain:
//   * the MQ state table (47 entries) and the current entry of each of the 19 contexts live across the LANES of two VGPRs
//     (v_readlane / v_writelane with a scalar index: ~13 ns, no LDS round trip of ~38 ns);
//   * the context look-ups are lane tables too: ZC context by the ADDITIVE index h + 3 v + 9 d (every neighbour adds a constant),
//     sign context by (hc + 2) + 5 (vc + 2);
//   * per 64-column word of a row (SigProp) or of a 4-row stripe (Cleanup) the lanes (= columns) compute the STATIC part of every
//     sample's indices from the row masks -- the neighbours that the pass cannot change before it gets there -- and the chain
//     fetches them with one v_readlane per sample / column and adds the few dynamic neighbours (W in SigProp; NW, W, SW, N in
//     Cleanup) itself.
// State per block in LDS: four 256-bit-per-row mask arrays (significant, negative, visited, refined) + the current plane's bits.
// Magnitudes are OR-ed into the output block once per plane by all lanes; signs applied at the end (t1.go:1281-1289).
// Compressed bytes: a 256-byte window across the lanes (bytes past the end read as 0xFF, which makes byteIn's marker branch do
// what its past-the-end branch does, mqc.go:402-439), eight bytes at a time in an SGPR pair.

// NWD words of 64 columns, RWS = rows + 2 (row y at index y + 1; the first and the last row stay zero): <4, 258> for blocks up to 256 x 256
// (33 KB: four per CU), <2, 130> for blocks up to 128 x 128 (8 KB) -- twelve of the 21 blocks of a 512 x 512 frame at the reference's
// default block size are of the second kind, and with batches of frames in flight LDS is what bounds the number of resident chains.
template <int NWD, int RWS>
struct T1BigDec {
    alignas(16) uint64_t S[RWS][NWD], NEG[RWS][NWD], VIS[RWS][NWD], REF[RWS][NWD];
    // (the bits a pass decodes go straight into the output block -- a predicated OR without a return value, one instruction for the 64
    //  columns of a row word, nothing for the chain to wait for -- instead of into a fifth array that a loop over the block emptied at
    //  the end of every plane: 41 -> 33 KB, four blocks of 256 x 256 per CU instead of three)
    uint8_t zct[64];                      // ZC context by h + 3 v + 9 d (this block's band); [45] = 0 so that index 44 + 1 reads defined memory
    uint8_t sct[32];                      // sign context | prediction << 3 by (hc + 2) + 5 (vc + 2)
    uint32_t wsimd[4], mqslot;            // the SIMD of each launched wave / the SIMD whose wave decodes (t1_big.inc: t1b_cu_key)
};

__device__ __forceinline__ uint32_t tbd_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t tbd_u64(uint64_t v) {
    // (the builtin returns int: without the casts the low word is sign-extended over the high one)
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32 | (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
}
// v_writelane_b32 (this compiler has no builtin for it): lane `sel` of `old` <- the scalar `val`.  The s_nop covers the gfx9 hazard
// "an SGPR written by a VALU instruction (v_readlane) used as a lane select needs 4 wait states", which the compiler cannot see
// inside inline asm.
__device__ __forceinline__ uint32_t tbd_writelane(uint32_t val, uint32_t sel, uint32_t old) {
    val = (uint32_t)__builtin_amdgcn_readfirstlane(val); sel = (uint32_t)__builtin_amdgcn_readfirstlane(sel);   // (free when the value is scalar already; an "s" operand the compiler holds in a VGPR is an assembler error)
    asm("s_mov_b32 m0, %2\n\ts_nop 3\n\tv_writelane_b32 %0, %1, m0" : "+v"(old) : "s"(val), "s"(sel) : "m0");   // (two SGPRs would break the constant-bus limit)
    return old;
}
// lutZCCtx (t1_luts.go:34-110) as a function of the counts: h = W + E, v = N + S, d = the four diagonals
__device__ __forceinline__ int tbd_zc_ctx(int band, int hh, int v, int d) {
    if (band == 1) { const int t = hh; hh = v; v = t; }
    if (band == 3) {
        const int hv = hh + v;
        if (hv >= 3) return 8;
        if (hv == 2) return d >= 2 ? 7 : (d >= 1 ? 6 : 5);
        if (hv == 1) return d >= 2 ? 4 : 3;
        return d >= 2 ? 2 : (d >= 1 ? 1 : 0);
    }
    if (hh == 2) return 8;
    if (hh == 1) return v >= 1 ? 7 : (d >= 1 ? 6 : 5);
    if (v == 2) return 4;
    if (v == 1) return d >= 1 ? 3 : 2;
    return d >= 2 ? 1 : 0;
}
// lutSignCtx | lutSignPred << 3 (t1_luts.go:153-230) as a function of the contributions hc, vc in -2..2 (same arithmetic as build_tables)
__device__ __forceinline__ int tbd_sc(int hc, int vc) {
    int pred = 0, sctx = 0;
    if (hc < 0) { pred = 1; hc = -hc; }
    if (hc == 0 && vc < 0) { pred = 1; vc = -vc; }
    if (hc == 1) sctx = vc == 1 ? 4 : (vc == 0 ? 2 : 1);
    else if (hc == 0) sctx = vc == 1 ? 1 : 0;
    else if (hc == 2) sctx = 3;
    return sctx | pred << 3;
}

// The wave-uniform MQ decoder (mqc.go:352-497).  Entry format: qe | nmps << 16 | nlps << 22 | switch << 28 | mps << 29.
struct MqUni {
    uint32_t A, C, CT;
    uint64_t win;            // the next bytes of the (0xFF-padded) stream, lowest byte first: byte(bp + 1), byte(bp + 2), ...
    uint32_t nwin;           // valid bytes in win
    uint32_t cur;            // byte(bp)
    uint32_t wpos;           // dword index (in the lane window) of the next refill
    uint32_t wbase;          // stream byte offset of lane 0 of the lane window
    uint32_t len;
    const uint8_t *data;
    uint32_t wv;             // VGPR: lane l = bytes wbase + 4 l .. + 3
    uint32_t entv;           // VGPR: lane c = entry of context c
    uint32_t tabv;           // VGPR: lane i = entry of state i (mps bit clear)
#ifdef J2K_TBD_TRACE
    uint16_t *trace; uint32_t tn, tcap;      // dev: (ctx | decision << 8) of every decision, in the output block instead of the coefficients
#endif
};
__device__ __forceinline__ uint32_t tbd_load_window(const uint8_t *data, uint32_t len, uint32_t base, int lane) {
    const uint32_t o = base + 4u * (uint32_t)lane;
    uint32_t v = 0xFFFFFFFFu;
    if (o + 4 <= len) {
        v = (uint32_t)data[o] | (uint32_t)data[o + 1] << 8 | (uint32_t)data[o + 2] << 16 | (uint32_t)data[o + 3] << 24;
    } else if (o < len) {
        v = 0;
        for (int b = 0; b < 4; b++) v |= (o + b < len ? (uint32_t)data[o + b] : 0xFFu) << (8 * b);
    }
    return v;
}
// refill `win` with eight more bytes (two dwords of the lane window; the window itself every 256 bytes)
__device__ __forceinline__ void tbd_refill(MqUni &q, int lane) {
    if (q.wpos >= 64) {
        q.wbase += 256;
        q.wv = tbd_load_window(q.data, q.len, q.wbase, lane);
        q.wpos = 0;
    }
    const uint32_t lo = __builtin_amdgcn_readlane(q.wv, q.wpos), hi = __builtin_amdgcn_readlane(q.wv, q.wpos + 1);
    q.win = (uint64_t)hi << 32 | lo;
    q.nwin = 8;
    q.wpos += 2;
}
__device__ __forceinline__ void tbd_byte_in(MqUni &q, int lane) {      // mqc.go:402-439 on the padded stream
    if (q.nwin == 0) tbd_refill(q, lane);
    const uint32_t next = (uint32_t)q.win & 0xFFu;
    if (q.cur == 0xFF) {
        if (next > 0x8F) { q.C += 0xFF00; q.CT = 8; return; }
        q.C += next << 9; q.CT = 7;
    } else { q.C += next << 8; q.CT = 8; }
    q.cur = next; q.win >>= 8; q.nwin--;
}
__device__ __forceinline__ void tbd_mq_init(MqUni &q, const uint8_t *data, uint32_t len, int lane) {   // NewMQDecoder mqc.go:370-399
    q.data = data; q.len = len; q.wbase = 0; q.wpos = 0;
    q.wv = tbd_load_window(data, len, 0, lane);
    tbd_refill(q, lane);
    q.cur = (uint32_t)q.win & 0xFFu; q.win >>= 8; q.nwin--;            // byte(0); win now starts at byte(1)
    q.C = q.cur << 16;
    tbd_byte_in(q, lane);
    q.C <<= 7; q.CT -= 7; q.A = 0x8000;
}
__device__ __forceinline__ uint32_t tbd_decode_(MqUni &q, uint32_t ctx, int lane);
__device__ __forceinline__ uint32_t tbd_decode(MqUni &q, uint32_t ctx, int lane) {
    const uint32_t d = tbd_decode_(q, ctx, lane);
#ifdef J2K_TBD_TRACE
    if (q.tn < q.tcap) q.trace[q.tn] = (uint16_t)(ctx | d << 8);
    q.tn++;
#endif
    return d;
}
__device__ __forceinline__ uint32_t tbd_decode_(MqUni &q, uint32_t ctx, int lane) {   // mqc.go:443-497
    const uint32_t en = __builtin_amdgcn_readlane(q.entv, ctx);
    const uint32_t qe = en & 0xFFFFu, mps = (en >> 29) & 1u;
    const uint32_t A1 = q.A - qe;
    // 0 / 1 flags by subtraction and shift, not by comparison: a comparison is an i1 to the compiler, which keeps uniform i1 values as
    // 64-bit lane masks and sends them through v_cndmask / v_readfirstlane when they meet an integer (both operands are below 2^16)
    // (and the difference goes through an empty asm: the compiler otherwise recognises the idiom and turns it back into a comparison)
    uint32_t dreg = (q.C >> 16) - qe;
    asm("" : "+s"(dreg));
    const uint32_t reg = dreg >> 31;                          // the code value is in the LPS sub-interval: (C >> 16) < qe
    if (((A1 >> 15) & (reg ^ 1u)) != 0) { q.C -= qe << 16; q.A = A1; return mps; }      // MPS, no renormalisation
    uint32_t dlt = A1 - qe;
    asm("" : "+s"(dlt));
    const uint32_t lt = dlt >> 31;                            // A1 < qe
    const uint32_t lps = reg ^ lt;                            // conditional exchange (mqc.go:452-481)
    const uint32_t ni = (en >> (16u + 6u * lps)) & 63u;       // nmps at bit 16, nlps at bit 22
    const uint32_t nmps_bit = mps ^ (lps & (en >> 28));
    const uint32_t ne = __builtin_amdgcn_readlane(q.tabv, ni) | nmps_bit << 29;
    q.entv = tbd_writelane(ne, ctx, q.entv);
    q.C -= (qe << 16) & (reg - 1u);
    const uint32_t A = A1 + ((qe - A1) & (0u - reg));         // reg ? qe : A1
    uint32_t n = (uint32_t)__builtin_clz(A) - 16u;            // A < 0x8000 here: 1..15 doublings (mqc.go:488-497)
    q.A = A << n;
    // the reference's bit-by-bit loop with a byte-in whenever CT is 0: the common case -- the shift fits the bits at hand -- first and
    // straight-line, the rest (a byte-in, then whatever is left; n <= 15 and a byte-in gives 7 or 8 bits) behind it
    if (q.CT == 0) tbd_byte_in(q, lane);
    uint32_t s = n < q.CT ? n : q.CT;
    q.C <<= s; q.CT -= s; n -= s;
    while (n) {
        tbd_byte_in(q, lane);
        s = n < q.CT ? n : q.CT;
        q.C <<= s; q.CT -= s; n -= s;
    }
    return mps ^ lps;
}

// From here on ONE wavefront works (rot = 1: the other three have returned), so what orders its LDS traffic is the wavefront's own
// program order plus the wait for the outstanding LDS operations -- not a workgroup barrier, which waves that have already ended
// would have to be left out of (ADVICE r4).
__device__ __forceinline__ void tbd_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
// Launched with 64 threads (rot = 0) or 256 (rot = 1): of four waves, one per SIMD, the one on the SIMD the CU's counter names
// decodes and the other three leave at once -- two chains of dependent scalar instructions on one SIMD run at half speed each
// (t1_big.inc, "Where the MQ chain runs").
template <int NWD, int RWS>
__global__ __launch_bounds__(256) void t1_decode_big_kernel(const BlockJob *__restrict__ jobs, int njobs, const uint8_t *__restrict__ stream,
                                                           const uint64_t *__restrict__ offs, const uint32_t *__restrict__ lens,
                                                           const uint8_t *__restrict__ numbps, int32_t *__restrict__ decoded, int rot, int all_sizes, int skip_uniform, const uint8_t *__restrict__ floors) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tbd_lds[];
    T1BigDec<NWD, RWS> &F = *reinterpret_cast<T1BigDec<NWD, RWS> *>(tbd_lds);
    const int jid = blockIdx.x;
    if (jid >= njobs) return;
    const int skip_planes = t1_floor_of(skip_uniform, floors, jid);       // this block's floor: the call's, or its own if that is higher
    const BlockJob J = jobs[jid];
    const int w = (int)tbd_u((uint32_t)J.w), h = (int)tbd_u((uint32_t)J.h);
    if ((w <= 64 && h <= 64) || w > 256 || h > 256) return;       // t1_decode64_kernel / the general kernel take these
    if (!all_sizes && (w <= 128 && h <= 128) != (NWD == 2)) return;   // the other instantiation's (all_sizes: the large state serves every block)
    const int lane = threadIdx.x & 63;
    if (rot) {
        const int wv = (int)tbd_u(threadIdx.x >> 6);
        if (lane == 0) F.wsimd[wv] = t1b_simd_id();
        if (threadIdx.x == 0) F.mqslot = atomicAdd(&g_t1b_cu_rot[t1b_cu_key()], 1u) & 3u;
        __syncthreads();
        int mine = 0;
        for (int k = 3; k >= 0; k--) if (F.wsimd[k] == F.mqslot) mine = k;
        if (wv != (int)tbd_u((uint32_t)mine)) return;
    }
    const int nw = (w + 63) >> 6;
    int32_t *out = decoded + J.out_off;
    // ---- tables across the lanes; state cleared ----
    MqUni q;
    {
        const int i = lane < 47 ? lane : 46;
        q.tabv = (uint32_t)c_iso_qe[i] | (uint32_t)c_iso_nmps[i] << 16 | (uint32_t)c_iso_nlps[i] << 22 | (uint32_t)c_iso_switch[i] << 28;
        const int st0 = lane == CtxUni ? 46 : 0;                    // contexts start at state 0, UNI at 46 (mqc.go:135-166)
        q.entv = (uint32_t)c_iso_qe[st0] | (uint32_t)c_iso_nmps[st0] << 16 | (uint32_t)c_iso_nlps[st0] << 22 | (uint32_t)c_iso_switch[st0] << 28;
        if (lane < 45) F.zct[lane] = (uint8_t)tbd_zc_ctx(J.band, lane % 3, (lane / 3) % 3, lane / 9);
        if (lane < 25) F.sct[lane] = (uint8_t)tbd_sc(lane % 5 - 2, lane / 5 - 2);
    }
    {
        uint64_t *z = &F.S[0][0];
        for (int i = lane; i < 4 * RWS * NWD; i += 64) z[i] = 0;     // S, NEG, VIS, REF are contiguous
    }
    for (size_t i = lane; i < (size_t)w * h; i += 64) out[i] = 0;
    tbd_wave_sync();
    const uint32_t zcv = lane < 45 ? F.zct[lane] : 0u;              // VGPR: lane idx = ZC context of the additive index
    const uint32_t scv = lane < 25 ? F.sct[lane] : 0u;              // VGPR: lane idx = sign context | prediction << 3
    {
        const uint64_t o = tbd_u64(offs[jid]);
        tbd_mq_init(q, stream + o, tbd_u(lens[jid]), lane);
    }
    const int nb = (int)tbd_u((uint32_t)numbps[jid]);
#ifdef J2K_TBD_TRACE
    q.trace = reinterpret_cast<uint16_t *>(out); q.tn = 0; q.tcap = 2u * (uint32_t)(w * h);
#endif
    const uint64_t lastmask = (w & 63) ? ((1ull << (w & 63)) - 1) : ~0ull;      // valid columns of the last word
    // the samples of row y, word k whose bit of plane `bit` is 1 (t1.go:1311, 1345, 1394: first significance sets the magnitude to the
    // bit, refinement ORs it in -- the same OR on a block that starts as zeros)
    auto emit = [&](int y, int k, uint64_t ones, int32_t bit) {
#ifndef J2K_TBD_TRACE
        if ((ones >> lane) & 1) atomicOr(reinterpret_cast<unsigned int *>(out) + (size_t)y * w + 64 * k + lane, (unsigned int)bit);
#endif
    };

    const int floor_bp = (int)tbd_u((uint32_t)skip_planes);       // the quality floor (j2k_*_coarse): planes below it stay undecoded
    for (int bp = nb - 1; bp >= floor_bp; bp--) {
        const int32_t bit = bp < 32 ? (int32_t)(1u << bp) : 0;
        // =================== significance propagation (t1.go:1295-1319): raster order ===================
        for (int y = 0; y < h; y++) {
            const int r = y + 1;
            uint64_t prevS = 0, prevN = 0;                            // word k - 1 of this row, as updated by this pass
            for (int k = 0; k < nw; k++) {
                const uint64_t colmask = k == nw - 1 ? lastmask : ~0ull;
                const uint64_t Sc = tbd_u64(F.S[r][k]);
                const uint64_t Su = tbd_u64(F.S[r - 1][k]), Sd = tbd_u64(F.S[r + 1][k]);
                const uint64_t ScN = k + 1 < NWD ? tbd_u64(F.S[r][k + 1]) : 0, SuN = k + 1 < NWD ? tbd_u64(F.S[r - 1][k + 1]) : 0, SdN = k + 1 < NWD ? tbd_u64(F.S[r + 1][k + 1]) : 0;
                const uint64_t SuP = k > 0 ? tbd_u64(F.S[r - 1][k - 1]) : 0, SdP = k > 0 ? tbd_u64(F.S[r + 1][k - 1]) : 0;
                const uint64_t upL = Su << 1 | SuP >> 63, upR = Su >> 1 | SuN << 63;
                const uint64_t dnL = Sd << 1 | SdP >> 63, dnR = Sd >> 1 | SdN << 63;
                const uint64_t curL = Sc << 1 | prevS >> 63, curR = Sc >> 1 | ScN << 63;
                const uint64_t HN = upL | Su | upR | dnL | Sd | dnR | curL | curR;
                uint64_t cand = ~Sc & HN & colmask;
                if (cand == 0) { prevS = Sc; prevN = tbd_u64(F.NEG[r][k]); continue; }
                const uint64_t Nc = tbd_u64(F.NEG[r][k]), Nu = tbd_u64(F.NEG[r - 1][k]), Nd = tbd_u64(F.NEG[r + 1][k]);
                const uint64_t NcN = k + 1 < NWD ? tbd_u64(F.NEG[r][k + 1]) : 0;
                // lanes = columns: the static part of every sample's indices (everything but W)
                uint32_t cx;
                {
                    const uint32_t e = (uint32_t)(curR >> lane) & 1u, n_ = (uint32_t)(Su >> lane) & 1u, s_ = (uint32_t)(Sd >> lane) & 1u;
                    const uint32_t dg = ((uint32_t)(upL >> lane) & 1u) + ((uint32_t)(upR >> lane) & 1u) + ((uint32_t)(dnL >> lane) & 1u) + ((uint32_t)(dnR >> lane) & 1u);
                    const uint32_t zi = e + 3u * (n_ + s_) + 9u * dg;
                    const uint32_t zc01 = (uint32_t)F.zct[zi] | (uint32_t)F.zct[zi + 1] << 4;      // the ZC context without / with a significant W
                    const uint32_t en_ = (uint32_t)((Nc >> 1 | NcN << 63) >> lane) & 1u, nn = (uint32_t)(Nu >> lane) & 1u, sn = (uint32_t)(Nd >> lane) & 1u;
                    const int hc = (int)e - 2 * (int)(e & en_), vc = (int)n_ - 2 * (int)(n_ & nn) + (int)s_ - 2 * (int)(s_ & sn);
                    cx = zc01 | (uint32_t)(hc + 5 * vc + 12) << 8;     // (hc + 2) + 5 (vc + 2) without W's contribution
                }
                uint64_t newsig = 0, newneg = 0, vis = 0;
                uint64_t WS = curL, WN = Nc << 1 | prevN >> 63;         // W neighbour of column x at bit x: significance / sign
                do {
                    const uint32_t x = (uint32_t)__builtin_ctzll(cand);
                    const uint64_t bx = 1ull << x;
                    cand &= ~bx; vis |= bx;
                    const uint32_t cv = __builtin_amdgcn_readlane(cx, x);
                    const uint32_t wb = (uint32_t)(WS >> x) & 1u;
                    const uint32_t zc = (cv >> (4u * wb)) & 15u;             // (both variants come with the lane's word: no second look-up on the chain)
                    if (tbd_decode(q, zc, lane)) {
                        const uint32_t wn = (uint32_t)(WN >> x) & 1u;
                        const uint32_t sv = __builtin_amdgcn_readlane(scv, (cv >> 8) + wb - 2u * (wb & wn));
                        const uint64_t sg = tbd_decode(q, CtxSC0 + (sv & 7u), lane) ^ (sv >> 3);
                        newsig |= bx; newneg |= sg << x;
                        WS |= bx << 1; WN |= (sg << x) << 1;
                        cand |= (bx << 1) & ~Sc & colmask;                // t1.go:1303: the right-hand neighbour now has a significant neighbour
                    }
                } while (cand);
                prevS = Sc | newsig; prevN = Nc | newneg;
                if (lane == 0) {
                    F.S[r][k] = prevS; F.NEG[r][k] = prevN; F.VIS[r][k] = vis;
                }
                if (newsig) emit(y, k, newsig, bit);
            }
        }
        // =================== magnitude refinement (t1.go:1331-1347): raster order ===================
        for (int y = 0; y < h; y++) {
            const int r = y + 1;
            for (int k = 0; k < nw; k++) {
                const uint64_t Sc = tbd_u64(F.S[r][k]);
                uint64_t M = Sc & ~tbd_u64(F.VIS[r][k]);
                if (M == 0) continue;
                const uint64_t R2 = tbd_u64(F.REF[r][k]);
                uint64_t m1 = 0;
                if (M & ~R2) {
                    const uint64_t Su = tbd_u64(F.S[r - 1][k]), Sd = tbd_u64(F.S[r + 1][k]);
                    const uint64_t ScN = k + 1 < NWD ? tbd_u64(F.S[r][k + 1]) : 0, SuN = k + 1 < NWD ? tbd_u64(F.S[r - 1][k + 1]) : 0, SdN = k + 1 < NWD ? tbd_u64(F.S[r + 1][k + 1]) : 0;
                    const uint64_t ScP = k > 0 ? tbd_u64(F.S[r][k - 1]) : 0, SuP = k > 0 ? tbd_u64(F.S[r - 1][k - 1]) : 0, SdP = k > 0 ? tbd_u64(F.S[r + 1][k - 1]) : 0;
                    m1 = (Su << 1 | SuP >> 63) | Su | (Su >> 1 | SuN << 63) | (Sd << 1 | SdP >> 63) | Sd | (Sd >> 1 | SdN << 63) |
                         (Sc << 1 | ScP >> 63) | (Sc >> 1 | ScN << 63);
                }
                const uint64_t M0 = M;
                uint64_t bits = 0;
                do {
                    const uint32_t x = (uint32_t)__builtin_ctzll(M);
                    M &= M - 1;
                    const uint32_t ctx = ((R2 >> x) & 1) ? CtxMag2 : (((m1 >> x) & 1) ? CtxMag1 : CtxMag0);
                    bits |= (uint64_t)tbd_decode(q, ctx, lane) << x;
                } while (M);
                if (lane == 0) F.REF[r][k] = R2 | M0;
                if (bits) emit(y, k, bits, bit);
            }
        }
        // =================== cleanup (t1.go:1350-1410): 4-row stripes, column by column ===================
        for (int y0 = 0; y0 < h; y0 += 4) {
            const int r0 = y0 + 1;
            const bool full = y0 + 4 <= h;
            uint32_t pcol = 0, pneg = 0;                               // column 64 k - 1 (rows -1..4 at bits 0..5), current state
            for (int k = 0; k < nw; k++) {
                const uint64_t colmask = k == nw - 1 ? lastmask : ~0ull;
                uint64_t Sr[6], mem[4], anym = 0;
#pragma unroll
                for (int j = 0; j < 6; j++) Sr[j] = tbd_u64(F.S[r0 - 1 + j][k]);      // (rows past the block are zero: the array has 258 rows; r0 + 4 <= 257)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    mem[i] = y0 + i < h ? ~Sr[i + 1] & ~tbd_u64(F.VIS[r0 + i][k]) & colmask : 0;
                    anym |= mem[i];
                }
                if (anym == 0) {
                    pcol = 0; pneg = 0;
#pragma unroll
                    for (int j = 0; j < 6; j++) pcol |= (uint32_t)(Sr[j] >> 63) << j;
                    if (pcol) {
#pragma unroll
                        for (int j = 0; j < 6; j++) pneg |= (uint32_t)(tbd_u64(F.NEG[r0 - 1 + j][k]) >> 63) << j;
                    }
                    continue;
                }
                uint64_t Ng[6], SrN[6], NgN[6];
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    Ng[j] = tbd_u64(F.NEG[r0 - 1 + j][k]);
                    SrN[j] = k + 1 < NWD ? tbd_u64(F.S[r0 - 1 + j][k + 1]) : 0;
                    NgN[j] = k + 1 < NWD ? tbd_u64(F.NEG[r0 - 1 + j][k + 1]) : 0;
                }
                // lanes = columns.  colv / negv: the column's six rows (current state, updated by the chain); stv: per row of the
                // stripe the static part of the ZC index (E, S, NE, SE: 5 bits) | membership (bits 20..23) | run-length eligibility as
                // far as it is static (bit 24); ssv: per row the static part of the sign index (E, S; 5 bits)
                uint32_t colv = 0, negv = 0, stv = 0, ssv = 0;
                {
                    uint32_t ecol = 0, eneg = 0;                      // column x + 1
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        colv |= ((uint32_t)(Sr[j] >> lane) & 1u) << j;
                        negv |= ((uint32_t)(Ng[j] >> lane) & 1u) << j;
                        ecol |= ((uint32_t)((Sr[j] >> 1 | SrN[j] << 63) >> lane) & 1u) << j;
                        eneg |= ((uint32_t)((Ng[j] >> 1 | NgN[j] << 63) >> lane) & 1u) << j;
                    }
                    uint32_t m4 = 0;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        // sample (x, i) = row j = i + 1 of the window: E = ecol[j], S = colv[j + 1], NE = ecol[j - 1], SE = ecol[j + 1]
                        const uint32_t e = (ecol >> (i + 1)) & 1u, s_ = (colv >> (i + 2)) & 1u;
                        const uint32_t dg = ((ecol >> i) & 1u) + ((ecol >> (i + 2)) & 1u);
                        stv |= (e + 3u * s_ + 9u * dg) << (5 * i);
                        const uint32_t en_ = (eneg >> (i + 1)) & 1u, sn = (negv >> (i + 2)) & 1u;
                        const int hc = (int)e - 2 * (int)(e & en_), vc = (int)s_ - 2 * (int)(s_ & sn);
                        ssv |= (uint32_t)(hc + 5 * vc + 12) << (5 * i);
                        m4 |= ((uint32_t)(mem[i] >> lane) & 1u) << i;
                    }
                    const bool rls = full && m4 == 15u && ecol == 0 && (colv & 0x21u) == 0;
                    stv |= m4 << 20 | (rls ? 1u << 24 : 0u);
                }
                uint64_t ns[4] = {0, 0, 0, 0}, nn[4] = {0, 0, 0, 0};
                uint64_t cols = anym;
                do {
                    const uint32_t x = (uint32_t)__builtin_ctzll(cols);
                    cols &= cols - 1;
                    const uint32_t st = __builtin_amdgcn_readlane(stv, x), ss = __builtin_amdgcn_readlane(ssv, x);
                    uint32_t cc = __builtin_amdgcn_readlane(colv, x), nc = __builtin_amdgcn_readlane(negv, x);
                    const uint32_t cw = x ? __builtin_amdgcn_readlane(colv, x - 1) : pcol;
                    const uint32_t nwc = x ? __builtin_amdgcn_readlane(negv, x - 1) : pneg;
                    const uint32_t m4 = (st >> 20) & 15u;
                    const uint32_t cc0 = cc;
                    int first = 0;
                    if ((st >> 24) & 1u && cw == 0) {                      // canUseRunLength (t1.go:1195-1208)
                        if (tbd_decode(q, CtxRL, lane) == 0) continue;
                        uint32_t pos = tbd_decode(q, CtxUni, lane) << 1;
                        pos |= tbd_decode(q, CtxUni, lane);
                        const uint32_t sv = __builtin_amdgcn_readlane(scv, 12);   // no significant neighbour: hc = vc = 0
                        const uint32_t sg = tbd_decode(q, CtxSC0 + (sv & 7u), lane) ^ (sv >> 3);
                        cc |= 1u << (pos + 1); nc |= sg << (pos + 1);
                        first = (int)pos + 1;
                    }
                    for (int i = first; i < 4; i++) {
                        if (!((m4 >> i) & 1u)) continue;
                        const uint32_t w3 = (cw >> i) & 7u;                   // NW, W, SW
                        const uint32_t nbit = (cc >> i) & 1u;                 // N (row i - 1 of the stripe = window row i)
                        const uint32_t zi = ((st >> (5 * i)) & 31u) + 9u * (w3 & 1u) + ((w3 >> 1) & 1u) + 9u * (w3 >> 2) + 3u * nbit;
                        const uint32_t zc = __builtin_amdgcn_readlane(zcv, zi);
                        if (tbd_decode(q, zc, lane)) {
                            const uint32_t wb = (w3 >> 1) & 1u, wn = (nwc >> (i + 1)) & 1u, ng = (nc >> i) & 1u;
                            const uint32_t si = ((ss >> (5 * i)) & 31u) + wb - 2u * (wb & wn) + 5u * (nbit - 2u * (nbit & ng));
                            const uint32_t sv = __builtin_amdgcn_readlane(scv, si);
                            const uint32_t sg = tbd_decode(q, CtxSC0 + (sv & 7u), lane) ^ (sv >> 3);
                            cc |= 1u << (i + 1); nc |= sg << (i + 1);
                        }
                    }
                    if (cc != cc0) {
                        colv = tbd_writelane(cc, x, colv);
                        negv = tbd_writelane(nc, x, negv);
                        const uint32_t nw4 = ((cc ^ cc0) >> 1) & 15u, ng4 = (nc >> 1) & 15u;
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            ns[i] |= (uint64_t)((nw4 >> i) & 1u) << x;
                            nn[i] |= (uint64_t)((nw4 >> i) & (ng4 >> i) & 1u) << x;
                        }
                    }
                } while (cols);
                pcol = __builtin_amdgcn_readlane(colv, 63); pneg = __builtin_amdgcn_readlane(negv, 63);
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (ns[i]) { F.S[r0 + i][k] = Sr[i + 1] | ns[i]; F.NEG[r0 + i][k] = Ng[i + 1] | nn[i]; }
                }
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (ns[i]) emit(y0 + i, k, ns[i], bit);
            }
        }
        // =================== visit flags cleared (t1.go:1372-1375) ===================
        tbd_wave_sync();
        {
            uint64_t *z = &F.VIS[0][0];
            for (int i = lane; i < RWS * NWD; i += 64) z[i] = 0;
        }
        tbd_wave_sync();
    }
    __threadfence();                                                // (the ORs above are done before the magnitudes are read back)
    // ---- signs (t1.go:1281-1289) ----
    const uint32_t mid = t1_coarse_mid(skip_planes);                // with a floor: the midpoint into every non-zero magnitude, before its sign
    for (int y = 0; y < h; y++)
        for (int k = 0; k < nw; k++) {
            const uint64_t ng = F.NEG[y + 1][k];
            const uint64_t touch = mid ? F.S[y + 1][k] : ng;        // (a negative sample is a significant one)
#ifndef J2K_TBD_TRACE
            if ((touch >> lane) & 1) { const size_t i = (size_t)y * w + 64 * k + lane; out[i] = t1_coarse_finish(out[i], mid, (ng >> lane) & 1); }
#endif
        }
}
