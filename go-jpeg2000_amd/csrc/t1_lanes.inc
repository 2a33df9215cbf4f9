// t1_lanes.inc -- the significance passes of the plane-stepped MQ block decoder, one code-block per LANE.
// Included by t1.hip inside namespace j2k (after the plane-stepped kernels: it shares their workspace records).
//
//   T1.Decode: decodeSigPropPass / decodeCleanupPass   internal/entropy/t1.go:1295-1319, 1350-1410
//   MQDecoder.Decode / byteIn / renorm                 internal/entropy/mqc.go:402-497
//
// Round 2's plane-stepped decoder put the MagRef chains of 64 blocks on the 64 lanes of a wavefront; SigProp and Cleanup stayed
// one block per wavefront with the decisions on lane 0, and those step kernels were what a C3 frame cost the device: 17 ms of
// issue-bound work per frame that frames in flight cannot share.  Here they are lanes kernels too.  Per block the state is a
// handful of 64-bit ROW MASKS (significant, negative, visited) instead of byte flags, kept per group of 64 blocks as
// [array][row][lane] so that a wavefront reads one row of all its blocks with a single 512-byte access:
//   * SigProp, row-synchronous: every lane holds rows y-1, y, y+1 of ITS block; the candidates of a row are a mask expression;
//     a trip of the inner loop takes the lowest candidate of every lane, forms its ZC (or, in the trip after a 1, its sign)
//     context from 3-bit windows of the masks through a 512-entry table, and runs ONE select-only MQ step for all lanes;
//   * Cleanup, stripe-synchronous: six rows of masks per lane (the stripe and the rows above / below), a per-lane state
//     (column, row, run-length / uniform / ZC / sign) and again one MQ step per trip.
// A wavefront costs what its slowest lane's row (stripe) costs, summed over rows; the 110 wavefronts of a 4K frame occupy a tenth
// of the SIMDs, so the chains of other frames run beside them.  What needs a wavefront per block -- the MagRef context list
// in coding order, the row words of every bit plane -- is t1_dec_plane_kernel, between the lanes kernels; the magnitudes are
// assembled from the bit planes once, by t1_dec_assemble_kernel after the last plane.
//
// Launch sequence: t1_order_kernel (which block rides on which lane), then per k (block-relative plane p = numBPS - 1 - k):
//   t1_dec_sig_lanes_kernel(k)     Cleanup(p + 1), SigProp(p)                       [k = 0: initialise]
//   t1_dec_plane_kernel(k)         row words of bit plane p + 1 (MagRef decisions, Cleanup's new samples) and of plane p (SigProp's
//                                  new samples); MagRef(p)'s context list             [k = 0: empty masks; zero a block without planes]
//   t1_dec_magref_lanes_kernel(k)  MagRef(p) chain (t1.hip: MqLaneDec is shared with the significance kernel)
// and t1_dec_assemble_kernel: magnitudes and signs into the output buffer.

enum { T1L_S = 0, T1L_NEG, T1L_VIS, T1L_REF, T1L_NEWS, T1L_NEWC, T1L_MEMB, T1L_NA };
#define T1L_GROUP_WORDS ((size_t)T1L_NA * 64 * 64)        /* u64 words of mask arrays per group of 64 blocks */
__device__ __forceinline__ uint64_t *t1l_row(uint64_t *masks, long group, int arr, int y) {
    return masks + (((size_t)group * T1L_NA + arr) * 64 + y) * 64;
}
size_t t1_dec_lanes_mask_offset(size_t njobs) { return (njobs * T1DS_STRIDE + 255) & ~size_t(255); }
size_t t1_dec_lanes_perm_offset(size_t njobs) { return t1_dec_lanes_mask_offset(njobs) + ((njobs + 63) / 64) * T1L_GROUP_WORDS * 8; }
size_t t1_dec_lanes_planes_offset(size_t njobs) { return (t1_dec_lanes_perm_offset(njobs) + (((njobs + 63) / 64) * 64 + njobs) * 4 + 255) & ~size_t(255); }
#define T1L_PLANE_WORDS ((size_t)32 * 64)               /* per block: one 64-bit row mask per bit plane and row, [plane][row] */
size_t t1_dec_lanes_bytes(size_t njobs) { return t1_dec_lanes_planes_offset(njobs) + njobs * T1L_PLANE_WORDS * 8 + 256; }
// The raw-MagRef style (j2k_plan_set_raw_magref): behind the plane words, per block the un-stuffed RAW part of its body as a linear bit string
// (decision r of the block = bit r & 31 of word r >> 5; ones from the string's end on, as RawDecoder.DecodeBit returns them) -- room for the
// 31 x 4096 decisions a plane-stepped block can have and the words a trip of t1l_raw_unstuff may run over.  The running offset of the next
// plane's decisions is the first word of the record's T1DS_BITS area, which the style does not use otherwise.
#define T1L_RAWB_WORDS ((size_t)31 * 4096 / 32 + 32)
size_t t1_dec_lanes_bytes_raw(size_t njobs) { return t1_dec_lanes_bytes(njobs) + njobs * T1L_RAWB_WORDS * 4 + 256; }
__device__ __forceinline__ uint32_t *t1l_rawbits(uint64_t *planes, int njobs, long jid) {
    return reinterpret_cast<uint32_t *>(planes + (size_t)njobs * T1L_PLANE_WORDS + 32) + (size_t)jid * T1L_RAWB_WORDS;
}

// x's bits at the set positions of m, packed to the low end (compress) and the inverse (expand), 64 bits wide: Hacker's Delight
// 7-4 / 7-5.  The six move masks depend on m only and serve any number of words.
struct T1LBitMoves {
    uint64_t mv[6];
    __device__ __forceinline__ explicit T1LBitMoves(uint64_t m) {
        uint64_t mk = ~m << 1;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            uint64_t mp = mk ^ (mk << 1);
            mp ^= mp << 2; mp ^= mp << 4; mp ^= mp << 8; mp ^= mp << 16; mp ^= mp << 32;
            mv[i] = mp & m;
            m = (m ^ mv[i]) | (mv[i] >> (1 << i));
            mk &= ~mp;
        }
    }
    __device__ __forceinline__ uint64_t compress(uint64_t x, uint64_t m) const {
        x &= m;
#pragma unroll
        for (int i = 0; i < 6; i++) { const uint64_t t = x & mv[i]; x = (x ^ t) | (t >> (1 << i)); }
        return x;
    }
    __device__ __forceinline__ uint64_t expand(uint64_t x, uint64_t m) const {
#pragma unroll
        for (int i = 5; i >= 0; i--) { const uint64_t t = x << (1 << i); x = (x & ~mv[i]) | (t & mv[i]); }
        return x & m;
    }
};

// Which block rides on which lane: blocks in descending order of a work estimate (decoder: compressed bytes, encoder: symbols),
// so that the 64 chains of a wavefront are of similar length -- a wavefront runs as long as its longest lane, and in job order
// (neighbouring blocks of a band) the longest lane of a C3 frame had 1.8 times the decisions of the average one.  One
// workgroup, counting sort over 4096 buckets; order inside a bucket is whatever the atomics give (it only places lanes).
// perm[slot] = job (0xFFFFFFFF: no job), slot_of[job] = slot.  mode 0: key = compressed bytes per bit plane of the blocks the
// plane-stepped decoder takes (others sort last; the total length orders by depth, not by how dense a plane's decisions are); mode 1: key = symbol count of the split encoder (T1F_SKIPPED sorts last).
__global__ __launch_bounds__(1024) void t1_order_kernel(const BlockJob *__restrict__ jobs, int njobs, const uint8_t *__restrict__ numbps,
                                                        const uint32_t *__restrict__ key, int mode, uint32_t *__restrict__ perm,
                                                        uint32_t *__restrict__ slot_of, int nslots) {
    __shared__ uint32_t hist[4096];
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    auto bucket = [&](int j) -> uint32_t {
        uint32_t b;
        if (mode == 0) {
            const int nb = (int)numbps[j];
            const bool take = jobs[j].w <= 64 && jobs[j].h <= 64 && nb <= T1DS_MAXP && nb > 0;
            b = take ? min((key[j] << 1) / (uint32_t)nb, 4094u) + 1u : 0u;      // bytes per bit plane, in halves
        } else {
            const uint32_t n = key[j];
            b = n == T1F_SKIPPED ? 0u : min(n >> 5, 4095u);
        }
        return 4095u - b;                                   // descending
    };
    for (int b = t; b < 4096; b += 1024) hist[b] = 0;
    __syncthreads();
    for (int j = t; j < njobs; j += 1024) atomicAdd(&hist[bucket(j)], 1u);
    __syncthreads();
    const uint32_t h0 = hist[4 * t], h1 = hist[4 * t + 1], h2 = hist[4 * t + 2], h3 = hist[4 * t + 3];
    part[t] = h0 + h1 + h2 + h3;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t v = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const uint32_t base = part[t] - (h0 + h1 + h2 + h3);
    hist[4 * t] = base; hist[4 * t + 1] = base + h0; hist[4 * t + 2] = base + h0 + h1; hist[4 * t + 3] = base + h0 + h1 + h2;
    __syncthreads();
    for (int j = t; j < njobs; j += 1024) {
        const uint32_t slot = atomicAdd(&hist[bucket(j)], 1u);
        perm[slot] = (uint32_t)j;
        if (slot_of) slot_of[j] = slot;
    }
    for (int sl = njobs + t; sl < nslots; sl += 1024) perm[sl] = 0xFFFFFFFFu;
}

// The look-up tables are the same for every wavefront of a workgroup: one copy, which every wavefront fills completely by itself
// before it reads any of it (identical values; no wavefront depends on another's stores).  Their 2 KB per wavefront were what
// kept a 9-7 transform workgroup (36 KB of LDS) from fitting beside two of these workgroups on a CU -- with twenty frames in flight the
// transform launches of C3, 17 us alone, took a millisecond each.
struct T1LTables {
    uint32_t mqtab[96];
    uint8_t zc9[3 * 512];      // ZC context by NW | N<<1 | NE<<2 | W<<3 | E<<5 | SW<<6 | S<<7 | SE<<8; per band class (LL/LH, HL, HH)
    uint8_t sc[256];           // lutSignCtx | lutSignPred << 3 by T1Tables' index
};
struct T1LShared {
    uint32_t ent[19 * 64];     // per lane: the MQ table entry of each context's current state, [context][lane]
    alignas(16) uint8_t ring[64 * T1R_STRIDE];     // MqLaneDec's per-lane ring
    uint32_t stage[2][132];                        // PERSIST: t1l_plane_work's staging
};

__device__ __forceinline__ uint32_t t1l_win3(uint64_t m, uint32_t x) {     // bits x-1, x, x+1 of m as bits 0, 1, 2
    const uint32_t sh = max(x, 1u) - 1u;
    uint32_t v = (uint32_t)(m >> sh);
    v = x == 0 ? v << 1 : v;
    return v & 7u;
}
__device__ __forceinline__ uint32_t t1l_bit(uint64_t m, uint32_t x) { return (uint32_t)(m >> x) & 1u; }
// a, b, c, d by i = 0..3, as two levels of bit tests (an equality chain on i is turned into a switch, i.e. into branches)
__device__ __forceinline__ uint64_t t1l_sel4(uint32_t i, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    const bool i0 = (i & 1u) != 0, i1 = (i & 2u) != 0;
    const uint64_t lo = i0 ? b : a, hi = i0 ? d : c;
    return i1 ? hi : lo;
}

// RawDecoder (mqc.go:516-562) over a whole RAW part at once, all 64 lanes: the first `need` decisions (and up to a trip more) as a linear bit
// string in dst.  A byte carries 8 bits, 7 behind an 0xFF -- its width depends on the byte before it only -- so a trip places 64 bytes with one
// prefix sum of the widths: every lane ORs its byte, first bit lowest, into a 20-word LDS stage that starts with the partial word the trip
// before left, the full words go to dst.  At an 0xFF followed by a byte above 0x8F, and at the end of the bytes, the reader stays at 0xFF:
// ones from there to the end of the record.  stage: 20 words of LDS owned by the calling wavefront.
__device__ __forceinline__ void t1l_raw_unstuff(int lane, const uint8_t *raw, uint32_t rawlen, uint32_t need, uint32_t *dst, uint32_t *stage) {
    const uint32_t needw = (need + 31u) / 32u + 3u;
    uint32_t P = 0, carry = 0, prev_last = 0;
    bool stuck = false;
    for (uint32_t base = 0; base < rawlen && P < need && !stuck; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        const bool in = i < rawlen;
        const uint32_t v = in ? raw[i] : 0u;
        uint32_t pv = (uint32_t)__shfl_up((int)v, 1);
        if (lane == 0) pv = prev_last;
        const uint64_t stopm = __ballot(in && pv == 0xFFu && v > 0x8Fu);
        const uint32_t nin = min(rawlen - base, 64u);
        const uint32_t nval = stopm ? (uint32_t)__ffsll((long long)stopm) - 1u : nin;
        stuck = stopm != 0;
        const bool val = (uint32_t)lane < nval;
        const uint32_t wd = val ? (pv == 0xFFu ? 7u : 8u) : 0u;
        uint32_t incl = wd;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if (lane >= o) incl += t; }
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        if (lane < 20) stage[lane] = lane == 0 ? carry : 0u;
        t1_wave_sync();
        if (val) {
            const uint32_t rev = __brev(v & ((1u << wd) - 1u)) >> (32u - wd);       // the byte's first bit lowest
            const uint32_t pos = (P & 31u) + incl - wd, w = pos >> 5, sh = pos & 31u;
            atomicOr(&stage[w], rev << sh);
            if (sh + wd > 32u) atomicOr(&stage[w + 1], rev >> (32u - sh));
        }
        t1_wave_sync();
        const uint32_t T = P + total, W0 = P >> 5, nfull = (T >> 5) - W0;              // nfull <= 16
        if ((uint32_t)lane < nfull) dst[W0 + lane] = stage[lane];
        carry = stage[nfull];
        t1_wave_sync();
        P = T;
        prev_last = (uint32_t)__shfl((int)v, 63);
    }
    const uint32_t W0 = P >> 5, first = carry | (0xFFFFFFFFu << (P & 31u));
    for (uint32_t w = W0 + (uint32_t)lane; w < needw; w += 64) dst[w] = w == W0 ? first : 0xFFFFFFFFu;
}

// The work of one block and one launch k >= 1 (see above), all 64 lanes = the block's rows.  l = the block's lane in its group;
// stage = 2 x 132 words of LDS owned by the calling wavefront.  Returns the length of MagRef(p)'s list (0 at p = -1).
// RAWMR (the raw-MagRef style): the decisions of MagRef(p + 1) are not what a chain left in the record but the next popcount(members) bits of
// the block's un-stuffed raw string `rawwords`, from the running offset on; the context list of MagRef(p) is still written (nobody reads it).
template <bool RAWMR = false>
__device__ __forceinline__ uint32_t t1l_plane_work(int lane, int w, int h, int p, int k, uint8_t *rec, uint64_t *masks, long group, int l,
                                                   uint64_t *pl, uint32_t (*stage)[132], const uint32_t *rawwords = nullptr) {
    auto row_ptr = [&](int arr) -> uint64_t * { return t1l_row(masks, group, arr, lane) + l; };     // lane = row
    const bool inrow = lane < h;
    const uint64_t S = inrow ? *row_ptr(T1L_S) : 0ull, VIS = inrow ? *row_ptr(T1L_VIS) : 0ull, REF = inrow ? *row_ptr(T1L_REF) : 0ull;
    const uint64_t NEWS = (inrow && p >= 0) ? *row_ptr(T1L_NEWS) : 0ull, NEWC = inrow ? *row_ptr(T1L_NEWC) : 0ull;
    const uint64_t MEMBP = inrow ? *row_ptr(T1L_MEMB) : 0ull;
    const uint64_t PLS = (inrow && k > 1) ? pl[64 * (p + 1)] : 0ull;          // SigProp(p + 1)'s new samples, stored by the launch before
    auto excl_sum = [&](uint32_t v, uint32_t &total) -> uint32_t {
        uint32_t incl = v;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        total = __shfl(incl, 63);
        return incl - v;
    };
    // ---- bit plane p + 1 of this row: MagRef decisions (t1.go:1331-1347) at the members' columns | Cleanup's | SigProp's new samples ----
    uint64_t PL1;
    {
        const uint32_t cnt = (uint32_t)__popcll(MEMBP);
        uint32_t total;
        uint32_t off = excl_sum(cnt, total);
        const uint32_t *bits = RAWMR ? rawwords : reinterpret_cast<const uint32_t *>(rec + T1DS_BITS);
        if (RAWMR) {
            uint32_t *const roffp = reinterpret_cast<uint32_t *>(rec + T1DS_BITS);
            const uint32_t roff = *roffp;
            off += roff;
            t1_wave_sync();
            if (lane == 0) *roffp = roff + total;
        }
        uint64_t d = 0;
        if (cnt) {
            const uint32_t w0 = off >> 5, sh = off & 31;
            const uint64_t lo = (uint64_t)bits[w0 + 1] << 32 | bits[w0];
            d = lo >> sh;
            if (sh) d |= (uint64_t)bits[w0 + 2] << (64 - sh);
            if (cnt < 64) d &= (1ull << cnt) - 1;
        }
        const T1LBitMoves mvp(MEMBP);
        PL1 = PLS | NEWC | mvp.expand(d, MEMBP);
    }
    if (p < 0) {                                               // plane 0 complete: t1_dec_assemble_kernel does the rest
        if (inrow) pl[0] = PL1;
        return 0;
    }
    if (inrow) { pl[64 * (p + 1)] = PL1; pl[64 * p] = NEWS; }
    // ---- MagRef(p): members in coding order and their contexts ----
    const uint64_t memb = S & ~VIS;
    uint64_t su = (uint64_t)__shfl_up((int)(S >> 32), 1) << 32 | (uint32_t)__shfl_up((int)S, 1);
    uint64_t sd = (uint64_t)__shfl_down((int)(S >> 32), 1) << 32 | (uint32_t)__shfl_down((int)S, 1);
    if (lane == 0) su = 0;
    if (lane == 63) sd = 0;
    const uint64_t hasnb = spread3(su) | spread3(sd) | (S << 1) | (S >> 1);
    for (int i = lane; i < 2 * 132; i += 64) (&stage[0][0])[i] = 0;
    const uint32_t cnt2 = (uint32_t)__popcll(memb);
    uint32_t nmr;
    const uint32_t off2 = excl_sum(cnt2, nmr);
    t1_wave_sync();
    if (cnt2) {
        const T1LBitMoves mvm(memb);
        const uint64_t c2 = mvm.compress(REF, memb), c1 = mvm.compress(hasnb & ~REF, memb);     // Mag2: refined before; Mag1: a significant neighbour
        const uint32_t w0 = off2 >> 5, sh = off2 & 31;
        auto deposit = [&](uint32_t *dst, uint64_t v) {
            if (!v) return;
            const uint64_t lo = v << sh;
            atomicOr(&dst[w0], (uint32_t)lo);
            if ((uint32_t)(lo >> 32)) atomicOr(&dst[w0 + 1], (uint32_t)(lo >> 32));
            if (sh) { const uint32_t top = (uint32_t)(v >> (64 - sh)); if (top) atomicOr(&dst[w0 + 2], top); }
        };
        deposit(stage[0], c2);
        deposit(stage[1], c1);
    }
    t1_wave_sync();
    {
        uint32_t *lst = reinterpret_cast<uint32_t *>(rec + T1DS_LIST);
        const uint32_t nw = (nmr + 31) >> 5;                                  // words in use (the lanes kernel reads whole 16-bit pieces below nmr)
        for (uint32_t i = lane; i < nw; i += 64) { lst[i] = stage[0][i]; lst[128 + i] = stage[1][i]; }
    }
    t1_wave_sync();                                                           // (the next caller clears the stage)
    if (inrow) { *row_ptr(T1L_REF) = REF | memb; *row_ptr(T1L_MEMB) = memb; }
    return nmr;
}

// Out of line for the PERSIST kernel: its phases never overlap, but inlined into one function their registers add up (209 against the
// significance passes' 145), and two such wavefronts per SIMD then leave too few for a transform workgroup of another frame to
// become resident beside them.  (The MagRef chain stays inline: out of line its decoder state lives in scratch memory, 86 ms per frame
// instead of 45.)
__device__ __attribute__((noinline)) uint32_t t1l_plane_work_call(int lane, int w, int h, int p, int k, uint8_t *rec, uint64_t *masks, long group, int l,
                                                                  uint64_t *pl, uint32_t (*stage)[132]) {
    return t1l_plane_work(lane, w, h, p, k, rec, masks, group, l, pl, stage);
}
__device__ __attribute__((noinline)) uint32_t t1l_plane_work_raw_call(int lane, int w, int h, int p, int k, uint8_t *rec, uint64_t *masks, long group, int l,
                                                                      uint64_t *pl, uint32_t (*stage)[132], const uint32_t *rawwords) {
    return t1l_plane_work<true>(lane, w, h, p, k, rec, masks, group, l, pl, stage, rawwords);
}

// PERSIST = false: launch k of the sequence above (Cleanup(p + 1), SigProp(p)).  PERSIST = true: the WHOLE plane-stepped decode of
// the wavefront's 64 blocks in one launch -- initialisation, then for k = 1 .. 31 the significance passes, the plane work of each of
// the 64 blocks (t1l_plane_work, the wavefront turned sideways: lanes = rows of one block at a time) and the MagRef chains, with the MQ
// decoder, its ring and the context entries staying where they are.  Nothing crosses wavefronts: no launch boundary makes a
// wavefront wait for the slowest one of another group, 3 launches per frame instead of 96, and the plane work runs at the lanes
// kernels' priority instead of queueing behind other frames' kernels.
// RAWMR (the raw-MagRef style): the MQ decoder runs on the MQ part of the body H | MQ | RAW; PERSIST un-stuffs every block's RAW part before the
// first plane and has no MagRef chains.
template <bool PERSIST, bool RAWMR = false>
__global__ __launch_bounds__(64 * T1_LANES_WPW) void t1_dec_sig_lanes_kernel(const BlockJob *__restrict__ jobs, int njobs, const uint8_t *__restrict__ stream,
                                                              const uint64_t *__restrict__ offs, const uint32_t *__restrict__ lens,
                                                              const uint8_t *__restrict__ numbps, uint8_t *__restrict__ ws,
                                                              uint64_t *__restrict__ masks, const uint32_t *__restrict__ perm,
                                                              uint64_t *__restrict__ planes, int k_launch, int skip_uniform, const uint8_t *__restrict__ floors) {
    __shared__ T1LShared L_w[T1_LANES_WPW];
    __shared__ T1LTables TB;
    T1_LANES_PRIO();
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    T1LShared &L = L_w[wv];
    const long group = (long)blockIdx.x * T1_LANES_WPW + wv;
    if (group * 64 >= (long)((njobs + 63) / 64) * 64) return;
    const uint32_t pj = perm[group * 64 + lane];
    const long jid = (long)pj;
    bool live0 = pj != 0xFFFFFFFFu;
    const int skip_planes = t1_floor_of(skip_uniform, floors, live0 ? jid : 0);       // this block's floor: the call's, or its own if that is higher
    const BlockJob J = jobs[live0 ? jid : 0];
    const int nb0 = live0 ? (int)numbps[jid] : 0;
    const int nb = max(nb0 - skip_planes, 0);     // the planes above the quality floor: below, plane p stands for bit plane p + skip_planes
    live0 = live0 && J.w <= 64 && J.h <= 64 && nb0 <= T1DS_MAXP && nb > 0;
    const int w = J.w, h = J.h;
    uint8_t *const rec = ws + (size_t)(live0 ? jid : 0) * T1DS_STRIDE;
    T1DecState *const stp = reinterpret_cast<T1DecState *>(rec + T1DS_STATE);
    uint32_t *const gent = reinterpret_cast<uint32_t *>(rec + offsetof(T1Dec64Shared, ent));

    if (!PERSIST && k_launch == 0) {
        // every block of the group starts with empty masks; SigProp and MagRef of the first plane have nothing to do (t1.go:1291-1293)
        for (int y = 0; y < 64; y++) {
            t1l_row(masks, group, T1L_S, y)[lane] = 0; t1l_row(masks, group, T1L_NEG, y)[lane] = 0; t1l_row(masks, group, T1L_VIS, y)[lane] = 0;
        }
        if (live0) {
            MqDec d;
            if (RAWMR) {
                uint32_t m, rawlen;
                t1_raw_split(stream + offs[jid], lens[jid], m, rawlen);
                mq_dec_init(d, stream + offs[jid] + T1_RAW_HDR, (long)m);
            } else
            mq_dec_init(d, stream + offs[jid], (long)lens[jid]);
            T1DecState t; t.C = d.C; t.A = d.A; t.CT = d.CT; t.nmr = 0; t.bp = d.bp; t.len = d.len;
            *stp = t;
            for (int c = 0; c < 20; c++) gent[c] = c < NumContexts ? c_mq94.v[c == CtxUni ? 92 : 0] : 0u;
        }
        return;
    }
    bool live = live0 && (PERSIST || nb - 1 - k_launch >= -1);
    if (!__any(live)) return;
    // ---- tables ----
    for (int q = lane; q < 94; q += 64) TB.mqtab[q] = c_mq94.v[q];
    for (int q = lane; q < 3 * 512; q += 64) {
        const int cls = q >> 9, ix = q & 511;
        const int nw = ix & 1, n = (ix >> 1) & 1, ne = (ix >> 2) & 1, wv = (ix >> 3) & 1, e = (ix >> 5) & 1, sw = (ix >> 6) & 1, s = (ix >> 7) & 1, se = (ix >> 8) & 1;
        int hh = wv + e, v = n + s, ctx;
        const int d = nw + ne + sw + se;
        if (cls == 1) { const int t = hh; hh = v; v = t; }            // HL: swap h and v (t1_luts.go:34-110)
        if (cls == 2) {
            const int hv = hh + v;
            if (hv >= 3) ctx = 8;
            else if (hv == 2) ctx = d >= 2 ? 7 : (d >= 1 ? 6 : 5);
            else if (hv == 1) ctx = d >= 2 ? 4 : 3;
            else ctx = d >= 2 ? 2 : (d >= 1 ? 1 : 0);
        } else {
            if (hh == 2) ctx = 8;
            else if (hh == 1) ctx = v >= 1 ? 7 : (d >= 1 ? 6 : 5);
            else if (v == 2) ctx = 4;
            else if (v == 1) ctx = d >= 1 ? 3 : 2;
            else ctx = d >= 2 ? 1 : 0;
        }
        TB.zc9[q] = (uint8_t)ctx;
    }
    for (int q = lane; q < 256; q += 64) {                             // t1_luts.go:153-230, as build_tables
        int hc = 0, vc = 0, pred = 0, sctx = 0;
        if (q & 1) hc += (q & 2) ? -1 : 1;
        if (q & 4) hc += (q & 8) ? -1 : 1;
        if (q & 16) vc += (q & 32) ? -1 : 1;
        if (q & 64) vc += (q & 128) ? -1 : 1;
        if (hc < 0) { pred = 1; hc = -hc; }
        if (hc == 0 && vc < 0) { pred = 1; vc = -vc; }
        if (hc == 1) sctx = vc == 1 ? 4 : (vc == 0 ? 2 : 1);
        else if (hc == 0) sctx = vc == 1 ? 1 : 0;
        else if (hc == 2) sctx = 3;
        TB.sc[q] = (uint8_t)(sctx | pred << 3);
    }
    T1DecState st;
    if (PERSIST) {
        for (int y = 0; y < 64; y++) {
            t1l_row(masks, group, T1L_S, y)[lane] = 0; t1l_row(masks, group, T1L_NEG, y)[lane] = 0; t1l_row(masks, group, T1L_VIS, y)[lane] = 0;
            t1l_row(masks, group, T1L_REF, y)[lane] = 0; t1l_row(masks, group, T1L_MEMB, y)[lane] = 0;
        }
        for (int c = 0; c < 19; c++) L.ent[c * 64 + lane] = c_mq94.v[c == CtxUni ? 92 : 0];
        st = T1DecState{0, 0x8000u, 0, 0, 0, 0};
        if (live) {
            MqDec d;
            if (RAWMR) {
                uint32_t m, rawlen;
                t1_raw_split(stream + offs[jid], lens[jid], m, rawlen);
                mq_dec_init(d, stream + offs[jid] + T1_RAW_HDR, (long)m);
            } else
            mq_dec_init(d, stream + offs[jid], (long)lens[jid]);
            st.C = d.C; st.A = d.A; st.CT = d.CT; st.bp = d.bp; st.len = d.len;
        }
    } else {
        for (int c = 0; c < 19; c++) L.ent[c * 64 + lane] = live ? gent[c] : c_mq94.v[0];
        st = *stp;
    }
    const uint32_t zcbase = (J.band == 1 ? 1u : (J.band == 3 ? 2u : 0u)) * 512u;

    // ---- this lane's MQ decoder ----
    MqLaneDec mq;
    mq.start(stream + offs[live ? jid : 0] + (RAWMR ? T1_RAW_HDR : 0u), st, live, L.ring, lane);
    t1_wave_sync();
    if (PERSIST && RAWMR) {                                     // every block's RAW part, un-stuffed once (lanes = bytes of one block at a time)
        uint64_t todo = __ballot(live);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t jl = (uint32_t)__builtin_amdgcn_readlane((int)pj, l);
            const uint32_t need = (uint32_t)(__builtin_amdgcn_readlane(nb0, l) * __builtin_amdgcn_readlane(w, l) * __builtin_amdgcn_readlane(h, l));
            const uint8_t *body = stream + offs[jl];
            uint32_t m, rawlen;
            t1_raw_split(body, lens[jl], m, rawlen);
            t1l_raw_unstuff(lane, body + T1_RAW_HDR + m, rawlen, need, t1l_rawbits(planes, njobs, (long)jl), &L.stage[0][0]);
            if (lane == 0) *reinterpret_cast<uint32_t *>(ws + (size_t)jl * T1DS_STRIDE + T1DS_BITS) = 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        t1_wave_sync();
    }
    uint32_t nact = 0;
    // one decision of every lane that has one (`act`) in context ctx; b0 / b1 from mq.peek() at the top of the trip
    auto mq_step = [&](uint32_t ctx, bool act, uint32_t b0, uint32_t b1) -> uint32_t {
#ifdef J2K_T1L_DEBUG
        nact += act ? 1u : 0u;
#endif
        uint32_t *const ep = &L.ent[ctx * 64 + lane];
        uint32_t e_new;
        const uint32_t dec = mq.step(*ep, TB.mqtab, act, b0, b1, e_new);
        *ep = e_new;
        return dec;
    };

    const uint64_t WM = w >= 64 ? ~0ull : ((1ull << w) - 1);
    auto wave_max = [&](int v) -> int {
        for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
        return v;
    };
    auto mrow = [&](int arr, int y) -> uint64_t * { return t1l_row(masks, group, arr, y) + lane; };

    uint32_t nmr_mine = 0;                                       // PERSIST: the length of this lane's MagRef list
#ifdef J2K_T1L_DEBUG
    uint32_t trips_cl = 0, nact_cl = 0;
#endif
    for (int k = PERSIST ? 1 : k_launch; k <= (PERSIST ? T1DS_MAXP : k_launch); k++) {
    const int p = nb - 1 - k;
    const bool docl = live && p >= -1;            // Cleanup(p + 1): p + 1 <= numBPS - 1 because k >= 1
    const bool dosig = live && p >= 0;            // SigProp(p)
    if (!__any(docl)) break;
    // ================= Cleanup(p + 1), stripe by stripe (t1.go:1350-1410) =================
    {
        const int hmax = wave_max(docl ? h : 0);
        // rows R0..R5 = y0 - 1 .. y0 + 4 of the significance mask, N0..N5 of the sign mask; V = visited (rows y0 .. y0 + 3)
        uint64_t R0 = 0, N0 = 0, R1, R2, R3, R4, R5, N1, N2, N3, N4, N5, V0, V1, V2, V3;
        auto ldrow = [&](int arr, int y) -> uint64_t { return y < 64 ? *mrow(arr, y) : 0ull; };
        uint64_t nR1 = ldrow(T1L_S, 0), nR2 = ldrow(T1L_S, 1), nR3 = ldrow(T1L_S, 2), nR4 = ldrow(T1L_S, 3), nR5 = ldrow(T1L_S, 4);
        uint64_t nN1 = ldrow(T1L_NEG, 0), nN2 = ldrow(T1L_NEG, 1), nN3 = ldrow(T1L_NEG, 2), nN4 = ldrow(T1L_NEG, 3), nN5 = ldrow(T1L_NEG, 4);
        uint64_t nV0 = ldrow(T1L_VIS, 0), nV1 = ldrow(T1L_VIS, 1), nV2 = ldrow(T1L_VIS, 2), nV3 = ldrow(T1L_VIS, 3);
        for (int y0 = 0; y0 < hmax; y0 += 4) {
            R1 = nR1; R2 = nR2; R3 = nR3; R4 = nR4; R5 = nR5; N1 = nN1; N2 = nN2; N3 = nN3; N4 = nN4; N5 = nN5;
            V0 = nV0; V1 = nV1; V2 = nV2; V3 = nV3;
            if (y0 + 4 < hmax) {                     // the next stripe's rows: nothing of them is written by this stripe
                nR1 = ldrow(T1L_S, y0 + 4); nR2 = ldrow(T1L_S, y0 + 5); nR3 = ldrow(T1L_S, y0 + 6); nR4 = ldrow(T1L_S, y0 + 7); nR5 = ldrow(T1L_S, y0 + 8);
                nN1 = ldrow(T1L_NEG, y0 + 4); nN2 = ldrow(T1L_NEG, y0 + 5); nN3 = ldrow(T1L_NEG, y0 + 6); nN4 = ldrow(T1L_NEG, y0 + 7); nN5 = ldrow(T1L_NEG, y0 + 8);
                nV0 = ldrow(T1L_VIS, y0 + 4); nV1 = ldrow(T1L_VIS, y0 + 5); nV2 = ldrow(T1L_VIS, y0 + 6); nV3 = ldrow(T1L_VIS, y0 + 7);
            }
            // members: neither significant nor visited by SigProp (t1.go:1385-1390)
            const uint64_t M0 = (docl && y0 + 0 < h) ? ~R1 & ~V0 & WM : 0ull;
            const uint64_t M1 = (docl && y0 + 1 < h) ? ~R2 & ~V1 & WM : 0ull;
            const uint64_t M2 = (docl && y0 + 2 < h) ? ~R3 & ~V2 & WM : 0ull;
            const uint64_t M3 = (docl && y0 + 3 < h) ? ~R4 & ~V3 & WM : 0ull;
            const bool full = y0 + 4 <= h;
            uint64_t cols = M0 | M1 | M2 | M3;
            uint32_t cst = 0, x = 0, i = 0, mem = 0, posacc = 0;     // cst, one bit: 0 idle, 1 run-length, 2 / 4 uniform, 8 ZC, 16 sign
            uint64_t orall = R0 | R1 | R2 | R3 | R4 | R5;
            // One trip = one decision of every lane that still has one in this stripe.  Everything is computed by every lane
            // and kept by selects: a divergent `if` costs exec-mask bookkeeping and register copies at the loop header that
            // tripled the trip (648 instructions against 250).
            while (__any(cst != 0 || cols != 0)) {
                mq.tick();
                uint32_t b0, b1;
                mq.peek(b0, b1);
                // ---- idle lanes take their next column ----
                const bool newcol = cst == 0 && cols != 0;
                const uint32_t xn = (uint32_t)__ffsll((long long)cols) - 1u;
                x = newcol ? xn : x;
                cols = newcol ? cols & (cols - 1) : cols;
                const uint32_t memx = t1l_bit(M0, x) | t1l_bit(M1, x) << 1 | t1l_bit(M2, x) << 2 | t1l_bit(M3, x) << 3;
                const bool can_rl = full && memx == 15u && t1l_win3(orall, x) == 0;
                const uint32_t ifirst = (uint32_t)__ffs((int)memx) - 1u;
                cst = newcol ? (can_rl ? 1u : 8u) : cst;
                i = (newcol && !can_rl) ? ifirst : i;
                mem = newcol ? (can_rl ? memx : memx & (memx - 1)) : mem;
                const bool act = cst != 0;
                // ---- contexts of sample (i, x) ----
                const uint64_t ru = t1l_sel4(i, R0, R1, R2, R3), rc = t1l_sel4(i, R1, R2, R3, R4), rd = t1l_sel4(i, R2, R3, R4, R5);
                const uint64_t nu = t1l_sel4(i, N0, N1, N2, N3), nc = t1l_sel4(i, N1, N2, N3, N4), nd = t1l_sel4(i, N2, N3, N4, N5);
                const uint32_t wu = t1l_win3(ru, x), wc = t1l_win3(rc, x), wd = t1l_win3(rd, x);
                const uint32_t zctx = TB.zc9[zcbase + (wu | wc << 3 | wd << 6)];
                const uint32_t nc3 = t1l_win3(nc, x);
                const uint32_t sidx = (wc & 1u) | (nc3 & 1u) << 1 | ((wc >> 2) & 1u) << 2 | ((nc3 >> 2) & 1u) << 3 | ((wu >> 1) & 1u) << 4 |
                                      t1l_bit(nu, x) << 5 | ((wd >> 1) & 1u) << 6 | t1l_bit(nd, x) << 7;
                const uint32_t scv = TB.sc[sidx];
                const bool s1 = (cst & 1u) != 0, s2 = (cst & 2u) != 0, s3 = (cst & 4u) != 0, s4 = (cst & 8u) != 0, s5 = (cst & 16u) != 0;
                const uint32_t ctx = s1 ? (uint32_t)CtxRL : ((s2 || s3) ? (uint32_t)CtxUni : (s5 ? CtxSC0 + (scv & 7u) : zctx));
                const uint32_t dec = mq_step(ctx, act, b0, b1);
                // ---- what the decision does ----
                const uint64_t bx = s5 ? 1ull << x : 0ull;                 // the sample turns significant after its sign (t1.go:1322-1328)
                const uint64_t ng = (dec ^ (scv >> 3)) ? bx : 0ull;
                const uint32_t ib = 1u << i;
                const bool r0 = (ib & 1u) != 0, r1 = (ib & 2u) != 0, r2 = (ib & 4u) != 0, r3 = (ib & 8u) != 0;
                R1 |= r0 ? bx : 0ull; R2 |= r1 ? bx : 0ull; R3 |= r2 ? bx : 0ull; R4 |= r3 ? bx : 0ull;
                N1 |= r0 ? ng : 0ull; N2 |= r1 ? ng : 0ull; N3 |= r2 ? ng : 0ull; N4 |= r3 ? ng : 0ull;
                orall |= bx;
                posacc = s2 ? dec << 1 : posacc;
                const uint32_t irl = posacc | dec;                          // s3: the run's first significant row
                const bool advance = (s4 && !dec) || s5;                    // on to the column's next member row
                const uint32_t inext = (uint32_t)__ffs((int)mem) - 1u;
                const uint32_t st_adv = mem ? 8u : 0u;
                cst = s1 ? (dec ? 2u : 0u) : (s2 ? 4u : (s3 ? 16u : (advance ? st_adv : (s4 ? 16u : cst))));
                i = s3 ? irl : (advance && mem ? inext : i);
                mem = s3 ? (0xFu << (irl + 1)) & 0xFu : (advance ? mem & (mem - 1) : mem);
            }
            if (docl) {
                if (y0 + 0 < h) { *mrow(T1L_S, y0 + 0) = R1; *mrow(T1L_NEG, y0 + 0) = N1; *mrow(T1L_NEWC, y0 + 0) = R1 & M0; }
                if (y0 + 1 < h) { *mrow(T1L_S, y0 + 1) = R2; *mrow(T1L_NEG, y0 + 1) = N2; *mrow(T1L_NEWC, y0 + 1) = R2 & M1; }
                if (y0 + 2 < h) { *mrow(T1L_S, y0 + 2) = R3; *mrow(T1L_NEG, y0 + 2) = N3; *mrow(T1L_NEWC, y0 + 2) = R3 & M2; }
                if (y0 + 3 < h) { *mrow(T1L_S, y0 + 3) = R4; *mrow(T1L_NEG, y0 + 3) = N4; *mrow(T1L_NEWC, y0 + 3) = R4 & M3; }
            }
            R0 = R4; N0 = N4;
        }
    }
#ifdef J2K_T1L_DEBUG
    trips_cl = mq.nstep; nact_cl = nact;
#endif
    // the rows SigProp reads next were written by this wavefront's own lanes, each its own column of the arrays
    // ================= SigProp(p), row by row (t1.go:1295-1319) =================
    if (__any(dosig)) {
        const int hmax = wave_max(dosig ? h : 0);
        auto ldrow = [&](int arr, int y) -> uint64_t { return y < 64 ? *mrow(arr, y) : 0ull; };
        uint64_t Su = 0, Nu = 0, Sc = ldrow(T1L_S, 0), Nc = ldrow(T1L_NEG, 0), Sd = ldrow(T1L_S, 1), Nd = ldrow(T1L_NEG, 1);
        for (int y = 0; y < hmax; y++) {
            const uint64_t Sn = ldrow(T1L_S, y + 2), Nn = ldrow(T1L_NEG, y + 2);
            const bool rowlive = dosig && y < h;
            // candidates: not significant, a significant neighbour (the row above as this pass left it)
            uint64_t m = rowlive ? (~Sc & WM & (spread3(Su) | spread3(Sd) | (Sc << 1) | (Sc >> 1))) : 0ull;
            uint64_t newsig = 0, newneg = 0, vis = 0;
            uint32_t phase = 0, xi = 0;
            while (__any(m != 0 || phase != 0)) {
                mq.tick();
                uint32_t b0, b1;
                mq.peek(b0, b1);
                const bool pick = phase == 0 && m != 0;
                const uint32_t xnext = (uint32_t)__ffsll((long long)m) - 1u;
                xi = pick ? xnext : xi;
                m = pick ? m & (m - 1) : m;
                const bool act = pick || phase != 0;
                const uint64_t bx = 1ull << xi;
                const uint64_t cur = Sc | newsig, ncur = Nc | newneg;
                const uint32_t wu = t1l_win3(Su, xi), wc = t1l_win3(cur, xi), wd = t1l_win3(Sd, xi);
                const uint32_t zctx = TB.zc9[zcbase + (wu | wc << 3 | wd << 6)];
                const uint32_t nc3 = t1l_win3(ncur, xi);
                const uint32_t sidx = (wc & 1u) | (nc3 & 1u) << 1 | ((wc >> 2) & 1u) << 2 | ((nc3 >> 2) & 1u) << 3 | ((wu >> 1) & 1u) << 4 |
                                      t1l_bit(Nu, xi) << 5 | ((wd >> 1) & 1u) << 6 | t1l_bit(Nd, xi) << 7;
                const uint32_t scv = TB.sc[sidx];
                const bool sg = phase != 0;
                const uint32_t ctx = sg ? CtxSC0 + (scv & 7u) : zctx;
                const uint32_t dec = mq_step(ctx, act, b0, b1);
                const uint64_t bs = sg ? bx : 0ull;
                newsig |= bs;
                newneg |= (dec ^ (scv >> 3)) ? bs : 0ull;
                m |= (bs << 1) & WM & ~Sc;              // the right-hand neighbour becomes a candidate (t1.go:1303)
                vis |= pick ? bx : 0ull;
                phase = pick ? dec : 0u;
            }
            if (rowlive) {
                Sc |= newsig; Nc |= newneg;
                *mrow(T1L_S, y) = Sc; *mrow(T1L_NEG, y) = Nc; *mrow(T1L_VIS, y) = vis; *mrow(T1L_NEWS, y) = newsig;
            }
            Su = Sc; Nu = Nc; Sc = Sd; Nc = Nd; Sd = Sn; Nd = Nn;
        }
    }
    if (PERSIST) {
        // ---- the plane work of every block of the group that is still being decoded (lanes = rows of one block at a time) ----
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");     // the masks the lanes wrote above are read across lanes below
        t1_wave_sync();
        uint64_t todo = __ballot(docl);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int wl = __builtin_amdgcn_readlane(w, l), hl = __builtin_amdgcn_readlane(h, l), pl_ = __builtin_amdgcn_readlane(p, l);
            const uint32_t jl = (uint32_t)__builtin_amdgcn_readlane((int)pj, l);
            const uint32_t n_l = RAWMR ? t1l_plane_work_raw_call(lane, wl, hl, pl_, k, ws + (size_t)jl * T1DS_STRIDE, masks, group, l,
                                                                 planes + (size_t)jl * T1L_PLANE_WORDS + lane, L.stage, t1l_rawbits(planes, njobs, (long)jl))
                                       : t1l_plane_work_call(lane, wl, hl, pl_, k, ws + (size_t)jl * T1DS_STRIDE, masks, group, l,
                                                planes + (size_t)jl * T1L_PLANE_WORDS + lane, L.stage);
            if (lane == l) nmr_mine = n_l;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");     // lists and masks written by rows are read by the blocks' own lanes
        t1_wave_sync();
        // ---- MagRef(p) ----
        const uint32_t n = (dosig && !RAWMR) ? nmr_mine : 0u;          // (the style: MagRef(p) is read from the raw string by the next plane work)
        uint32_t nmax = n;
        for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, o));
        if (nmax) {
            uint32_t e0 = L.ent[CtxMag0 * 64 + lane], e1 = L.ent[CtxMag1 * 64 + lane], e2 = L.ent[CtxMag2 * 64 + lane];
            t1_magref_chain<true>(mq, TB.mqtab, e0, e1, e2, rec, n, nmax, dosig);
            L.ent[CtxMag0 * 64 + lane] = e0; L.ent[CtxMag1 * 64 + lane] = e1; L.ent[CtxMag2 * 64 + lane] = e2;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");     // the decision bits are read by the next plane work
    }
    }   // k
#ifdef J2K_T1L_DEBUG
    {
        const int k = k_launch;
        uint32_t sum = nact, mx = nact;
        for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o); mx = max(mx, (uint32_t)__shfl_xor((int)mx, o)); }
        uint32_t mxc = nact_cl;
        for (int o = 32; o > 0; o >>= 1) mxc = max(mxc, (uint32_t)__shfl_xor((int)mxc, o));
        if (lane == 0 && (blockIdx.x % 16) == 0 && k <= 6) printf("T1L k=%d wave=%d trips=%u (cleanup %u) sum=%u max=%u (cleanup max %u)\n", k, (int)blockIdx.x, mq.nstep, trips_cl, sum, mx, mxc);
    }
#endif
    if (!PERSIST && live) {
        for (int c = 0; c < 19; c++) gent[c] = L.ent[c * 64 + lane];
        mq.save(st);
        *stp = st;
    }
}

// One block per wavefront, between the lanes kernels: everything of a plane that is parallel over the block's samples, with
// lane = ROW throughout and no loop over rows:
//   * the MagRef decisions of plane p + 1 are a contiguous range of the decision bits per row (exclusive prefix sum of the rows'
//     member counts); expanded to the members' columns, OR-ed with Cleanup's new samples and SigProp's (stored one launch
//     earlier) they are the row's word of bit plane p + 1 -- kept per block as [plane][row], 512 bytes per plane;
//   * MagRef(p)'s context list is two bit strings (Mag2, Mag1) in coding order: per row the two masks compressed by the member mask,
//     OR-ed into place in LDS at the row's offset;
//   * the magnitudes are assembled ONCE from the planes and signed, by t1_dec_assemble_kernel after the last plane's launch.
// Round 3's first version touched the output buffer in every plane (32 KB read and written per block and plane) and walked the
// 64 rows twice per launch: 46 000 instructions per block against 16 000 now.
__global__ __launch_bounds__(64) void t1_dec_plane_kernel(const BlockJob *__restrict__ jobs, int njobs, const uint8_t *__restrict__ numbps,
                                                          int32_t *__restrict__ decoded, uint8_t *__restrict__ ws, uint64_t *__restrict__ masks,
                                                          const uint32_t *__restrict__ slot_of, uint64_t *__restrict__ planes, int k, int skip_uniform, const uint8_t *__restrict__ floors) {
    __shared__ uint32_t stage[2][132];
    const int jid = blockIdx.x;
    if (jid >= njobs) return;
    const int skip_planes = t1_floor_of(skip_uniform, floors, jid);       // this block's floor: the call's, or its own if that is higher
    const int nb0 = (int)numbps[jid];
    const int nb = max(nb0 - skip_planes, 0);                  // as in t1_dec_sig_lanes_kernel: plane p = bit plane p + skip_planes
    const int p = nb - 1 - k;
    if (nb0 > T1DS_MAXP || p < -1) return;
    const BlockJob J = jobs[jid];
    const int w = J.w, h = J.h;
    if (w > 64 || h > 64) return;
    const int lane = threadIdx.x;
    const uint32_t slot = slot_of[jid];
    const long group = slot >> 6;
    const int l = slot & 63;
    uint8_t *const rec = ws + (size_t)jid * T1DS_STRIDE;
    T1DecState *const stp = reinterpret_cast<T1DecState *>(rec + T1DS_STATE);
    uint64_t *const pl = planes + (size_t)jid * T1L_PLANE_WORDS + lane;                             // + 64 * plane
    if (k == 0) {                                              // (a block without planes is zeroed by t1_dec_assemble_kernel)
        t1l_row(masks, group, T1L_REF, lane)[l] = 0; t1l_row(masks, group, T1L_MEMB, lane)[l] = 0;
        if (lane == 0) stp->nmr = 0;
        return;
    }
    const uint32_t nmr = t1l_plane_work(lane, w, h, p, k, rec, masks, group, l, pl, stage);
    if (lane == 0 && p >= 0) stp->nmr = nmr;
}

// t1_dec_plane_kernel in the raw-MagRef style: k = 0 also un-stuffs the block's RAW part (t1l_raw_unstuff) and clears the running offset; the
// later launches read MagRef's decisions from that string, and no t1_dec_magref_lanes_kernel runs between them.
__global__ __launch_bounds__(64) void t1_dec_plane_raw_kernel(const BlockJob *__restrict__ jobs, int njobs, const uint8_t *__restrict__ stream,
                                                              const uint64_t *__restrict__ offs, const uint32_t *__restrict__ lens, const uint8_t *__restrict__ numbps,
                                                              uint8_t *__restrict__ ws, uint64_t *__restrict__ masks, const uint32_t *__restrict__ slot_of,
                                                              uint64_t *__restrict__ planes, int k, int skip_uniform, const uint8_t *__restrict__ floors) {
    __shared__ uint32_t stage[2][132];
    const int jid = blockIdx.x;
    if (jid >= njobs) return;
    const int skip_planes = t1_floor_of(skip_uniform, floors, jid);
    const int nb0 = (int)numbps[jid];
    const int nb = max(nb0 - skip_planes, 0);
    const int p = nb - 1 - k;
    if (nb0 > T1DS_MAXP || p < -1) return;
    const BlockJob J = jobs[jid];
    const int w = J.w, h = J.h;
    if (w > 64 || h > 64) return;
    const int lane = threadIdx.x;
    const uint32_t slot = slot_of[jid];
    const long group = slot >> 6;
    const int l = slot & 63;
    uint8_t *const rec = ws + (size_t)jid * T1DS_STRIDE;
    T1DecState *const stp = reinterpret_cast<T1DecState *>(rec + T1DS_STATE);
    uint64_t *const pl = planes + (size_t)jid * T1L_PLANE_WORDS + lane;
    uint32_t *const rawwords = t1l_rawbits(planes, njobs, jid);
    if (k == 0) {
        t1l_row(masks, group, T1L_REF, lane)[l] = 0; t1l_row(masks, group, T1L_MEMB, lane)[l] = 0;
        if (lane == 0) { stp->nmr = 0; *reinterpret_cast<uint32_t *>(rec + T1DS_BITS) = 0u; }
        const uint8_t *body = stream + offs[jid];
        uint32_t m, rawlen;
        t1_raw_split(body, lens[jid], m, rawlen);
        t1l_raw_unstuff(lane, body + T1_RAW_HDR + m, rawlen, (uint32_t)(nb0 * w * h), rawwords, &stage[0][0]);
        return;
    }
    const uint32_t nmr = t1l_plane_work<true>(lane, w, h, p, k, rec, masks, group, l, pl, stage, rawwords);
    if (lane == 0 && p >= 0) stp->nmr = nmr;
}

// t1.go:1281-1289 after the last launch: every sample's magnitude from the block's bit-plane words, its sign from the sign mask.  A
// wavefront per block, lanes = columns, one row per trip; the words of a row are wave-uniform loads.
__global__ __launch_bounds__(64) void t1_dec_assemble_kernel(const BlockJob *__restrict__ jobs, int njobs, const uint8_t *__restrict__ numbps,
                                                             int32_t *__restrict__ decoded, const uint64_t *__restrict__ masks,
                                                             const uint32_t *__restrict__ slot_of, const uint64_t *__restrict__ planes, int skip_uniform, const uint8_t *__restrict__ floors) {
    const int jid = blockIdx.x;
    if (jid >= njobs) return;
    const int skip_planes = t1_floor_of(skip_uniform, floors, jid);       // this block's floor: the call's, or its own if that is higher
    const int nb0 = (int)numbps[jid];
    if (nb0 > T1DS_MAXP) return;
    const int nb = max(nb0 - skip_planes, 0);                  // the planes that were decoded: word q holds bit plane q + skip_planes
    const BlockJob J = jobs[jid];
    const int w = J.w, h = J.h;
    if (w > 64 || h > 64) return;
    const int lane = threadIdx.x;
    int32_t *out = decoded + J.out_off;
    if (nb == 0) {                                              // no planes (or none above the floor): T1.Decode leaves the zeroed data (t1.go:1261-1289)
        for (int i = lane; i < w * h; i += 64) out[i] = 0;
        return;
    }
    const uint32_t slot = slot_of[jid];
    const uint64_t *neg = masks + ((((size_t)(slot >> 6)) * T1L_NA + T1L_NEG) * 64) * 64 + (slot & 63);     // + 64 * row
    const uint64_t *pl = planes + (size_t)jid * T1L_PLANE_WORDS;                                              // + 64 * plane + row
    const bool hi_half = lane >= 32;
    const uint32_t sh = (uint32_t)lane & 31u;
    const uint32_t mid = t1_coarse_mid(skip_planes);
    for (int y = 0; y < h; y++) {
        uint32_t v = 0;
        for (int q = 0; q < nb; q++) {
            const uint64_t pw = pl[64 * q + y];
            v |= (((hi_half ? (uint32_t)(pw >> 32) : (uint32_t)pw) >> sh) & 1u) << q;
        }
        v = v ? v << skip_planes | mid : 0u;
        const uint64_t ng = neg[64 * y];
        if (((hi_half ? (uint32_t)(ng >> 32) : (uint32_t)ng) >> sh) & 1u) v = 0u - v;
        if (lane < w) out[(size_t)y * w + lane] = (int32_t)v;
    }
}
