// dwt53_l0pix.inc -- level 0 of the 5-3 forward transform for packed RGBA8 frames (the C2 / C4 headline path), included
// by dwt53.hip (product) and tools/probe/l0_fwd_dev.hip (stand-alone timing + check against a CPU restatement).
//
// Replaces, fused: encoder.extractImageData's RGBA branch (encoder.go:107-123), mct.DCLevelShiftForward (mct.go:96-101),
// mct.ForwardRCT (mct.go:28-38), dwt.Forward2D53 (dwt.go:356-407) as level 0 of DecomposeMultiLevel53 (dwt.go:524-531).
//
// Why this is not dwt53_fwd_kernel<8,3,true,false,true> (round 1): that kernel marches a band of pair-rows per wavefront
// with ~170 VGPRs -- at most 3 waves per SIMD, one dependent load -> compute -> store chain per wave, 3440 waves over 3072
// slots -- and reaches 4.3-4.5 TB/s.  tools/probe/l0_probe.hip (same byte mix, no arithmetic) shows what the memory system
// gives: 5.0-6.0 TB/s when MANY SHORT waves each put all their loads in flight at once, 4.3 TB/s when few long waves march.
// Measured on the way here (tools/probe/l0_fwd_dev.hip, 4K frame, per-launch events, cache-resident / 945 MB footprint):
//   general kernel (round 1)                                                  30-31 us in bench.py
//   one wave = 1..4 pair-rows, halo rows re-read and recomputed, no LDS       25.0 / 30.6 us (1450 instructions per pair-row,
//                                                                             168 VGPRs; not memory-bound any more)
//   workgroup form below, plain stores                                        21.8 / 29.5 us
//   workgroup form below, nt stores of the final coefficients                 20.9 / 25.6 us  (0.79 / 0.65 of 8 TB/s)
// 8-bit input lets the arithmetic be restated without changing a bit: with raw bytes R, G, B and c = dc_shift,
//     Y = ((R-c) + 2(G-c) + (B-c)) >> 2 = ((R + 2G + B) >> 2) - c,   U = B - G,   V = R - G              (mct.go:28-38)
// and a constant offset on the input of the 5-3 lifting appears unchanged in its low-pass output and not at all in its
// high-pass output (floor((a - c + b - c) / 2) = floor((a + b) / 2) - c), so the kernel lifts Y + c and subtracts c from the
// LL quadrant of Y only (4 subtractions per pair-row instead of 48); all intermediates stay below 2^12, so (e + e) >> 1 == e
// and the mirror rules of dwt.go:89-99 become DPP `old` operands instead of selects.
// Geometry contract (checked by the plan before choosing this kernel): every plane 16 <= w <= 512, w % 8 == 0, h >= 2,
// 16-byte aligned rows.  Everything else takes the general kernel.

// Final-coefficient store flavours (template parameter NT of the kernels below): 0 plain, 1 nt, 2 sc1, 3 sc0 sc1, 4 sc1 nt.
// As inline asm: with __builtin_nontemporal_store on one side of a branch hipcc merges the two sides into one plain store
// with a selected address and the hint is lost (seen in the .s: no " nt" on any store).
template <int FL>
__device__ __forceinline__ void st_final(v4i *p, const v4i &v) {
    // The s_nop is part of the store: the hardware reads a > 64-bit store's data registers over the cycles after issue
    // (the "VMEM store data" hazard), and the compiler's hazard recogniser does not look inside inline asm -- without it
    // a VALU write to v's registers scheduled right behind the asm (an address for the next store, seen in the fused
    // kernel: v_lshl_add_u64 into the first two data registers) lands in memory instead of the data.
    if constexpr (FL == 1) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else if constexpr (FL == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else if constexpr (FL == 3) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else if constexpr (FL == 4) asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else *p = v;
}

// The 16-bit hand-off to the deep launch (option l0_scr16; dwt53_fwd_rgba8_wg16_kernel -> dwt53_deep_fwd16_kernel).  What level 0 of a
// packed 8-bit frame sends to `nxt` is bounded whatever the pixels are.  With raw bytes R, G, B the lifted inputs are Y + c =
// (R + 2G + B) >> 2 in [0, 255] and U = B - G, V = R - G in [-255, 255]: |x| <= M = 255.  One 1-D lifting step of values |x| <= M gives
//     d = x_odd - ((x_e + x_e') >> 1),  |d| <= 2M;      s = x_e + ((d + d' + 2) >> 2),  |s| <= M + ((4M + 2) >> 2) = 2M,
// so after the horizontal and the vertical step every L / H half-row element is within 4M = 1020, and the LL quadrant of Y has the DC
// shift c subtracted once more: |value| <= 4 * 255 + 3 + c (the + 3 is slack, not needed), 1151 for c = 128 -- 12 bits of int16's 16.
// The plan checks J2K_SCR16_BOUND + dc_shift against INT16_MAX before it chooses these kernels (j2k_planbuild.cpp), so the
// truncation below drops only copies of the sign bit and the reader's sign extension gives the int32 back.
// p = the row's slot + 2 * lane int32s, i.e. int16 element 4 * lane of the row: one 8-byte store instead of a 16-byte one.
__device__ __forceinline__ void st_scr16(int32_t *p, const v4i &v) {
    const unsigned lo = __builtin_amdgcn_perm((unsigned)v.y, (unsigned)v.x, 0x05040100u);      // low halves of x | y << 16
    const unsigned hi = __builtin_amdgcn_perm((unsigned)v.w, (unsigned)v.z, 0x05040100u);
    *reinterpret_cast<v2i *>(p) = (v2i){(int)lo, (int)hi};
}


// ================================================================================================================
// Workgroup form (round 2, the one the plan launches): NO recomputation.  A workgroup of NW wavefronts owns NW-1
// consecutive pair-rows of one <= 512-column tile plane; wave i loads exactly its two source rows (all four 16-byte
// loads in flight at once), runs the horizontal pass on them and the waves exchange what the vertical lifting needs
// through LDS:
//   slot[i]   <- E_i   (the horizontally lifted even row of wave i)                     | barrier
//   wave i reads E_{i+1} from slot[i+1], forms d_i = O_i - ((E_i + E_{i+1}) >> 1) and overwrites slot[i+1] with d_i
//   (slot[i+1]'s E is read by wave i only, so the slot can be recycled at once)          | barrier
//   wave i reads d_{i-1} from slot[i], s_i = E_i + ((d_{i-1} + d_i + 2) >> 2), stores s_i and d_i.
// The last wave of the workgroup is a HELPER: it loads the three halo rows (two above the band, one below), publishes
// the even row below into slot[NW-1] and d of the pair-row above into slot[0]; it stores nothing.  So every source row
// is read once plus 3 rows per workgroup (read side = a quarter of the traffic), every wave runs ~500 instructions at
// <= 128 VGPRs, and a 4K frame is ~9900 short independent waves with all their loads issued in their first cycles.
// 24 dwords per lane and exchange as six b128 accesses, lane-contiguous (conflict-free); 6 KB of LDS per wave.
// ================================================================================================================
// The workgroup's work over `slot` (NW x 6 x 64 v4i of LDS) as a device function, for dwt53_mega_fwd_kernel (dwt53_deep.inc):
// NW = 16 on its dynamic LDS, for the bands that run beside the deep levels.
template <int NW, int NT>
__device__ __forceinline__ void dwt53_fwd_rgba8_wg_body(v4i (&slot)[NW][6][64], const DwtJob job, const DwtPlane *__restrict__ planes,
                                                        const uint32_t *__restrict__ pix, int32_t *__restrict__ out, int32_t *__restrict__ nxt,
                                                        int dc_shift, int pix_stride) {
    constexpr bool MAL = false;                    // (the merged launch is not built for Mallat plans)
    constexpr bool S16 = false;                    // (... nor for the 16-bit hand-off)
#include "dwt53_l0pix_fwd_body.inc"
}
// MAL: the level 0 of a Mallat plan (the body's store_row)
template <int NW, int NT, int WPE, bool MAL = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt53_fwd_rgba8_wg_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes,
                               const uint32_t *__restrict__ pix, int32_t *__restrict__ out, int32_t *__restrict__ nxt,
                               int dc_shift, int pix_stride) {
    __shared__ v4i slot[NW][6][64];
    const DwtJob job = jobs[blockIdx.x];           // uniform: scalar loads
    if (job.plane < 0) return;                     // padding entry of the XCD-aware job order (whole workgroup, before any barrier)
    constexpr bool S16 = false;
#include "dwt53_l0pix_fwd_body.inc"
}
// The same workgroup with the rows of X_1 stored as int16 (st_scr16; option l0_scr16): a kernel of its own name, so that the one above
// stays what it was.  Prefix plans only, and only when dwt53_deep_fwd16_kernel reads the scratch next (plan_forward_impl).
template <int NW, int NT, int WPE>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt53_fwd_rgba8_wg16_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes,
                                 const uint32_t *__restrict__ pix, int32_t *__restrict__ out, int32_t *__restrict__ nxt,
                                 int dc_shift, int pix_stride) {
    __shared__ v4i slot[NW][6][64];
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    constexpr bool MAL = false, S16 = true;
#include "dwt53_l0pix_fwd_body.inc"
}
// The same workgroup over an image.YCbCr (encoder.go:178-195, the default branch; j2k_plan_forward_image): SRC = 1 + J2K_YCBCR_444 /
// 422 / 420 selects the body's second row source, which loads the Y and chroma bytes of a row and converts them in registers to
// the packed pixels the RGBA8 source would have loaded (J2K_L0_YCC: the RGBA8 kernels above are compiled without it).
#define J2K_L0_YCC 1
template <int NW, int NT, int WPE, int SRC>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt53_fwd_ycc_wg_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes, const YccSrc ycc,
                             int32_t *__restrict__ out, int32_t *__restrict__ nxt, int dc_shift) {
    static_assert(SRC >= 1 + J2K_YCBCR_444 && SRC <= 1 + J2K_YCBCR_420, "YCbCr 4:4:4, 4:2:2, 4:2:0 only");
    __shared__ v4i slot[NW][6][64];
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    constexpr bool MAL = false;                    // (prefix plans only: plan_rgba8_wg_fusable)
    constexpr bool S16 = false;                    // (the YCbCr source keeps the int32 hand-off)
#include "dwt53_l0pix_fwd_body.inc"
}
#undef J2K_L0_YCC

// ================================================================================================================
// Inverse counterpart: level 0 of ReconstructMultiLevel53 (dwt.go:534-548) = Inverse2D53 (dwt.go:410-429, columns first,
// then rows) + mct.InverseRCT (mct.go:56-66) + mct.DCLevelShiftInverse (mct.go:113-118) + decoder.createImage's RGBA branch
// (decoder.go:477-505: clamp to 0..255, alpha 255), straight to the packed RGBA8 frame.
// Same workgroup shape: wave i owns pair-row q = q0 + i, loads its low-pass row s_q and high-pass row d_q (twelve 16-byte
// loads, all in flight at once) and the waves exchange through LDS
//   slot[i+1] <- d_q                                                                        | barrier
//   wave i reads d_{q-1} from slot[i], e_q = s_q - ((d_{q-1} + d_q + 2) >> 2), recycles slot[i] for e_q     | barrier
//   wave i reads e_{q+1} from slot[i+1], o_q = d_q + ((e_q + e_{q+1}) >> 1); then the horizontal inverse of rows e_q, o_q
//   across the wave (DPP), inverse RCT, + dc, clamp, pack, two 16-byte nt stores per row.
// The helper wave supplies d_{q0-1} (slot[0]) and e_{q0+NR} (slot[NR], which needs the last regular wave's d).
// Coefficients are arbitrary int32 here (a decoder's input): every sum wraps like Go's int32 and the mirror rules are real
// selects, not the small-value shortcuts of the forward kernel.
// ================================================================================================================
// MAL: the level 0 of a Mallat plan -- load_row routes as inv_load_row<MAL> does: LL (the low half of a low-pass row, while there is a coarser
// level) from its dense (w/2) x ceil(h/2) result, every other half-row from the plane at row * coef_stride + column.
// S16 (dwt53_inv_rgba8_wg16_kernel, behind dwt53_deep_inv16_kernel; option l0_scr16 bit 1): a half-row of `prev` is int16 in the first half of its
// slot when its format byte says so (fmt[(nxt_off + row start) >> 3] = 1), else int32.  The 8-byte load of the narrow form and the byte are issued
// with the coefficient loads, addressed from the plane table alone -- neither waits for the other, so a narrow row costs no round trip more
// than before; only a row marked wide (a wave-uniform branch: one byte per half-row) pays a second one for its 16-byte load.
template <int NW, bool PARK, bool MAL = false, bool S16 = false>
__device__ __forceinline__ void dwt53_inv_rgba8_wg_body(v4i (&slot)[NW][PARK ? 8 : 6][64], const DwtJob job, const DwtPlane *__restrict__ planes,
                                                        const int32_t *__restrict__ coef, const int32_t *__restrict__ prev, uint32_t *__restrict__ pix,
                                                        int dc_shift, int pix_stride, const uint8_t *__restrict__ fmt = nullptr) {
    static_assert(!(S16 && MAL), "the 16-bit hand-off is not built for Mallat plans");
    constexpr int NR = NW - 1;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const DwtPlane P = planes[job.plane];
    const int w = P.w, h = P.h, halfH = (h + 1) >> 1, halfW = w >> 1, nhigh = h - halfH;
    const int c = lane * 8;
    const bool active = c < w;
    const bool last_lane = c + 8 >= w;
    const int q0 = job.prow0;
    const bool helper = wv == NR;
    const int q = q0 + wv;
    const bool live = !helper && q < halfH;
    const int lo4 = active ? lane * 4 : 0;          // clamped: idle lanes load valid addresses
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    auto wadd4 = [](const v4i &a, const v4i &b) { return (v4i)((u4)a + (u4)b); };
    auto wsub4 = [](const v4i &a, const v4i &b) { return (v4i)((u4)a - (u4)b); };
    // row `ro` of the level matrix: v[2k] = L part, v[2k+1] = H part of component k; elements below n_next come from the
    // coarser level's output (prev), the rest from the coefficient plane -- uniform per half-row (n_next % (w/2) == 0)
    auto load_row = [&](int ro, v4i (&v)[6]) {
        if constexpr (MAL) {
            const bool ll = P.n_next != 0 && ro < halfH;
            const int offP = ro * P.coef_stride + lo4, offL = ll ? ro * halfW + lo4 : offP;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                v[2 * k] = *reinterpret_cast<const v4i *>((ll ? prev + P.nxt_off[k] : coef + P.src_off[k]) + offL);
                v[2 * k + 1] = *reinterpret_cast<const v4i *>(coef + P.src_off[k] + offP + halfW);
            }
            return;
        }
        const int idxL = ro * w + lo4, idxH = idxL + halfW;
        const bool finL = ro * w >= P.n_next, finH = ro * w + halfW >= P.n_next;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v[2 * k] = *reinterpret_cast<const v4i *>((finL ? coef + P.src_off[k] : prev + P.nxt_off[k]) + idxL);
            v[2 * k + 1] = *reinterpret_cast<const v4i *>((finH ? coef + P.src_off[k] : prev + P.nxt_off[k]) + idxH);
        }
    };
    // S16, a low-pass row (the only rows with halves below n_next): the loads ...
    [[maybe_unused]] auto load_row16 = [&](int ro, v4i (&v)[6], int (&f)[6]) {
        const int rowL = ro * w, rowH = rowL + halfW;
        const bool finL = rowL >= P.n_next, finH = rowH >= P.n_next;
#pragma unroll
        for (int k = 0; k < 3; k++) {
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
                const int row = hf ? rowH : rowL;
                if (hf ? finH : finL) {
                    v[2 * k + hf] = *reinterpret_cast<const v4i *>(coef + P.src_off[k] + row + lo4);
                    f[2 * k + hf] = 1;
                } else {
                    const v2i t = *reinterpret_cast<const v2i *>(prev + P.nxt_off[k] + row + (lo4 >> 1));      // int16 element 4 * lane
                    v[2 * k + hf] = (v4i){t.x, t.y, 0, 0};
                    f[2 * k + hf] = fmt[(P.nxt_off[k] + row) >> 3];
                }
            }
        }
    };
    // ... and what they mean: a narrow half-row is sign-extended, one marked wide is loaded again as int32
    [[maybe_unused]] auto fix_row16 = [&](int ro, v4i (&v)[6], const int (&f)[6]) {
        const int rowL = ro * w, rowH = rowL + halfW;
        const bool finL = rowL >= P.n_next, finH = rowH >= P.n_next;
#pragma unroll
        for (int k = 0; k < 3; k++) {
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
                if (hf ? finH : finL) continue;
                const int row = hf ? rowH : rowL;
                if (__builtin_amdgcn_readfirstlane(f[2 * k + hf])) {
                    const int a = v[2 * k + hf].x, b = v[2 * k + hf].y;
                    v[2 * k + hf] = (v4i){(int)(short)a, a >> 16, (int)(short)b, b >> 16};
                } else {
                    v[2 * k + hf] = *reinterpret_cast<const v4i *>(prev + P.nxt_off[k] + row + lo4);
                }
            }
        }
    };
    v4i S[6], D[6];
    const v4i two = {2, 2, 2, 2};
    if (helper) {
        // d of the pair-row above the band -> slot[0]; s, d of the pair-row below it stay in registers for phase 2
        // (d above first, on its own: with all three rows in flight the helper path holds 72 data VGPRs and sets the kernel's
        //  register count; the helper has nothing else to do in this phase, so its second round trip costs nothing)
        {
            v4i Da[6];
            load_row(halfH + min(max(q0 - 1, 0), max(nhigh - 1, 0)), Da);
#pragma unroll
            for (int v = 0; v < 6; v++) slot[0][v][lane] = Da[v];
        }
        asm volatile("" ::: "memory");
        if constexpr (S16) {
            int f[6];
            load_row16(min(q0 + NR, halfH - 1), S, f);
            load_row(halfH + min(q0 + NR, max(nhigh - 1, 0)), D);
            fix_row16(min(q0 + NR, halfH - 1), S, f);
        } else {
        load_row(min(q0 + NR, halfH - 1), S);
        load_row(halfH + min(q0 + NR, max(nhigh - 1, 0)), D);
        }
    } else if (live) {
        if constexpr (S16) {
            int f[6];
            load_row16(q, S, f);
            load_row(halfH + min(q, max(nhigh - 1, 0)), D);
            fix_row16(q, S, f);
        } else {
        load_row(q, S);
        load_row(halfH + min(q, max(nhigh - 1, 0)), D);      // odd height: the last pair-row has no d row (clamped, unused)
        }
#pragma unroll
        for (int v = 0; v < 6; v++) slot[wv + 1][v][lane] = D[v];
    }
    __syncthreads();
    // undo update (dwt.go:132-138): e_q = s_q - ((d_{q-1} + d_q + 2) >> 2); d_{-1} := d_0; no d_q (odd height, last row) := d_{q-1}
    const int qq = helper ? q0 + NR : q;
    if ((helper && qq < halfH) || live) {
        const int sl = helper ? NR : wv;
        const bool has_d = qq < nhigh;
#pragma unroll
        for (int v = 0; v < 6; v++) {
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
        for (int v = 0; v < 6; v++) {
            const v4i En = has_next ? slot[wv + 1][v][lane] : S[v];
            D[v] = wadd4(D[v], has_next ? wadd4(S[v], En) >> 1 : S[v]);   // D becomes o
        }
    }
    const int64_t y0 = P.out_off[0] / P.out_stride;
    uint32_t *base = pix + y0 * pix_stride + (P.out_off[0] - y0 * P.out_stride);
    // staging for the pixel rows (below): 2 KB of this wave's slot[wv + 1], whose e_{q+1} only this wave reads -- and has read
    v4i *stage = &slot[wv + 1][PARK ? 6 : 0][0];
    // horizontal inverse of one row (dwt.go:122-147 across the wave) + inverse RCT + dc + clamp + pack
    auto finish_row = [&](int r, const v4i (&v)[6]) {
        int x[3][8];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const v4i lo = v[2 * k], hi = v[2 * k + 1];
            const int dleft = __builtin_amdgcn_update_dpp(hi[0], hi[3], 0x138, 0xf, 0xf, false);   // lane 0: d[-1] := d[0]
            int e[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                e[j] = (int)((unsigned)lo[j] - (unsigned)((int)((unsigned)(j > 0 ? hi[j - 1] : dleft) + (unsigned)hi[j] + 2u) >> 2));
            const int eright = __builtin_amdgcn_update_dpp(e[3], e[0], 0x130, 0xf, 0xf, false);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int en = j < 3 ? e[j + 1] : eright;
                int pred = (int)((unsigned)e[j] + (unsigned)en) >> 1;
                if (j == 3) pred = last_lane ? e[3] : pred;              // last odd sample of an even-length row
                x[k][2 * j] = e[j];
                x[k][2 * j + 1] = (int)((unsigned)hi[j] + (unsigned)pred);
            }
        }
        uint32_t px[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int y_ = x[0][i], u_ = x[1][i], v_ = x[2][i];
            const int g_ = (int)((unsigned)y_ - (unsigned)((int)((unsigned)u_ + (unsigned)v_) >> 2));
            const int r_ = (int)((unsigned)v_ + (unsigned)g_), b_ = (int)((unsigned)u_ + (unsigned)g_);
            const int rc = min(max((int)((unsigned)r_ + (unsigned)dc_shift), 0), 255), gc = min(max((int)((unsigned)g_ + (unsigned)dc_shift), 0), 255),
                      bc = min(max((int)((unsigned)b_ + (unsigned)dc_shift), 0), 255);
            px[i] = (uint32_t)rc | (uint32_t)gc << 8 | (uint32_t)bc << 16 | 0xFF000000u;
        }
        // A lane holds 8 consecutive pixels = 32 bytes; stored from there, each store instruction would write 16-byte pieces
        // 32 bytes apart (half of every 128-byte line per instruction).  Through LDS the row becomes lane-contiguous per
        // instruction: lane l stores bytes [16 l, 16 l + 16) and [1024 + 16 l, ...) -- tools/probe/l0_inv_probe.hip: 5.44 ->
        // 5.73 TB/s for this byte mix at an HBM footprint.
        const v4i v0 = {(int)px[0], (int)px[1], (int)px[2], (int)px[3]}, v1 = {(int)px[4], (int)px[5], (int)px[6], (int)px[7]};
        stage[2 * lane] = v0;
        stage[2 * lane + 1] = v1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // same wave: no barrier, the LDS returns in order
        const v4i t0 = stage[lane], t1 = stage[64 + lane];
        uint32_t *p = base + (int64_t)r * pix_stride;
        if (lane * 4 < w) __builtin_nontemporal_store(t0, reinterpret_cast<v4i *>(p + lane * 4));
        if (256 + lane * 4 < w) __builtin_nontemporal_store(t1, reinterpret_cast<v4i *>(p + 256 + lane * 4));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the reads are done before the next row overwrites the stage
    };
    // The odd row waits in LDS while the even row is finished (slot[wv + 1] held e_{q+1}, which only this wave reads): 24
    // fewer live VGPRs across the horizontal pass -- the difference between 5 and 7 waves per SIMD.  (The asm fence keeps the
    // compiler from forwarding the stored values to the reload, which would keep them in registers after all.)
    if (PARK) {
#pragma unroll
        for (int v = 0; v < 6; v++) slot[wv + 1][v][lane] = D[v];
        asm volatile("" ::: "memory");
    }
    finish_row(2 * q, S);
    if (2 * q + 1 < h) {
        if (PARK) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int v = 0; v < 6; v++) D[v] = slot[wv + 1][v][lane];
        }
        finish_row(2 * q + 1, D);
    }
}
template <int NW, int WPE, bool PARK = (WPE > 5), bool MAL = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt53_inv_rgba8_wg_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes,
                               const int32_t *__restrict__ coef, const int32_t *__restrict__ prev, uint32_t *__restrict__ pix,
                               int dc_shift, int pix_stride, const int *__restrict__ guard) {
    __shared__ v4i slot[NW][PARK ? 8 : 6][64];        // (PARK: two more vectors per wave for the pixel-row staging)
    if (guard && *guard) return;             // (the frame decoder: a stream that was refused leaves the caller's frame alone)
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    dwt53_inv_rgba8_wg_body<NW, PARK, MAL>(slot, job, planes, coef, prev, pix, dc_shift, pix_stride);
}
// The same workgroup behind dwt53_deep_inv16_kernel: the half-rows of `prev` are int16 where fmt says so (the body's S16).  A kernel of its own
// name, so that the one above stays what it was; four waves, everything in registers (the default shape, all the plan sets the flag for).
template <int NW, int WPE>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt53_inv_rgba8_wg16_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes,
                                 const int32_t *__restrict__ coef, const int32_t *__restrict__ prev, uint32_t *__restrict__ pix,
                                 int dc_shift, int pix_stride, const int *__restrict__ guard, const uint8_t *__restrict__ fmt) {
    __shared__ v4i slot[NW][6][64];
    if (guard && *guard) return;
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    dwt53_inv_rgba8_wg_body<NW, false, false, true>(slot, job, planes, coef, prev, pix, dc_shift, pix_stride, fmt);
}

// ================================================================================================================
// Levels 0 AND 1 in one launch (forward).  The reference's multi-level layout (dwt.go:524-531: level 1 transforms the
// contiguous prefix data[0 : w1*h1] of the level-0 result as a dense w1 x h1 matrix, w1 = w/2, h1 = ceil(h/2)) makes the
// level-1 input rows 2t and 2t+1 the L half and the H half of level 0's low-pass row s_t -- exactly what wave t holds in
// registers after its vertical lifting.  So the same workgroup runs a second, half-width lifting pipeline on them: horizontal
// 5-3 on four values per lane, two more LDS exchanges (level-1 even row -> next wave, level-1 d -> previous wave), and the
// level-1 results go straight to the coefficient plane / to the scratch that feeds level 2.  The 25 MB prefix of a 4K frame is
// never written and never read back, and the level-1 launch disappears.
// Price: a band of NR level-1 pair-rows needs s of one pair-row above and one below, i.e. level-0 d of two above and one
// below: NW = NR + 3 waves (wave i owns pair-row t = q0 - 2 + i; the outer three store nothing), the last wave transforms the
// even row below itself.  Only the bands of the top half of a plane (t < ceil(h1/2)) are launched this way; the rest takes
// dwt53_fwd_rgba8_wg_kernel.  Level-0 rows of a fused band that lie past the prefix are stored as usual.
// ================================================================================================================
template <int NW, int NT, int WPE>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void dwt53_fwd_rgba8_wg2_kernel(const DwtJob *__restrict__ jobs, int njobs, const DwtPlane *__restrict__ planes,
                                const DwtPlane *__restrict__ planes1, const uint32_t *__restrict__ pix, int32_t *__restrict__ out,
                                int32_t *__restrict__ nxt1, int dc_shift, int pix_stride) {
    typedef int v2i_ __attribute__((ext_vector_type(2)));
    __shared__ v4i slot[NW][6][64];         // slot[0] first carries the even row BELOW the band (wave 0's own e has no reader)
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const DwtJob job = jobs[blockIdx.x];
    if (job.plane < 0) return;
    const DwtPlane P = planes[job.plane];
    const int w = P.w, h = P.h, halfH = (h + 1) >> 1, halfW = w >> 1;
    const int c = lane * 8;
    const bool active = c < w;
    const bool last_lane = c + 8 >= w;
    const int q0 = job.prow0;
    const int t = q0 - 2 + wv;                                 // my pair-row
    const bool live = t >= 0 && t < halfH;
    const bool is_out = wv >= 2 && wv < NW - 1;                // the outer three waves only feed their neighbours
    const bool has_odd = live && 2 * t + 1 < h, has_next = live && 2 * t + 2 < h;
    // level 1: w1 x h1 matrix whose rows 2t, 2t+1 are the halves of s_t
    const int w1 = halfW, h1 = halfH, halfH1 = (h1 + 1) >> 1, halfW1 = w1 >> 1;
    const bool in1 = live && t < halfH1;                        // the L half of s_t is level-1 row 2t
    const bool odd1 = in1 && 2 * t + 1 < h1;                    // the H half of s_t is level-1 row 2t+1
    const bool next1 = in1 && 2 * t + 2 < h1;                   // level-1 row 2t+2 exists
    const int n_next1 = planes1[job.plane * 3].n_next;
    const int64_t y0 = P.src_off[0] / P.src_stride;
    const uint32_t *base = pix + y0 * pix_stride + (P.src_off[0] - y0 * P.src_stride) + (active ? c : 0);
    auto rowp = [&](int r) { return reinterpret_cast<const uint4 *>(base + (int64_t)min(max(r, 0), h - 1) * pix_stride); };

    auto hrow = [&](const uint4 &a, const uint4 &b, v4i (&v)[6]) {       // as in dwt53_fwd_rgba8_wg_kernel
        const uint32_t px[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            int x[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int R = (int)(px[i] & 0xFF), G = (int)((px[i] >> 8) & 0xFF), B = (int)((px[i] >> 16) & 0xFF);
                x[i] = (k == 0) ? (R + 2 * G + B) >> 2 : (k == 1 ? B - G : R - G);
            }
            int er = __builtin_amdgcn_update_dpp(x[6], x[0], 0x130, 0xf, 0xf, false);
            er = last_lane ? x[6] : er;
            int d[4];
#pragma unroll
            for (int j = 0; j < 4; j++) d[j] = x[2 * j + 1] - ((x[2 * j] + (j < 3 ? x[2 * j + 2] : er)) >> 1);
            const int dl = __builtin_amdgcn_update_dpp(d[0], d[3], 0x138, 0xf, 0xf, false);
#pragma unroll
            for (int j = 0; j < 4; j++) v[2 * k][j] = x[2 * j] + (((j > 0 ? d[j - 1] : dl) + d[j] + 2) >> 2);
            v[2 * k + 1] = (v4i){d[0], d[1], d[2], d[3]};
        }
    };
    // level-1 horizontal pass of one half-row (4 values per lane): {lo0, lo1, hi0, hi1}
    auto hrow1 = [&](const v4i &x) -> v4i {
        int er = __builtin_amdgcn_update_dpp(x[2], x[0], 0x130, 0xf, 0xf, false);
        er = last_lane ? x[2] : er;
        const int d0 = x[1] - ((x[0] + x[2]) >> 1), d1 = x[3] - ((x[2] + er) >> 1);
        const int dl = __builtin_amdgcn_update_dpp(d0, d1, 0x138, 0xf, 0xf, false);
        return (v4i){x[0] + ((dl + d0 + 2) >> 2), x[2] + ((d0 + d1 + 2) >> 2), d0, d1};
    };
    auto store_half0 = [&](int k, int64_t idx, const v4i &v) {             // a final level-0 half-row
        st_final<NT>(reinterpret_cast<v4i *>(out + P.out_off[k] + idx), v);
    };

    v4i E[6], O[6];
    if (live) {
        const uint4 *p0 = rowp(2 * t), *p1 = rowp(2 * t + 1), *p2 = rowp(2 * t + 2);
        const uint4 a0 = p0[0], b0 = p0[1], a1 = p1[0], b1 = p1[1];
        uint4 a2 = a0, b2 = b0;
        if (wv == NW - 1) { a2 = p2[0]; b2 = p2[1]; }
        hrow(a0, b0, E);
        if (wv > 0) {
#pragma unroll
            for (int v = 0; v < 6; v++) slot[wv][v][lane] = E[v];
        }
        hrow(a1, b1, O);
        if (wv == NW - 1) {                                       // the last wave transforms the even row below itself
            v4i N[6];
            hrow(a2, b2, N);
#pragma unroll
            for (int v = 0; v < 6; v++) slot[0][v][lane] = N[v];
        }
    }
    __syncthreads();
    if (has_odd) {
        if (has_next) {
#pragma unroll
            for (int v = 0; v < 6; v++) {
                const v4i En = slot[(wv + 1) % NW][v][lane];
                O[v] = O[v] - ((E[v] + En) >> 1);                // O becomes d
            }
        } else {
#pragma unroll
            for (int v = 0; v < 6; v++) O[v] = O[v] - E[v];
        }
        if (wv < NW - 1) {
#pragma unroll
            for (int v = 0; v < 6; v++) slot[wv + 1][v][lane] = O[v];
        }
    }
    __syncthreads();
    v4i E1[3], O1[3];
    if (live) {
        v4i Dp[6];
#pragma unroll
        for (int v = 0; v < 6; v++) Dp[v] = slot[wv][v][lane];   // wave 0 reads its own e back: garbage that no stored result depends on
        if (!has_odd) {
#pragma unroll
            for (int v = 0; v < 6; v++) O[v] = Dp[v];
        }
        if (t == 0) {
#pragma unroll
            for (int v = 0; v < 6; v++) Dp[v] = O[v];
        }
#pragma unroll
        for (int v = 0; v < 6; v++) E[v] = E[v] + ((Dp[v] + O[v] + 2) >> 2);      // E becomes s
        E[0] = E[0] - dc_shift;                                                     // the LL quadrant of Y (see the header)
        if (is_out && active) {
            const int64_t idxL = (int64_t)t * w + lane * 4;
            if (has_odd) {                                                          // d rows are always past the prefix
                const int64_t idxD = (int64_t)(halfH + t) * w + lane * 4;
#pragma unroll
                for (int k = 0; k < 3; k++) { store_half0(k, idxD, O[2 * k]); store_half0(k, idxD + halfW, O[2 * k + 1]); }
            }
            if (!in1) {
#pragma unroll
                for (int k = 0; k < 3; k++) { store_half0(k, idxL, E[2 * k]); store_half0(k, idxL + halfW, E[2 * k + 1]); }
            } else if (!odd1) {                                                     // odd h1: the last H half is not a level-1 row
#pragma unroll
                for (int k = 0; k < 3; k++) store_half0(k, idxL + halfW, E[2 * k + 1]);
            }
        }
        if (in1) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                E1[k] = hrow1(E[2 * k]);
                O1[k] = hrow1(E[2 * k + 1]);
                slot[wv][k][lane] = E1[k];
            }
        }
    }
    __syncthreads();
    if (odd1) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const v4i En = (next1 && wv < NW - 1) ? slot[wv + 1][k][lane] : E1[k];
            O1[k] = O1[k] - (next1 ? (E1[k] + En) >> 1 : E1[k]);                    // O1 becomes the level-1 d
        }
        if (wv < NW - 1) {
#pragma unroll
            for (int k = 0; k < 3; k++) slot[wv + 1][k][lane] = O1[k];
        }
    }
    __syncthreads();
    if (!in1 || !is_out || !active) return;
    {
        const int64_t o1[3] = {planes1[job.plane * 3 + 0].out_off[0], planes1[job.plane * 3 + 1].out_off[0], planes1[job.plane * 3 + 2].out_off[0]};
        const int64_t x1[3] = {planes1[job.plane * 3 + 0].nxt_off[0], planes1[job.plane * 3 + 1].nxt_off[0], planes1[job.plane * 3 + 2].nxt_off[0]};
        auto store1 = [&](int k, int ro1, const v4i &v) {           // one level-1 row of component k: {L, L, H, H}
            const int64_t idxL = (int64_t)ro1 * w1 + lane * 2, idxH = idxL + halfW1;
            const bool finL = ro1 * w1 >= n_next1, finH = ro1 * w1 + halfW1 >= n_next1;
            *reinterpret_cast<v2i_ *>((finL ? out + o1[k] : nxt1 + x1[k]) + idxL) = (v2i_){v[0], v[1]};
            *reinterpret_cast<v2i_ *>((finH ? out + o1[k] : nxt1 + x1[k]) + idxH) = (v2i_){v[2], v[3]};
        };
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v4i Dp = slot[wv][k][lane];
            if (!odd1) O1[k] = Dp;
            if (t == 0) Dp = O1[k];
            const v4i s1 = E1[k] + ((Dp + O1[k] + 2) >> 2);
            store1(k, t, s1);
            if (odd1) store1(k, halfH1 + t, O1[k]);
        }
    }
}
