// rate.hip -- rate control of the MQ block coder (a feature of this library; the reference reads Options.CompressionRatio nowhere): the
// distortion of every block at every plane cut, and the allocation of a byte budget over the blocks' (rate, distortion) tables.
// tests/rate_cases.py is the definition both kernels agree with bit for bit; DESIGN.md 7 has the argument.
//
//   rate[j * 32 + p]   bytes of block j's codeword that decode its first p bit planes (t1.hip, the PLANES instantiations), p = 0 ... numBPS
//   dist[j * 32 + p]   sum over the block of (|v| - |coarse(v, numBPS - p)|)^2 in wrapping uint64 arithmetic (0 above numBPS)
//                      (region of interest, tests/roi_cases.py: the samples that reconstruct a rectangle of the frame count `gain` times)
//   kept[j]            the planes the allocation keeps of block j
#include "area_walk.h"

namespace j2k {

#define RATE_STRIDE 32

// One wavefront per block, lanes = columns.  Every sample adds to the sum of each floor k = 1 ... numBPS: what a decoder that stops after
// plane k leaves of the magnitude is |v| with its low k bits replaced by the midpoint 2^(k-1), or nothing where |v| < 2^k.
// KMAX: the floors this instantiation sums (the block's numBPS <= KMAX): a block of 8 planes does not pay for 31.  Lane k returns floor k's sum.
template <int KMAX>
__device__ __forceinline__ uint64_t rate_distortion_sums(const BlockJob &J, const int32_t *__restrict__ src, int lane) {
    uint64_t acc[KMAX + 1];
#pragma unroll
    for (int k = 0; k <= KMAX; k++) acc[k] = 0;
    for (int y = 0; y < J.h; y++)
        for (int x = lane; x < J.w; x += 64) {
            const int32_t v = src[(size_t)y * J.stride + x];
            const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
#pragma unroll
            for (int k = 1; k <= KMAX; k++) {            // (floors above numBPS see |v| < 2^k and sum |v|^2: never stored)
                const uint32_t half = 1u << (k - 1), low = a & (2u * half - 1u);
                const uint32_t d = (a >> k) ? (low >= half ? low - half : half - low) : low;
                acc[k] += (uint64_t)d * d;
            }
        }
    uint64_t mine = 0;
#pragma unroll
    for (int k = 1; k <= KMAX; k++) {
        uint64_t s = acc[k];
        for (int o = 32; o > 0; o >>= 1) s += (uint64_t)__shfl_xor((unsigned long long)s, o);
        if (lane == k) mine = s;
    }
    return mine;
}

__global__ __launch_bounds__(64) void rate_distortion_kernel(const BlockJob *__restrict__ jobs, int njobs, const int32_t *__restrict__ coef,
                                                              const uint8_t *__restrict__ numbps, uint64_t *__restrict__ dist) {
    const int jid = blockIdx.x;
    if (jid >= njobs) return;
    const int lane = threadIdx.x;
    const BlockJob J = jobs[jid];
    const int nb = min((int)numbps[jid], RATE_STRIDE - 1);
    const int32_t *src = coef + J.src_off;
    uint64_t mine = 0;                                   // wave-uniform choice
    if (nb == 0) mine = 0;
    else if (nb <= 8) mine = rate_distortion_sums<8>(J, src, lane);
    else if (nb <= 12) mine = rate_distortion_sums<12>(J, src, lane);
    else if (nb <= 16) mine = rate_distortion_sums<16>(J, src, lane);
    else mine = rate_distortion_sums<RATE_STRIDE - 1>(J, src, lane);
    if (lane < RATE_STRIDE) dist[(size_t)jid * RATE_STRIDE + (lane <= nb ? nb - lane : lane)] = lane <= nb ? mine : 0;
}

// ---- pass cuts (tests/pass_cases.py): the distortion at every coding-pass end -------------------------------------------------------------
// dist[j * 96 + q], q = 3 p - 2 + s: p whole planes and s passes of plane b = nb - p - 1.  With e_k the error of a sample at floor k (above) and
// t its top bit, only the samples with t == b see plane b's first two passes differently from a whole-plane cut:
//   s = 0   sum e_{b+1}^2                                   (rate_distortion_sums' floor b + 1)
//   s = 1   the same, but e_b for the samples of t == b that turned significant in SigProp (spmask); e_{b+1} = |v| for them
//   s = 2   sum e_b^2, but |v| for the samples of t == b that wait for Cleanup
// so per floor k three sums: e_k^2 over all samples, and |v|^2 - e_k^2 over the samples of t == k with and without their spmask bit.
#define RATE_PASS_STRIDE 96
template <int KMAX>
__device__ __forceinline__ void rate_distortion_pass_sums(const BlockJob &J, const int32_t *__restrict__ src, const uint64_t *__restrict__ sprow, int lane,
                                                          uint64_t &all, uint64_t &insp, uint64_t &incl) {
    uint64_t acc[KMAX + 1], g[KMAX + 1], c[KMAX + 1];
#pragma unroll
    for (int k = 0; k <= KMAX; k++) acc[k] = g[k] = c[k] = 0;
    for (int y = 0; y < J.h; y++) {
        const uint64_t spm = sprow[y];
        for (int x = lane; x < J.w; x += 64) {               // (blocks <= 64 x 64: x = lane)
            const int32_t v = src[(size_t)y * J.stride + x];
            const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
            const int t = 31 - __clz((int)a);                // -1 for a = 0: matches no floor
            const bool sp = (spm >> (x & 63)) & 1;
            const uint64_t aa = (uint64_t)a * a;
#pragma unroll
            for (int k = 0; k <= KMAX; k++) {
                uint64_t dd = 0;
                if (k >= 1) {
                    const uint32_t half = 1u << (k - 1), low = a & (2u * half - 1u);
                    const uint32_t d = (a >> k) ? (low >= half ? low - half : half - low) : low;
                    dd = (uint64_t)d * d;
                }
                acc[k] += dd;
                const uint64_t gain = t == k ? aa - dd : 0;
                g[k] += sp ? gain : 0;
                c[k] += sp ? 0 : gain;
            }
        }
    }
    all = insp = incl = 0;
#pragma unroll
    for (int k = 0; k <= KMAX; k++) {
        uint64_t s0 = acc[k], s1 = g[k], s2 = c[k];
        for (int o = 32; o > 0; o >>= 1) {
            s0 += (uint64_t)__shfl_xor((unsigned long long)s0, o);
            s1 += (uint64_t)__shfl_xor((unsigned long long)s1, o);
            s2 += (uint64_t)__shfl_xor((unsigned long long)s2, o);
        }
        if (lane == k) { all = s0; insp = s1; incl = s2; }
    }
}

// One wavefront per block, a sibling of rate_distortion_kernel: lane k holds floor k's three sums and writes the cuts that end at that floor.
__global__ __launch_bounds__(64) void rate_distortion_passes_kernel(const BlockJob *__restrict__ jobs, int njobs, const int32_t *__restrict__ coef,
                                                                     const uint8_t *__restrict__ numbps, const uint64_t *__restrict__ spmask,
                                                                     uint64_t *__restrict__ dist) {
    const int jid = blockIdx.x;
    if (jid >= njobs) return;
    const int lane = threadIdx.x;
    const BlockJob J = jobs[jid];
    const int nb = min((int)numbps[jid], RATE_STRIDE - 1);
    uint64_t *D = dist + (size_t)jid * RATE_PASS_STRIDE;
    const int last = nb > 0 ? 3 * nb - 2 : 0;
    for (int q = last + lane; q < RATE_PASS_STRIDE; q += 64) D[q] = 0;       // (the last cut itself: floor 0, no error)
    if (nb == 0 || J.w > 64 || J.h > 64) return;                             // wave-uniform
    const int32_t *src = coef + J.src_off;
    const uint64_t *sprow = spmask + (size_t)jid * 64;
    uint64_t all = 0, insp = 0, incl = 0;
    if (nb <= 8) rate_distortion_pass_sums<8>(J, src, sprow, lane, all, insp, incl);
    else if (nb <= 12) rate_distortion_pass_sums<12>(J, src, sprow, lane, all, insp, incl);
    else if (nb <= 16) rate_distortion_pass_sums<16>(J, src, sprow, lane, all, insp, incl);
    else rate_distortion_pass_sums<RATE_STRIDE - 1>(J, src, sprow, lane, all, insp, incl);
    const uint64_t above = (uint64_t)__shfl_down((unsigned long long)all, 1);        // floor lane + 1's sum
    if (lane >= 1 && lane <= nb) D[lane == nb ? 0 : 3 * (nb - lane) - 2] = all;      // s = 0 at floor `lane` (floor 0: zero, written above)
    if (lane <= nb - 2) {                                                            // plane b = lane, p = nb - 1 - lane whole planes above it
        const int p = nb - 1 - lane;
        D[3 * p - 1] = above - insp;
        D[3 * p] = all + incl;
    }
}

// ---- region of interest: the distortion of the samples that reconstruct a rectangle of the frame counts `gain` times ----------------------
// tests/roi_cases.py is the definition: D_roi[p] = D[p] + (gain - 1) * D_in[p] (mod 2^64), D_in the same sum over the block's footprint F_j
// alone (area_walk.h: roi_window).  The footprint is a sub-window of the block, so D_in is rate_distortion_sums on a job of that window.
__device__ __forceinline__ uint64_t rate_distortion_of(int nb, const BlockJob &J, const int32_t *__restrict__ src, int lane) {
    if (nb <= 8) return rate_distortion_sums<8>(J, src, lane);
    if (nb <= 12) return rate_distortion_sums<12>(J, src, lane);
    if (nb <= 16) return rate_distortion_sums<16>(J, src, lane);
    return rate_distortion_sums<RATE_STRIDE - 1>(J, src, lane);
}

// One wavefront per block, as rate_distortion_kernel; blocks / planes: the tables of area_blocks_kernel (job j = block j).  Every choice below
// is wave-uniform: the block, its numBPS, the rectangle and the gain are.
__global__ __launch_bounds__(64) void rate_distortion_roi_kernel(const BlockJob *__restrict__ jobs, int njobs, const int32_t *__restrict__ coef,
                                                                  const uint8_t *__restrict__ numbps, const j2k_block *__restrict__ blocks,
                                                                  const AreaPlane *__restrict__ planes, int rx0, int ry0, int rx1, int ry1, int margin,
                                                                  uint32_t gain, uint64_t *__restrict__ dist) {
    const int jid = blockIdx.x;
    if (jid >= njobs) return;
    const int lane = threadIdx.x;
    const BlockJob J = jobs[jid];
    const int nb = min((int)numbps[jid], RATE_STRIDE - 1);
    uint64_t mine = 0;
    if (nb > 0) {
        mine = rate_distortion_of(nb, J, coef + J.src_off, lane);
        if (gain > 1) {
            const j2k_block b = blocks[jid];
            const RoiWin F = roi_window(b, planes[b.plane], rx0, ry0, rx1, ry1, margin);
            if (F.w == J.w && F.h == J.h) mine *= (uint64_t)gain;            // the whole block: gain * D
            else if (F.w > 0) {
                BlockJob S = J;
                S.src_off = J.src_off + (int64_t)F.y * J.stride + F.x;
                S.w = F.w; S.h = F.h;
                mine += (uint64_t)(gain - 1) * rate_distortion_of(nb, S, coef + S.src_off, lane);
            }
        }
    }
    if (lane < RATE_STRIDE) dist[(size_t)jid * RATE_STRIDE + (lane <= nb ? nb - lane : lane)] = lane <= nb ? mine : 0;
}

// ---- allocation: one workgroup for a frame ------------------------------------------------------------------------------------------------
// A launch has F = gridDim.x workgroups; workgroup f allocates frame f of a batch plan (j2k_plan_set_rate_per_frame, tests/frame_rate_cases.py):
// the contiguous jobs frames[f], under that frame's own budget(s) or target(s).  Every other launch has ONE workgroup and frames == NULL: the
// frame is all njobs jobs.  Inside a workgroup every index is frame-LOCAL -- the table pointers are moved to the frame's first job, thread t
// owns the blocks t, t + 1024, ... of ITS frame -- so the float64 sums add in the order the definition fixes for that frame alone and the
// results are the bits a single-frame plan gives.  Workgroups share nothing: each has its own slice of the hull workspace (sliced by job
// index), writes kept[l * njobs + j] for its own jobs j and chosen / achieved [l * F + f]; a frame whose full lengths fit returns early while
// its neighbours search.
// Workspace per block: the planes of its hull points (32 bytes), their incoming slopes (32 doubles), the count.
#define RATE_WG 1024
// ST: the table stride -- RATE_STRIDE with a point per bit plane (points = numBPS), RATE_PASS_STRIDE with a point per coding pass
// (points = 3 numBPS - 2; tests/pass_cases.py).  The workspace is sized for the larger.
struct RateWs {
    double *slope;      // [n][ST]
    uint8_t *plane;     // [n][ST]
    uint32_t *count;    // [n]
};
template <int ST = RATE_STRIDE>
__host__ __device__ inline RateWs rate_ws(void *ws, size_t n) {
    RateWs W;
    W.slope = reinterpret_cast<double *>(ws);
    W.count = reinterpret_cast<uint32_t *>(W.slope + n * ST);
    W.plane = reinterpret_cast<uint8_t *>(W.count + n);
    return W;
}
size_t rate_allocate_workspace(int njobs) { return (size_t)njobs * (RATE_PASS_STRIDE * 9 + 4) + 256; }
// workgroup blockIdx.x's frame: its first job and its job count (wave-uniform)
__device__ __forceinline__ RateFrame rate_frame(const RateFrame *__restrict__ frames, int njobs) {
    return frames ? frames[blockIdx.x] : RateFrame{0, njobs};
}
// the workspace of all njobs jobs -> the slice of the frame that starts at job `first`
template <int ST>
__device__ __forceinline__ RateWs rate_ws_frame(void *ws, int njobs, int first) {
    RateWs W = rate_ws<ST>(ws, (size_t)njobs);
    W.slope += (size_t)first * ST;
    W.plane += (size_t)first * ST;
    W.count += first;
    return W;
}
// the last point of a block's table
template <int ST>
__device__ __forceinline__ int rate_points(const uint8_t *__restrict__ numbps, int j) {
    const int nb = min((int)numbps[j], RATE_STRIDE - 1);
    return ST == RATE_STRIDE ? nb : max(3 * nb - 2, 0);
}

// sum over the workgroup, the same value in every thread (integer sums: the order does not matter)
__device__ __forceinline__ uint64_t wg_sum(uint64_t v, uint64_t *sh) {
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
    __syncthreads();                                     // the previous sum has been read
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t t = 0;
    for (int i = 0; i < RATE_WG / 64; i++) t += sh[i];
    return t;
}

// hulls: the upper-left convex hull of (rate, distortion) from p = 0, pop while the new point is not less steep (every thread its own blocks)
template <int ST = RATE_STRIDE>
__device__ __forceinline__ void rate_hulls(int njobs, const uint32_t *__restrict__ rate, const uint64_t *__restrict__ dist, const uint8_t *__restrict__ numbps,
                                           const double *__restrict__ weights, const RateWs &W) {
    for (int j = threadIdx.x; j < njobs; j += RATE_WG) {
        const uint32_t *R = rate + (size_t)j * ST;
        const uint64_t *D = dist + (size_t)j * ST;
        double *sl = W.slope + (size_t)j * ST;
        uint8_t *pt = W.plane + (size_t)j * ST;
        const int nb = rate_points<ST>(numbps, j);
        const double w = weights[j];
        int cnt = 1;
        pt[0] = 0; sl[0] = 0.0;
        for (int p = 1; p <= nb; p++) {
            const uint32_t Rp = R[p];
            const uint64_t Dp = D[p];
            for (;;) {
                const int a = pt[cnt - 1];
                if (!(Dp < D[a])) break;                                 // no less distortion: never a hull point
                const bool free_ = Rp <= R[a];
                double s = __builtin_huge_val();
                if (!free_) {
                    const double num = w * (double)(D[a] - Dp);          // one multiply, one divide (-ffp-contract=off; nothing to fuse anyway)
                    s = num / (double)(Rp - R[a]);
                }
                if (cnt > 1) {
                    if (s >= sl[cnt - 1]) { cnt--; continue; }
                    pt[cnt] = (uint8_t)p; sl[cnt] = s; cnt++;
                } else if (free_) {
                    pt[0] = (uint8_t)p;                                  // less distortion for no more bytes: the new start
                } else {
                    pt[cnt] = (uint8_t)p; sl[cnt] = s; cnt++;
                }
                break;
            }
        }
        W.count[j] = (uint32_t)cnt;
    }
}
template <int ST = RATE_STRIDE>
__device__ __forceinline__ int rate_pick(const RateWs &W, int j, double lam) {
    const double *sl = W.slope + (size_t)j * ST;
    const int cnt = (int)W.count[j];
    int i = 0;
    while (i + 1 < cnt && sl[i + 1] >= lam) i++;
    return W.plane[(size_t)j * ST + i];
}
// The smallest bit pattern of a non-negative double whose choice fits: bisection over the patterns, 64 steps (the patterns above
// +infinity are NaNs: no slope is >= a NaN, every block is at its start point, whose rate is 0 -- the top of the range always fits).
// Writes that choice to kept[0 ... njobs) and returns its bytes.  (Each thread reads back only the hulls it built itself: no barrier
// needed between rate_hulls and the search.)
template <int ST = RATE_STRIDE>
__device__ __forceinline__ uint64_t rate_search(int njobs, const uint32_t *__restrict__ rate, const RateWs &W, uint64_t budget, uint64_t *sh,
                                                uint8_t *__restrict__ kept) {
    const int tid = threadIdx.x;
    uint64_t lo = 0, hi = 0x7FFFFFFFFFFFFFFFull;
    for (int step = 0; step < 64; step++) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const double lam = __longlong_as_double((long long)mid);
        uint64_t b = 0;
        for (int j = tid; j < njobs; j += RATE_WG) b += rate[(size_t)j * ST + rate_pick<ST>(W, j, lam)];
        b = wg_sum(b, sh);                               // every thread takes every step: wg_sum has barriers
        if (lo < hi) { if (b <= budget) hi = mid; else lo = mid + 1; }
    }
    const double lam = __longlong_as_double((long long)hi);
    uint64_t b = 0;
    for (int j = tid; j < njobs; j += RATE_WG) {
        const int p = rate_pick<ST>(W, j, lam);
        kept[j] = (uint8_t)p;
        b += rate[(size_t)j * ST + p];
    }
    return wg_sum(b, sh);
}

template <int ST = RATE_STRIDE>
__global__ __launch_bounds__(RATE_WG) void rate_allocate_kernel(int njobs, const uint32_t *__restrict__ rate, const uint64_t *__restrict__ dist,
                                                                const uint8_t *__restrict__ numbps, const double *__restrict__ weights, uint64_t budget,
                                                                void *__restrict__ ws, uint8_t *__restrict__ kept, uint64_t *__restrict__ chosen,
                                                                const RateFrame *__restrict__ frames, const uint64_t *__restrict__ frame_budgets) {
    __shared__ uint64_t sh[RATE_WG / 64];
    const int tid = threadIdx.x;
    const RateFrame fr = rate_frame(frames, njobs);
    const RateWs W = rate_ws_frame<ST>(ws, njobs, fr.first);
    if (frame_budgets) budget = frame_budgets[blockIdx.x];                   // (the _frames calls: a budget per frame)
    rate += (size_t)fr.first * ST; dist += (size_t)fr.first * ST; numbps += fr.first; weights += fr.first; kept += fr.first;
    chosen += blockIdx.x;
    njobs = fr.count;
    // nothing to cut?
    uint64_t part = 0;
    for (int j = tid; j < njobs; j += RATE_WG) part += rate[(size_t)j * ST + rate_points<ST>(numbps, j)];
    const uint64_t total = wg_sum(part, sh);
    if (total <= budget) {
        for (int j = tid; j < njobs; j += RATE_WG) kept[j] = (uint8_t)rate_points<ST>(numbps, j);
        if (tid == 0) *chosen = total;
        return;
    }
    rate_hulls<ST>(njobs, rate, dist, numbps, weights, W);
    const uint64_t b = rate_search<ST>(njobs, rate, W, budget, sh, kept);
    if (tid == 0) *chosen = b;
}

struct RateBudgets { uint64_t b[32]; };
// The same for nlayers cumulative budgets in one launch (quality layers): layer l is rate_allocate_kernel's result for budgets[l],
// kept[l * njobs + j] and chosen[l].  The hulls are built once (and not at all when every budget holds the full lengths); each layer that cuts
// runs its own 64-step bisection over them.  "The smallest lambda that fits" makes kept monotone in the budget.
__global__ __launch_bounds__(RATE_WG) void rate_allocate_layers_kernel(int njobs, const uint32_t *__restrict__ rate, const uint64_t *__restrict__ dist,
                                                                       const uint8_t *__restrict__ numbps, const double *__restrict__ weights,
                                                                       const RateBudgets budgets, int nlayers, void *__restrict__ ws,
                                                                       uint8_t *__restrict__ kept, uint64_t *__restrict__ chosen,
                                                                       const RateFrame *__restrict__ frames) {
    __shared__ uint64_t sh[RATE_WG / 64];
    const int tid = threadIdx.x;
    const RateFrame fr = rate_frame(frames, njobs);
    const RateWs W = rate_ws_frame<RATE_STRIDE>(ws, njobs, fr.first);
    const size_t nall = (size_t)njobs, nfr = gridDim.x;  // kept [l][all jobs], chosen [l][frames]
    rate += (size_t)fr.first * RATE_STRIDE; dist += (size_t)fr.first * RATE_STRIDE; numbps += fr.first; weights += fr.first; kept += fr.first;
    chosen += blockIdx.x;
    njobs = fr.count;
    uint64_t part = 0;
    for (int j = tid; j < njobs; j += RATE_WG) part += rate[(size_t)j * RATE_STRIDE + min((int)numbps[j], RATE_STRIDE - 1)];
    const uint64_t total = wg_sum(part, sh);
    bool have_hulls = false;                             // (uniform over the workgroup: budgets and total are)
    for (int l = 0; l < nlayers; l++) {
        const uint64_t budget = budgets.b[l];
        uint8_t *kl = kept + (size_t)l * nall;
        if (total <= budget) {
            for (int j = tid; j < njobs; j += RATE_WG) kl[j] = (uint8_t)min((int)numbps[j], RATE_STRIDE - 1);
            if (tid == 0) chosen[(size_t)l * nfr] = total;
            continue;
        }
        if (!have_hulls) { rate_hulls(njobs, rate, dist, numbps, weights, W); have_hulls = true; }
        const uint64_t b = rate_search(njobs, rate, W, budget, sh, kl);
        if (tid == 0) chosen[(size_t)l * nfr] = b;
    }
}

// ---- the dual: the fewest bytes whose weighted distortion stays within a target (tests/quality_cases.py is the definition) ------------------
// The sum of float64 terms over the workgroup in the definition's FIXED order: `v` is the thread's own sum (its terms in order, from 0.0),
// then six butterfly steps inside the wavefront, then the 16 wavefront values in order from 0.0.  The same value in every thread.
__device__ __forceinline__ double wg_sum_f64(double v, double *sh) {
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    __syncthreads();                                     // the previous sum has been read
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < RATE_WG / 64; i++) t = t + sh[i];
    return t;
}
// The LARGEST bit pattern of a non-negative double whose choice has S <= target: bisection over the patterns, 64 steps, the midpoint rounded
// up.  Pattern 0 always fits (lambda = +0.0 takes every hull to its last point, where D = 0), so `lo` is a fitting pattern throughout.
// Writes that choice to kept[0 ... njobs), its bytes to *bytes (every thread), and returns its S.
template <int ST = RATE_STRIDE>
__device__ __forceinline__ double quality_search(int njobs, const uint32_t *__restrict__ rate, const uint64_t *__restrict__ dist, const double *__restrict__ weights,
                                                 const RateWs &W, double target, uint64_t *sh, double *shf, uint8_t *__restrict__ kept, uint64_t *bytes) {
    const int tid = threadIdx.x;
    uint64_t lo = 0, hi = 0x7FFFFFFFFFFFFFFFull;
    for (int step = 0; step < 64; step++) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        const double lam = __longlong_as_double((long long)mid);
        double s = 0.0;
        for (int j = tid; j < njobs; j += RATE_WG) s = s + weights[j] * (double)dist[(size_t)j * ST + rate_pick<ST>(W, j, lam)];
        s = wg_sum_f64(s, shf);                          // every thread takes every step: wg_sum_f64 has barriers
        if (s <= target) lo = mid; else hi = mid - 1;
    }
    const double lam = __longlong_as_double((long long)lo);
    uint64_t b = 0;
    double s = 0.0;
    for (int j = tid; j < njobs; j += RATE_WG) {
        const int p = rate_pick<ST>(W, j, lam);
        kept[j] = (uint8_t)p;
        b += rate[(size_t)j * ST + p];
        s = s + weights[j] * (double)dist[(size_t)j * ST + p];
    }
    *bytes = wg_sum(b, sh);
    return wg_sum_f64(s, shf);
}

struct RateTargets { double t[32]; };
// the one-target form on the pass tables (j2k_plan_rate_allocate_quality_passes): the same search, a point per coding pass
__global__ __launch_bounds__(RATE_WG) void rate_allocate_quality_passes_kernel(int njobs, const uint32_t *__restrict__ rate, const uint64_t *__restrict__ dist,
                                                                               const uint8_t *__restrict__ numbps, const double *__restrict__ weights,
                                                                               double target, void *__restrict__ ws, uint8_t *__restrict__ kept,
                                                                               uint64_t *__restrict__ chosen, double *__restrict__ achieved,
                                                                               const RateFrame *__restrict__ frames, const double *__restrict__ frame_targets) {
    __shared__ uint64_t sh[RATE_WG / 64];
    __shared__ double shf[RATE_WG / 64];
    const RateFrame fr = rate_frame(frames, njobs);
    const RateWs W = rate_ws_frame<RATE_PASS_STRIDE>(ws, njobs, fr.first);
    if (frame_targets) target = frame_targets[blockIdx.x];                   // (the _frames calls: a target per frame)
    rate += (size_t)fr.first * RATE_PASS_STRIDE; dist += (size_t)fr.first * RATE_PASS_STRIDE; numbps += fr.first; weights += fr.first; kept += fr.first;
    njobs = fr.count;
    rate_hulls<RATE_PASS_STRIDE>(njobs, rate, dist, numbps, weights, W);
    uint64_t b = 0;
    const double s = quality_search<RATE_PASS_STRIDE>(njobs, rate, dist, weights, W, target, sh, shf, kept, &b);
    if (threadIdx.x == 0) { chosen[blockIdx.x] = b; achieved[blockIdx.x] = s; }
}

// One workgroup, a sibling of rate_allocate_layers_kernel: layer l is the search for targets.t[l] -- kept[l * njobs + j], chosen[l] (body bytes),
// achieved[l] (S).  The hulls are built once.  Targets fall with l, "the largest lambda that fits" then makes kept monotone in l.
__global__ __launch_bounds__(RATE_WG) void rate_allocate_quality_kernel(int njobs, const uint32_t *__restrict__ rate, const uint64_t *__restrict__ dist,
                                                                        const uint8_t *__restrict__ numbps, const double *__restrict__ weights,
                                                                        const RateTargets targets, int nlayers, void *__restrict__ ws,
                                                                        uint8_t *__restrict__ kept, uint64_t *__restrict__ chosen, double *__restrict__ achieved,
                                                                        const RateFrame *__restrict__ frames, const double *__restrict__ frame_targets) {
    __shared__ uint64_t sh[RATE_WG / 64];
    __shared__ double shf[RATE_WG / 64];
    const RateFrame fr = rate_frame(frames, njobs);
    const RateWs W = rate_ws_frame<RATE_STRIDE>(ws, njobs, fr.first);
    const size_t nall = (size_t)njobs, nfr = gridDim.x;  // kept [l][all jobs], chosen / achieved [l][frames]
    rate += (size_t)fr.first * RATE_STRIDE; dist += (size_t)fr.first * RATE_STRIDE; numbps += fr.first; weights += fr.first; kept += fr.first;
    chosen += blockIdx.x; achieved += blockIdx.x;
    njobs = fr.count;
    rate_hulls(njobs, rate, dist, numbps, weights, W);
    for (int l = 0; l < nlayers; l++) {
        uint64_t b = 0;
        const double target = frame_targets ? frame_targets[blockIdx.x] : targets.t[l];      // (the _frames calls: one layer, a target per frame)
        const double s = quality_search(njobs, rate, dist, weights, W, target, sh, shf, kept + (size_t)l * nall, &b);
        if (threadIdx.x == 0) { chosen[(size_t)l * nfr] = b; achieved[(size_t)l * nfr] = s; }
    }
}

// One value per frame of a batch (the _frames calls) into the plan's table: the values travel BY VALUE, so a captured call replays with the
// values it was captured with and the host array may go as soon as the call returns; RATE_FRAME_CHUNK of them per launch, any number of frames.
#define RATE_FRAME_CHUNK 128
struct RateFrameValues { uint64_t v[RATE_FRAME_CHUNK]; };
__global__ __launch_bounds__(RATE_FRAME_CHUNK) void rate_frame_values_kernel(const RateFrameValues vals, int count, uint64_t *__restrict__ table) {
    if ((int)threadIdx.x < count) table[threadIdx.x] = vals.v[threadIdx.x];
}
// values: nframes 64-bit patterns on the host (budgets, or the bits of float64 targets); table: nframes words on the device
hipError_t launch_rate_frame_values(hipStream_t s, const uint64_t *values, int nframes, uint64_t *table) {
    for (int at = 0; at < nframes; at += RATE_FRAME_CHUNK) {
        RateFrameValues V{};
        const int count = std::min(RATE_FRAME_CHUNK, nframes - at);
        for (int i = 0; i < count; i++) V.v[i] = values[at + i];
        hipLaunchKernelGGL(rate_frame_values_kernel, dim3(1), dim3(RATE_FRAME_CHUNK), 0, s, V, count, table + at);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// targets: nlayers <= 32 values on the host (a kernel argument); kept: nlayers x njobs bytes; chosen: nlayers x nframes uint64; achieved: nlayers x
// nframes double.  frames (device, or null with nframes = 1): the job range of every frame; frame_targets (device, or null): nlayers = 1, frame
// f's target in the place of targets[0]
hipError_t launch_rate_allocate_quality(hipStream_t s, int njobs, const uint32_t *rate, const uint64_t *dist, const uint8_t *numbps, const double *weights,
                                        const double *targets, int nlayers, void *ws, uint8_t *kept, uint64_t *chosen, double *achieved, int nframes,
                                        const RateFrame *frames, const double *frame_targets) {
    RateTargets T{};
    for (int l = 0; l < nlayers && l < 32; l++) T.t[l] = targets ? targets[l] : 0.0;
    hipLaunchKernelGGL(rate_allocate_quality_kernel, dim3(frames ? nframes : 1), dim3(RATE_WG), 0, s, njobs, rate, dist, numbps, weights, T, std::min(nlayers, 32), ws, kept,
                       chosen, achieved, frames, frame_targets);
    return hipGetLastError();
}

hipError_t launch_rate_distortion(hipStream_t s, const BlockJob *jobs, int njobs, const int32_t *coef, const uint8_t *numbps, uint64_t *dist) {
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(rate_distortion_kernel, dim3(njobs), dim3(64), 0, s, jobs, njobs, coef, numbps, dist);
    return hipGetLastError();
}

hipError_t launch_rate_distortion_roi(hipStream_t s, const BlockJob *jobs, int njobs, const int32_t *coef, const uint8_t *numbps, const j2k_block *blocks,
                                      const AreaPlane *planes, int x0, int y0, int x1, int y1, int margin, uint32_t gain, uint64_t *dist) {
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(rate_distortion_roi_kernel, dim3(njobs), dim3(64), 0, s, jobs, njobs, coef, numbps, blocks, planes, x0, y0, x1, y1, margin, gain, dist);
    return hipGetLastError();
}

// frames (device, or null with nframes = 1): the job range of every frame of a batch, one workgroup each, chosen: nframes words; frame_budgets
// (device, or null): frame f's budget in the place of `budget`
hipError_t launch_rate_allocate(hipStream_t s, int njobs, const uint32_t *rate,const uint64_t *dist, const uint8_t *numbps, const double *weights,
                                uint64_t budget, void *ws, uint8_t *kept, uint64_t *chosen, int nframes, const RateFrame *frames, const uint64_t *frame_budgets) {
    hipLaunchKernelGGL(rate_allocate_kernel<RATE_STRIDE>, dim3(frames ? nframes : 1), dim3(RATE_WG), 0, s, njobs, rate, dist, numbps, weights, budget, ws, kept, chosen,
                       frames, frame_budgets);
    return hipGetLastError();
}

// ---- pass cuts: tables of 96 entries per block, kept[j] = a pass index ----
hipError_t launch_rate_distortion_passes(hipStream_t s, const BlockJob *jobs, int njobs, const int32_t *coef, const uint8_t *numbps, const uint64_t *spmask,
                                         uint64_t *dist) {
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(rate_distortion_passes_kernel, dim3(njobs), dim3(64), 0, s, jobs, njobs, coef, numbps, spmask, dist);
    return hipGetLastError();
}
hipError_t launch_rate_allocate_passes(hipStream_t s, int njobs, const uint32_t *rate, const uint64_t *dist, const uint8_t *numbps, const double *weights,
                                       uint64_t budget, void *ws, uint8_t *kept, uint64_t *chosen, int nframes, const RateFrame *frames,
                                       const uint64_t *frame_budgets) {
    hipLaunchKernelGGL(rate_allocate_kernel<RATE_PASS_STRIDE>, dim3(frames ? nframes : 1), dim3(RATE_WG), 0, s, njobs, rate, dist, numbps, weights, budget, ws, kept, chosen,
                       frames, frame_budgets);
    return hipGetLastError();
}
hipError_t launch_rate_allocate_quality_passes(hipStream_t s, int njobs, const uint32_t *rate, const uint64_t *dist, const uint8_t *numbps, const double *weights,
                                               double target, void *ws, uint8_t *kept, uint64_t *chosen, double *achieved, int nframes,
                                               const RateFrame *frames, const double *frame_targets) {
    hipLaunchKernelGGL(rate_allocate_quality_passes_kernel, dim3(frames ? nframes : 1), dim3(RATE_WG), 0, s, njobs, rate, dist, numbps, weights, target, ws, kept, chosen,
                       achieved, frames, frame_targets);
    return hipGetLastError();
}

// budgets: nlayers <= 32 values on the host (a kernel argument); kept: nlayers x njobs bytes; chosen: nlayers x nframes uint64
hipError_t launch_rate_allocate_layers(hipStream_t s, int njobs, const uint32_t *rate, const uint64_t *dist, const uint8_t *numbps, const double *weights,
                                       const uint64_t *budgets, int nlayers, void *ws, uint8_t *kept, uint64_t *chosen, int nframes, const RateFrame *frames) {
    RateBudgets B{};
    for (int l = 0; l < nlayers && l < 32; l++) B.b[l] = budgets[l];
    hipLaunchKernelGGL(rate_allocate_layers_kernel, dim3(frames ? nframes : 1), dim3(RATE_WG), 0, s, njobs, rate, dist, numbps, weights, B, nlayers, ws, kept, chosen, frames);
    return hipGetLastError();
}

}  // namespace j2k
