// j2k_tables.h -- the device job tables' entries: shared between the HIP kernels (through j2k_internal.h) and the plan's table builder
// (plan_tables.h), which runs without HIP.  Nothing of HIP in here; the layouts are the kernels' and are pinned below.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace j2k {

// One tile-component (or RCT/ICT group of three) at one decomposition level.
// All offsets are in ELEMENTS relative to the base pointer the launch passes.
struct DwtPlane {
    int64_t src_off[3];   // level input: comp k at src + src_off[k], row stride src_stride
    int64_t out_off[3];   // final coefficient plane of comp k (dense, stride = w of level 0... see n_next)
    int64_t nxt_off[3];   // scratch that receives the prefix [0, n_next) = input of the next level
    int32_t src_stride;
    int32_t w, h;         // dims of this level: dense w x h matrix
    int32_t n_next;       // w_{l+1}*h_{l+1}; linear idx < n_next -> nxt, else -> out (0 on the last level)
    int32_t out_stride;   // inverse level 0 only: row stride of the destination frame
    int32_t coef_stride;  // Mallat plans only (the MAL kernels): row stride of the coefficient plane = w of level 0.  They route on row and
                          // column, not on the linear index: LL (row < h_{l+1}, column < w_{l+1}) <-> nxt as a dense w_{l+1} x h_{l+1}
                          // matrix while n_next != 0, everything else <-> the plane at row * coef_stride + column
};

// One wavefront's work: a column strip x a band of pair-rows of one plane.
struct DwtJob {
    int32_t plane;
    int32_t col0;         // first OWNED input column (multiple of CPL); 0 for the first strip
    int32_t prow0;        // first pair-row of the band
    int32_t nprow;        // pair-rows in the band (low 16 bits) | J2K_LINK_* (forward 5-3 only)
};
// forward 5-3: this band and its neighbour in the same workgroup exchange their halo rows through LDS (dwt53.hip)
#define J2K_LINK_UP 0x10000
#define J2K_LINK_DOWN 0x20000

// One code-block job (device form).
struct BlockJob {
    int64_t src_off;      // element offset of the window origin inside the coefficient buffer
    int64_t out_off;      // byte offset of this job's slot / element offset of its decoded block
    int32_t stride;       // plane width
    int32_t w, h;
    int32_t band;
};

// One distinct block window of the HT encoder (j2k_plan_encode_stream): the job + the jobs that read the same window
struct HtUJob {
    BlockJob J;
    int32_t jid;          // the job that is coded (first of its list)
    int32_t alias_off;    // its list of job ids in the plan's alias_ids table (its own id first)
    int32_t nalias;
    int32_t pad_;
};

// HT decode, byte-identical blocks once (j2k_plan.h d_ht_dec_fol: a count and this many ids per job): jobs that may follow one leader
#define J2K_HT_DEC_MAX_FOLLOWERS 7

// One tile-component for the fused "tail" kernels: decomposition levels l0..l0+nlev-1 run inside LDS.
struct TailPlane {
    int64_t scr_off;      // forward: level-l0 input prefix in scratch; inverse: where X_{l0} is written
    int64_t coef_off;     // final coefficient plane
    int32_t w, h;         // dims at level l0
    int32_t nlev;
    int32_t pad_;
};

// One tile-component (or MCT triple) of a Mallat plan decoded to its coarsest resolution (reduce = levels): no inverse level runs, the LL
// rectangle [0, w) x [0, h) of each coefficient plane is the picture (mct.hip: mallat_ll_kernel)
struct LLPlane {
    int64_t coef_off[3];  // coefficient plane of comp k (row stride coef_stride)
    int64_t out_off[3];   // its place in the reduced int32 frame (row stride out_stride)
    int32_t w, h, coef_stride, out_stride;
    int32_t nc, pad_;     // 1, or 3 = inverse RCT / ICT on the triple
};

// One tile-component for the need set of a region decode (area.hip): its tile's rectangle in the frame and its decomposition levels
struct AreaPlane {
    int32_t x0, y0, w, h;
    int32_t levels;
    int32_t pad_[3];
};

// One frame of a batch plan for the rate allocation (rate.hip, j2k_plan_set_rate_per_frame): its contiguous range of code-block jobs
struct RateFrame {
    int32_t first, count;
};

// |element of X_1| <= J2K_SCR16_BOUND + dc_shift after level 0 of a packed 8-bit frame (derived at st_scr16, dwt53_l0pix.inc)
#define J2K_SCR16_BOUND (4 * 255 + 3)

#define J2K_TABLE_LAYOUT(T, size, last, off) static_assert(sizeof(T) == size && offsetof(T, last) == off, #T ": the kernels read this layout")
J2K_TABLE_LAYOUT(DwtPlane, 96, coef_stride, 92);
J2K_TABLE_LAYOUT(DwtJob, 16, nprow, 12);
J2K_TABLE_LAYOUT(BlockJob, 32, band, 28);
J2K_TABLE_LAYOUT(HtUJob, 48, pad_, 44);
J2K_TABLE_LAYOUT(TailPlane, 32, pad_, 28);
J2K_TABLE_LAYOUT(LLPlane, 72, pad_, 68);
J2K_TABLE_LAYOUT(AreaPlane, 32, pad_, 20);
J2K_TABLE_LAYOUT(RateFrame, 8, count, 4);

}  // namespace j2k
