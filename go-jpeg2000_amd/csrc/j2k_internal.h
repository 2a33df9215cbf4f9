// j2k_internal.h -- shared between the HIP kernels and the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include "../../include/j2kgfx.h"
#include "image_color.h"
#include "j2k_tables.h"

namespace j2k {

// launch wrappers (dwt53.hip, dwt97.hip, mct.hip, ht.hip, t1.hip)
// A YCbCr image read by the 5-3 level-0 workgroup kernel itself (j2k_plan_forward_image): the planes at the frame's origin
// (Rect.Min even and >= 0), one chroma stride for Cb and Cr (Go's CStride); ratio J2K_YCBCR_444 / 422 / 420.
struct YccSrc {
    const uint8_t *y, *cb, *cr;
    int64_t ystride, cstride;
    int32_t ratio, pad_;
};

struct LevelLaunch {
    const DwtJob *jobs;   // device
    int njobs;
    const DwtPlane *planes;  // device
    int cpl;              // columns per lane: 2, 4 or 8
    int vec;              // 1: every plane satisfies the vector-access alignment rules
    int ncomp;            // 1 or 3 (3 = fused colour transform on level 0)
    int pf;               // forward 5-3: software-prefetch variant
    int pix_stride;       // level 0: > 0 = the frame is packed pixels with this row stride in PIXELS (RGBA8 for a triple unless pix_src says otherwise)
    int pix_src;          // ... which pixels (dwt53_plane_wg.inc SRC / DST: 1 Gray16, 2 Gray8, 3 a byte of a four-byte pixel, 4 a 16-bit sample of an eight-byte pixel)
    long long comp_elems; // ... W * H of the frame (plane offsets are component * W * H + y0 * W + x0)
    int wg_waves;         // > 0: `jobs` is the per-WORKGROUP table of dwt53_fwd_rgba8_wg_kernel (dwt53_l0pix.inc): wg_waves
                          // wavefronts per workgroup, wg_waves - 1 pair-rows each; level 0 of an RGBA8 frame only
    int wg_store;         // its final-coefficient store flavour (0 plain, 1 nt, ...)
    // levels 0 + 1 in one launch (dwt53_fwd_rgba8_wg2_kernel): jobs2 = the bands of the top half of every plane (wg2_waves waves
    // each), planes1 = the level-1 plane table (three per level-0 plane), nxt1 = the scratch that feeds level 2; `jobs` then
    // holds only the remaining bands
    const DwtJob *jobs2;
    int njobs2, wg2_waves;
    const DwtPlane *planes1;
    int32_t *nxt1;
    const DwtJob *pjobs;  // single-component planes in workgroup form (dwt53_plane_wg.inc): per-workgroup table, pwaves waves each
    int pnjobs, pwaves, pmulti;
    hipEvent_t ev_start, ev_stop;   // non-null: the dispatch itself stamps these (hipExtLaunchKernelGGL) -- the kernel's own
                                    // begin / end, without the launch gap an event pair around the launch would include
    YccSrc ycc;           // ycc.y non-null: level 0 of the workgroup form reads this YCbCr image instead of packed RGBA8
    const int *guard;     // inverse: non-null = a device word; the launch writes nothing if it is not 0 (the frame decoder's status, j2k_frame.cpp)
    int mallat;           // 1: a level of a Mallat plan (DwtPlane::coef_stride): the MAL instantiation of the general kernels
    const uint8_t *scr16_fmt;   // inverse, non-null: the workgroup form of the packed RGBA8 level 0 reads the half-rows of X_1 as int16 where this table says so
                                // (dwt53_inv_rgba8_wg16_kernel behind dwt53_deep_inv16_kernel; j2k_plan::d_scr16_fmt)
    int scr16;            // 1: the workgroup form of the packed RGBA8 level 0 stores the rows of X_1 as int16 (dwt53_fwd_rgba8_wg16_kernel; j2k_plan::scr16_fwd)
};

hipError_t launch_dwt53_fwd(hipStream_t s, const LevelLaunch &L, const int32_t *src, int32_t *out,
                            int32_t *nxt, int dc_shift);
hipError_t launch_dwt53_inv(hipStream_t s, const LevelLaunch &L, const int32_t *coef, const int32_t *prev,
                            int32_t *dst, int dc_shift, int final_level);
hipError_t launch_dwt53_tail_fwd(hipStream_t s, const TailPlane *planes, int nplanes, size_t lds_bytes, const int32_t *scr,
                                 int32_t *coef, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t launch_dwt53_tail_inv(hipStream_t s, const TailPlane *planes, int nplanes, size_t lds_bytes, const int32_t *coef,
                                 int32_t *scr, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// every level below level 0 in one launch (dwt53_deep.inc); ev0 / ev1: optional begin / end events stamped by the dispatch
// scr16: the rows of `scr` are int16 in the first half of their slots (the level-0 launch was dwt53_fwd_rgba8_wg16_kernel)
hipError_t launch_dwt53_deep_fwd(hipStream_t s, const DwtJob *jobs, int njobs, const TailPlane *planes, size_t lds_bytes, const int32_t *scr,
                                 int32_t *coef, hipEvent_t ev0, hipEvent_t ev1, int scr16 = 0);
hipError_t launch_dwt53_deep_inv(hipStream_t s, const DwtJob *jobs, int njobs, const TailPlane *planes, size_t lds_bytes, const int32_t *coef,
                                 int32_t *scr, hipEvent_t ev0, hipEvent_t ev1, uint8_t *scr16_fmt = nullptr);   // scr16_fmt: dwt53_deep_inv16_kernel and its format table

hipError_t launch_dwt53_mega_fwd(hipStream_t s, const DwtJob *jobs, int njobs, const TailPlane *tplanes, const DwtPlane *l0planes, size_t lds_bytes,
                                 const int32_t *scr, int32_t *coef, const uint32_t *pix, int32_t *nxt0, int dc_shift, int pix_stride,
                                 hipEvent_t ev0, hipEvent_t ev1);
hipError_t launch_dwt53_mega_inv(hipStream_t s, const DwtJob *jobs, int njobs, const TailPlane *tplanes, const DwtPlane *l0planes, size_t lds_bytes,
                                 const int32_t *coef, int32_t *scr, const int32_t *prev0, uint32_t *pix, int dc_shift, int pix_stride,
                                 hipEvent_t ev0, hipEvent_t ev1);
hipError_t launch_unpack_pixels(hipStream_t s, const uint8_t *pix, size_t stride, int format, int w, int h, int src_max, int dst_max,
                                int32_t *planes);
hipError_t launch_colorspace(hipStream_t s, int cs, int32_t *planes, int ncomp, size_t n, int precision);
hipError_t launch_pack_pixels(hipStream_t s, const int32_t *planes, int ncomp, int precision, int w, int h, uint8_t *pix, size_t stride);
hipError_t launch_pack_pixels_rect(hipStream_t s, const int32_t *planes, int ncomp, int precision, int w, int h, int x0, int y0, int rw, int rh, uint8_t *pix,
                                   size_t stride, const int *guard = nullptr);   // the rectangle (x0, y0, rw, rh) of the frame only
// ... written to pix at origin (0, 0): pix holds rh rows of rw pixels (region decode)
hipError_t launch_pack_pixels_window(hipStream_t s, const int32_t *planes, int ncomp, int precision, int w, int h, int x0, int y0, int rw, int rh, uint8_t *pix,
                                     size_t stride, const int *guard);
// region decode (area.hip): the need set of a rectangle; the table entries of the blocks outside it emptied
hipError_t launch_area_blocks(hipStream_t s, const j2k_block *blocks, int n, const AreaPlane *planes, int x0, int y0, int x1, int y1, int reduce, int margin,
                              uint8_t *need, uint32_t *lens, uint8_t *numbps, uint8_t *floors);
// image.YCbCr / CMYK / Paletted -> packed RGBA8 (image.hip); *flag = J2K_ERR_GO_PANIC for a palette index >= npal
hipError_t launch_image_to_rgba8(hipStream_t s, const j2k_image &img, uint32_t *pix, size_t stride_px, int *flag);

// Tier-2 packets on device buffers (t2dev.hip)
hipError_t launch_t2_fill_cbs(hipStream_t s, long n, const uint64_t *offs, const uint32_t *lens, const uint8_t *numbps, int mb, int ht, j2k_t2_dev_cb *cbs, uint64_t *reset = nullptr,
                              const uint8_t *kept = nullptr, const uint32_t *rate = nullptr,    // kept + rate: blocks cut at bit planes (rate control)
                              int passes = 0);                                                  // passes: kept counts coding passes, rate has 96 entries per block
hipError_t launch_t2_encode_tile_parts(hipStream_t s, const j2k_t2_dev_packet *packets, long npackets, const j2k_t2_dev_cb *cbs, uint64_t ncbs, const uint8_t *data,
                                       int sop, int eph, uint8_t *out, uint64_t cap, uint64_t *offs, void *ws, uint64_t *result, const int32_t *ptile,
                                       const int *tile_packet0, int ntiles, int tile_first, uint64_t *tile_offs, int *status, const BlockJob *slot_jobs,
                                       const uint32_t *maglens, int ht, int body_slices);
size_t t2_dev_workspace(long npackets);
hipError_t launch_t2_encode_packets(hipStream_t s, const j2k_t2_dev_packet *packets, long npackets, const j2k_t2_dev_cb *cbs, uint64_t ncbs, const uint8_t *data,
                                    int sop, int eph, int delay_in, uint8_t *out, uint64_t cap, uint64_t *offs, void *ws, uint64_t *result);

// n bytes src -> dst, any alignment on both sides, one wavefront: bytes up to the destination's next 16-byte boundary,
// then aligned 16-byte stores of (possibly unaligned) 16-byte loads, then the tail bytes
__device__ __forceinline__ void copy_bytes(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t n, int lane) {
    const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
    if ((uint32_t)lane < head) dst[lane] = src[lane];
    const uint32_t nv = (n - head) >> 4;
    for (uint32_t i = lane; i < nv; i += 64) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16 * (size_t)i, 16);
        *reinterpret_cast<uint4 *>(dst + head + 16 * (size_t)i) = v;
    }
    const uint32_t done = head + (nv << 4);
    if (done + lane < n) dst[done + lane] = src[done + lane];
}
__device__ __forceinline__ void zero_run(uint8_t *__restrict__ dst, uint32_t n, int lane) {
    const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
    if ((uint32_t)lane < head) dst[lane] = 0;
    const uint32_t nv = (n - head) >> 4;
    for (uint32_t i = lane; i < nv; i += 64) *reinterpret_cast<uint4 *>(dst + head + 16 * (size_t)i) = make_uint4(0, 0, 0, 0);
    const uint32_t done = head + (nv << 4);
    if (done + lane < n) dst[done + lane] = 0;
}

// one wavefront per job.  maglens != NULL (HT blocks coded by j2k_plan_encode_stream): the slot holds
// MagSgn | <hole> | VLC | SCUP -- the MEL segment of max(64, 2wh)/4 zero bytes (ht.go:978, 1019) was never written to the
// slot and is produced here as zeros, so two thirds of a 64x64 block's bytes are neither stored twice nor read back.
__device__ __forceinline__ void gather_job(const BlockJob &J, const uint8_t *__restrict__ slots, uint8_t *__restrict__ dst, uint32_t len,
                                           bool ht, uint32_t mag, int lane) {
    const uint8_t *src = slots + J.out_off;
    if (!ht) {
        copy_bytes(dst, src, len, lane);
        return;
    }
    const size_t nsamp = (size_t)J.w * J.h;
    const uint32_t mel = (uint32_t)((nsamp * 2 < 64 ? 64 : nsamp * 2) / 4);
    copy_bytes(dst, src, mag, lane);
    zero_run(dst + mag, mel, lane);
    copy_bytes(dst + mag + mel, src + mag + mel, len - mag - mel, lane);
}

// an environment variable of the tuning set: read only when J2K_TUNING=1 (see j2k_ctx_create)
inline const char *tuning_env(const char *name) {
    static const int on = [] { const char *t = getenv("J2K_TUNING"); return (t && t[0] == '1' && !t[1]) ? 1 : 0; }();
    return on ? getenv(name) : nullptr;
}

// DEV BUILDS ONLY (make CXXFLAGS+=-DJ2K_DEV; env J2K_DEV_SKIP = bit mask): launches left out to measure what each kernel
// costs with several frames in flight (`J2K_DEV_SKIP=<mask> bash tools/ab.sh ...` on a -DJ2K_DEV build).  Results are wrong with any bit set, so the shipped library
// does not have the switch at all: g_dev_skip is the constant 0 and every test of it folds away.
#ifdef J2K_DEV
extern int g_dev_skip, g_dev_dup;      // J2K_DEV_DUP: the same bits, launches issued TWICE (every one is idempotent: results stay valid)
inline int dev_reps(int bit) { return (g_dev_skip & bit) ? 0 : ((g_dev_dup & bit) ? 2 : 1); }
#else
constexpr int g_dev_skip = 0;
constexpr int dev_reps(int) { return 1; }
#endif
}  // namespace j2k
