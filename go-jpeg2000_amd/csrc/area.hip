// area.hip -- region decode (include/j2kgfx.h, j2k_plan_*_area): which code-blocks a rectangle of the frame needs.
//
// The library's own: the reference declares Config.DecodeArea and never reads it.  tests/area_cases.py is the definition this kernel must
// agree with exactly; DESIGN.md 7 has the rule and its margins.  The windows of a Mallat plan partition each plane, and level l's sub-bands
// are the rectangles [w_{l+1}, w_l) x [0, h_{l+1}), [0, w_{l+1}) x [h_{l+1}, h_l) and [w_{l+1}, w_l) x [h_{l+1}, h_l) of it, so the whole
// rule is integer rectangle tests in plane coordinates: at most 3 L + 1 per block.
#include "area_walk.h"

namespace j2k {

// One thread per block job.  need (optional): 1 / 0 per job.  lens / numbps / floors (each optional): the parsed block tables of the frame;
// the entries of a block that is not needed become 0 -- no bytes, no bit planes -- so every MQ decode kernel leaves that block zeros without
// reading its stream.  Blocks of the resolutions `reduce` drops lie outside [0, w_reduce) x [0, h_reduce) and so are never needed.
__global__ __launch_bounds__(256) void area_blocks_kernel(const j2k_block *__restrict__ blocks, int n, const AreaPlane *__restrict__ planes, int ax0, int ay0,
                                                          int ax1, int ay1, int reduce, int margin, uint8_t *__restrict__ need, uint32_t *__restrict__ lens,
                                                          uint8_t *__restrict__ numbps, uint8_t *__restrict__ floors) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const j2k_block b = blocks[j];
    const AreaPlane T = planes[b.plane];
    const bool hit = area_walk(T, ax0, ay0, ax1, ay1, reduce, margin,
                               [&](int x0, int x1, int y0, int y1) { return area_meets(x0, x1, y0, y1, b.x0, b.y0, b.w, b.h); });
    if (need) need[j] = hit ? 1 : 0;
    if (!hit) {
        if (lens) lens[j] = 0;
        if (numbps) numbps[j] = 0;
        if (floors) floors[j] = 0;
    }
}

// Region-of-interest encode (include/j2kgfx.h, j2k_plan_roi_windows): one thread per block job, win[4 j ...] = (fx, fy, fw, fh), the footprint of
// the rectangle inside block j relative to its window, all 0 when there is none.  tests/roi_cases.py is the definition.
__global__ __launch_bounds__(256) void roi_windows_kernel(const j2k_block *__restrict__ blocks, int n, const AreaPlane *__restrict__ planes, int rx0, int ry0,
                                                          int rx1, int ry1, int margin, int32_t *__restrict__ win) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const j2k_block b = blocks[j];
    const RoiWin F = roi_window(b, planes[b.plane], rx0, ry0, rx1, ry1, margin);
    int32_t *o = win + (size_t)j * 4;
    o[0] = F.x; o[1] = F.y; o[2] = F.w; o[3] = F.h;
}

hipError_t launch_area_blocks(hipStream_t s, const j2k_block *blocks, int n, const AreaPlane *planes, int x0, int y0, int x1, int y1, int reduce, int margin,
                              uint8_t *need, uint32_t *lens, uint8_t *numbps, uint8_t *floors) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(area_blocks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, blocks, n, planes, x0, y0, x1, y1, reduce, margin, need, lens, numbps,
                       floors);
    return hipGetLastError();
}

hipError_t launch_roi_windows(hipStream_t s, const j2k_block *blocks, int n, const AreaPlane *planes, int x0, int y0, int x1, int y1, int margin, int32_t *win) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(roi_windows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, blocks, n, planes, x0, y0, x1, y1, margin, win);
    return hipGetLastError();
}

}  // namespace j2k
