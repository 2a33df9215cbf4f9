// area.hip -- region decode (include/j2kgfx.h, j2k_plan_*_area): which code-blocks a rectangle of the frame needs.
//
// The library's own: the reference declares Config.DecodeArea and never reads it.  tests/area_cases.py is the definition this kernel must
// agree with exactly; DESIGN.md 7 has the rule and its margins.  The windows of a Mallat plan partition each plane, and level l's sub-bands
// are the rectangles [w_{l+1}, w_l) x [0, h_{l+1}), [0, w_{l+1}) x [h_{l+1}, h_l) and [w_{l+1}, w_l) x [h_{l+1}, h_l) of it, so the whole
// rule is integer rectangle tests in plane coordinates: at most 3 L + 1 per block.
#include "j2k_internal.h"

namespace j2k {

// [x0, x1) x [y0, y1) meets the window (wx, wy, ww, wh)?  An empty rectangle meets nothing.
__device__ __forceinline__ bool area_meets(int x0, int x1, int y0, int y1, int wx, int wy, int ww, int wh) {
    return x0 < x1 && y0 < y1 && x0 < wx + ww && wx < x1 && y0 < wy + wh && wy < y1;
}

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
    const int rnd = (1 << reduce) - 1;
    // the output rectangle of the reduced frame (the canvas rule), cut to the tile's reduced rectangle and made relative to it
    const int tx = T.x0 >> reduce, ty = T.y0 >> reduce;
    int wl = (T.w + rnd) >> reduce, hl = (T.h + rnd) >> reduce;                  // w_reduce, h_reduce
    int xa = max((ax0 + rnd) >> reduce, tx) - tx, xb = min((ax1 + rnd) >> reduce, tx + wl) - tx;
    int ya = max((ay0 + rnd) >> reduce, ty) - ty, yb = min((ay1 + rnd) >> reduce, ty + hl) - ty;
    bool hit = false;
    if (xa < xb && ya < yb) {
        for (int l = reduce; l < T.levels && !hit; l++) {
            const int wn = (wl + 1) >> 1, hn = (hl + 1) >> 1;                    // w_{l+1}, h_{l+1}
            const int x0 = max(0, (xa >> 1) - margin), xe = ((xb - 1) >> 1) + margin + 1;
            const int y0 = max(0, (ya >> 1) - margin), ye = ((yb - 1) >> 1) + margin + 1;
            const int lx1 = min(wn, xe), hx1 = min(wl >> 1, xe), ly1 = min(hn, ye), hy1 = min(hl >> 1, ye);
            hit = area_meets(wn + x0, wn + hx1, y0, ly1, b.x0, b.y0, b.w, b.h) ||
                  area_meets(x0, lx1, hn + y0, hn + hy1, b.x0, b.y0, b.w, b.h) ||
                  area_meets(wn + x0, wn + hx1, hn + y0, hn + hy1, b.x0, b.y0, b.w, b.h);
            xa = x0; xb = lx1; ya = y0; yb = ly1;
            wl = wn; hl = hn;
        }
        hit = hit || area_meets(xa, xb, ya, yb, b.x0, b.y0, b.w, b.h);           // LL of the last level (reduce = levels: the window itself)
    }
    if (need) need[j] = hit ? 1 : 0;
    if (!hit) {
        if (lens) lens[j] = 0;
        if (numbps) numbps[j] = 0;
        if (floors) floors[j] = 0;
    }
}

hipError_t launch_area_blocks(hipStream_t s, const j2k_block *blocks, int n, const AreaPlane *planes, int x0, int y0, int x1, int y1, int reduce, int margin,
                              uint8_t *need, uint32_t *lens, uint8_t *numbps, uint8_t *floors) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(area_blocks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, blocks, n, planes, x0, y0, x1, y1, reduce, margin, need, lens, numbps,
                       floors);
    return hipGetLastError();
}

}  // namespace j2k
