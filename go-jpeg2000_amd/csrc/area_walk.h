// area_walk.h -- the walk down the synthesis that area.hip (which blocks a rectangle needs) and rate.hip (which samples of a block a region of
// interest weights) share: the rectangles of a tile-component's plane whose coefficients reconstruct a rectangle of the frame.
// tests/area_cases.py (need_rects) is the definition; DESIGN.md 7 has the rule and its margins.
#pragma once
#include "j2k_internal.h"

namespace j2k {

// [x0, x1) x [y0, y1) meets the window (wx, wy, ww, wh)?  An empty rectangle meets nothing.
__device__ __forceinline__ bool area_meets(int x0, int x1, int y0, int y1, int wx, int wy, int ww, int wh) {
    return x0 < x1 && y0 < y1 && x0 < wx + ww && wx < x1 && y0 < wy + wh && wy < y1;
}

// visit(x0, x1, y0, y1) for every need rectangle of plane T (plane coordinates; some may be empty) of the frame rectangle [ax0, ax1) x
// [ay0, ay1) decoded `reduce` resolutions down, level by level (HL, LH, HH), then the LL of the last level, until a visit returns true.
// Returns whether one did.  Blocks of the resolutions `reduce` drops lie outside [0, w_reduce) x [0, h_reduce) and so are never visited.
template <typename Visit>
__device__ __forceinline__ bool area_walk(const AreaPlane &T, int ax0, int ay0, int ax1, int ay1, int reduce, int margin, Visit visit) {
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
            hit = visit(wn + x0, wn + hx1, y0, ly1) || visit(x0, lx1, hn + y0, hn + hy1) || visit(wn + x0, wn + hx1, hn + y0, hn + hy1);
            xa = x0; xb = lx1; ya = y0; yb = ly1;
            wl = wn; hl = hn;
        }
        hit = hit || visit(xa, xb, ya, yb);                                      // LL of the last level (reduce = levels: the window itself)
    }
    return hit;
}

// The footprint of a region of interest inside one block (tests/roi_cases.py: block_window): the part of the block's window that lies in the
// need rectangles of the frame rectangle at reduce = 0, relative to the window; w = h = 0 when there is none.  A closed-loop block lies in
// one band rectangle and a band has one need rectangle, so the first rectangle that meets the window is the only one.
struct RoiWin { int32_t x, y, w, h; };
__device__ __forceinline__ RoiWin roi_window(const j2k_block &b, const AreaPlane &T, int rx0, int ry0, int rx1, int ry1, int margin) {
    RoiWin F{0, 0, 0, 0};
    area_walk(T, rx0, ry0, rx1, ry1, 0, margin, [&](int x0, int x1, int y0, int y1) {
        const int ix0 = max(x0, b.x0), ix1 = min(x1, b.x0 + b.w), iy0 = max(y0, b.y0), iy1 = min(y1, b.y0 + b.h);
        if (ix0 >= ix1 || iy0 >= iy1) return false;
        F = RoiWin{ix0 - b.x0, iy0 - b.y0, ix1 - ix0, iy1 - iy0};
        return true;
    });
    return F;
}

}  // namespace j2k
