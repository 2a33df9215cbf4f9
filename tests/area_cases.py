"""The yardstick of the region decode (area=(x0, y0, x1, y1) of decode_frame_pixels / decode_pixels_host, the j2k_*_area calls), importable without
a GPU: tests/test_area_cases.py checks it on the CPU, tests/test_gpu_area_decode.py holds the device against it -- the need set exactly, the
pixels bit for bit.

The rectangle is half-open, in full-resolution frame coordinates.  With reduce = r the result is the rectangle output_rect(area, r) of the
reduced frame (the canvas rule: both corners ceil-divided by 2^r), and its pixels are the yardstick's FULL decode of the same call without
`area`, cropped (crop): nothing here computes pixels of its own.

The need set.  Per tile the output rectangle is cut to the tile's reduced rectangle (mallat_cases.reduced_rects) and made relative to it: the
window.  A tile-component of w x h with L levels and (w_l, h_l) = mallat_cases.dims is walked from l = r to L - 1.  Per axis, with the current
interval [a, b) and n = w_l (or h_l), and the margin m = MARGIN[wavelet]:

    lo = [max(0, a // 2 - m), min(ceil(n / 2), (b - 1) // 2 + m + 1))        low-pass samples of level l
    hi = [max(0, a // 2 - m), min(n // 2,      (b - 1) // 2 + m + 1))        high-pass samples of level l

The rectangles needed at level l, in plane coordinates (the Mallat layout), are (w_{l+1} + hi_x) x lo_y, lo_x x (h_{l+1} + hi_y) and
(w_{l+1} + hi_x) x (h_{l+1} + hi_y); then [a, b) <- lo on both axes.  After the last level lo_x x lo_y is needed, the LL rectangle (for r = L:
the window itself).  A code-block is needed iff its window in the plane meets one of these rectangles; the windows of a closed-loop plan
partition the plane, so no band names are involved.  Blocks of the resolutions `reduce` drops lie outside every such rectangle.

Why the margins: sample x of a synthesis is a lifting chain over interleaved neighbours, x +- 2 for the 5-3 (one predict, one update) and
x +- 4 for the 9-7 (two of each), so in subsampled coordinates one and two samples either side.  tests/test_area_cases.py shows on the
unchanged oracle that they suffice bit for bit and that one less does not."""
import numpy as np

import mallat_cases as mc

MARGIN = {"53": 1, "97": 2}


def output_rect(area, r):
    """(x0, y0, x1, y1) of the reduced frame; empty (x0 >= x1 or y0 >= y1) means the call is an error"""
    return tuple(mc.shr(int(v), r) for v in area)


def area_ok(area, W, H, r):
    x0, y0, x1, y1 = area
    if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
        return False
    a, b, c, d = output_rect(area, r)
    return a < c and b < d


def tile_window(out, rect):
    """the output rectangle cut to a tile's reduced rectangle (x, y, w, h), relative to it; None if they do not meet"""
    x, y, w, h = rect
    x0, y0, x1, y1 = max(out[0], x), max(out[1], y), min(out[2], x + w), min(out[3], y + h)
    if x0 >= x1 or y0 >= y1:
        return None
    return x0 - x, y0 - y, x1 - x, y1 - y


def _step(a, b, n, m):
    lo0 = max(0, a // 2 - m)
    end = (b - 1) // 2 + m + 1
    return (lo0, min((n + 1) // 2, end)), (lo0, min(n // 2, end))


def need_rects(w, h, L, r, win, wavelet, margin=None):
    """the rectangles (x0, y0, x1, y1), plane coordinates, that the window win = (x0, y0, x1, y1) of the tile's reduced rectangle needs of a
    w x h tile-component with L levels; empty ones are left out.  margin: MARGIN[wavelet] unless given (the insufficiency test)"""
    m = MARGIN[wavelet] if margin is None else margin
    d = mc.dims(w, h, L)
    ax, ay, bx, by = win
    assert 0 <= r <= L and 0 <= ax < bx <= d[r][0] and 0 <= ay < by <= d[r][1]
    out = []
    for l in range(r, L):
        (wl, hl), (wn, hn) = d[l], d[l + 1]
        lox, hix = _step(ax, bx, wl, m)
        loy, hiy = _step(ay, by, hl, m)
        out += [(wn + hix[0], loy[0], wn + hix[1], loy[1]), (lox[0], hn + hiy[0], lox[1], hn + hiy[1]), (wn + hix[0], hn + hiy[0], wn + hix[1], hn + hiy[1])]
        (ax, bx), (ay, by) = lox, loy
    out.append((ax, ay, bx, by))
    return [q for q in out if q[0] < q[2] and q[1] < q[3]]


def meets(q, x0, y0, w, h):
    return q[0] < x0 + w and x0 < q[2] and q[1] < y0 + h and y0 < q[3]


def need_blocks(blocks, w, h, L, r, win, wavelet, margin=None):
    """bool per block of ONE tile-component's plane (records with x0, y0, w, h: oracle.enumerate_blocks(..., windows=1) or plan.blocks());
    win None: the tile does not meet the rectangle, nothing is needed"""
    if win is None:
        return np.zeros(len(blocks), bool)
    rects = need_rects(w, h, L, r, win, wavelet, margin)
    return np.array([any(meets(q, int(b["x0"]), int(b["y0"]), int(b["w"]), int(b["h"])) for q in rects) for b in blocks], bool)


def frame_need(blocks, Cn, W, H, tile, nres, r, area, wavelet):
    """bool per job of a plan (plan.blocks(): plane = tile * Cn + component)"""
    out_rect = output_rect(area, r)
    rects = mc.reduced_rects(W, H, tile, r)
    tiles = mc.tiles_of(W, H, tile)
    L = mc.levels_of(nres)
    planes = np.asarray(blocks["plane"]).astype(np.int64)
    need = np.zeros(len(blocks), bool)
    for t, (_, _, w, h) in enumerate(tiles):
        win = tile_window(out_rect, rects[t])
        sel = np.nonzero(planes // Cn == t)[0]
        need[sel] = need_blocks(blocks[sel], w, h, L, r, win, wavelet)
    return need


def mask_coefficients(coefs, w, h, L, r, win, wavelet, margin=None):
    """a copy of one tile's coefficients [C, h, w] with everything outside the need rectangles zeroed (stricter than whole blocks)"""
    keep = np.zeros((h, w), bool)
    for x0, y0, x1, y1 in need_rects(w, h, L, r, win, wavelet, margin):
        keep[y0:y1, x0:x1] = True
    return np.where(keep[None], coefs, 0).astype(coefs.dtype)


def mask_blocks(coefs, blocks, need):
    """a copy of one tile's coefficients [C, h, w] with the windows of the blocks that are not needed zeroed (records with comp, x0, y0, w, h)"""
    out = coefs.copy()
    for b, n in zip(blocks, need):
        if not n:
            out[int(b["comp"]), int(b["y0"]):int(b["y0"]) + int(b["h"]), int(b["x0"]):int(b["x0"]) + int(b["w"])] = 0
    return out


def synthesize(oracle, plane, w, h, L, r, lossless):
    """mallat_cases.inverse_tile's level loop alone on one plane (int32 for the 5-3, float64 for the 9-7): levels L - 1 ... r, cropped to
    [0, w_r) x [0, h_r) -- before any rounding, so that a float64 comparison is one of the transform itself"""
    d = mc.dims(w, h, L)
    p = np.array(plane, dtype=np.int32 if lossless else np.float64).reshape(h, w)
    for l in range(L - 1, r - 1, -1):
        wl, hl = d[l]
        rect = np.ascontiguousarray(p[:hl, :wl])
        p[:hl, :wl] = (oracle.inv53_2d if lossless else oracle.inv97_2d)(rect, wl, hl)
    return np.ascontiguousarray(p[:d[r][1], :d[r][0]])


def crop(full_pix, area, r, bpp):
    """the expectation: the yardstick's full decode (uint8 [H_r, >= W_r * bpp], the Go Pix layout) cut to output_rect(area, r): uint8 [h, w * bpp]"""
    x0, y0, x1, y1 = output_rect(area, r)
    return np.ascontiguousarray(full_pix[y0:y1, x0 * bpp:x1 * bpp])


def bytes_per_pixel(Cn, prec):
    return (1 if Cn == 1 else 4) * (2 if prec > 8 else 1)


# ---- the cases of the issue -----------------------------------------------------------------------------------------------------------------
# (W, H, components, precision, tile, resolutions), code-block size, wavelet, Quality
GEOMETRIES = (
    ((200, 150, 3, 8, (64, 64), 6), 16, "53", 0),
    ((260, 44, 3, 8, (128, 32), 4), 16, "53", 0),
    ((130, 70, 1, 16, (0, 0), 4), 32, "53", 0),
    ((130, 70, 3, 8, (0, 0), 4), 16, "97", 75),        # dequantize=True
)
REDUCES = (0, 1, 2)


def geometry_id(g):
    return mc.case_id(g[0]) + "-cb%d-%s" % (g[1], g[2])


def windows(W, H):
    return (
        (0, 0, 1, 1), (W - 1, H - 1, W, H),                             # one pixel, first and last
        (0, 0, W, H),                                                   # the whole frame
        (W // 2 - 9, H // 2 - 7, W // 2 + 8, H // 2 + 6),               # odd origin, across the tile seams of the tiled cases
        (0, H - 3, W, H), (W - 5, 0, W, H),                             # the last three rows, the last five columns
        (37, 11, 90, 40),
    )


def window_cases(W, H):
    """(window, reduce) of a geometry whose reduced rectangle is not empty; the others belong to the refusals (empty_cases)"""
    return [(a, r) for a in windows(W, H) for r in REDUCES if area_ok(a, W, H, r)]


def empty_cases(W, H):
    return [(a, r) for a in windows(W, H) for r in REDUCES if not area_ok(a, W, H, r)]


# block counts of the issue: {(geometry index, window, reduce): (needed, total or None)}
COUNTS = {
    (0, (0, 0, 1, 1), 0): (48, 747), (0, (37, 11, 90, 40), 0): (114, 747),
    (1, (37, 11, 90, 40), 0): (96, 312),
    (2, (0, 0, 1, 1), 0): (10, 26),
    (3, (0, 0, 1, 1), 0): (30, 195),
}


def tile_blocks(oracle, g):
    """[(tile rectangle, oracle.enumerate_blocks of the tile)] of a geometry"""
    (W, H, Cn, _prec, tile, nres), cb = g[0], g[1]
    return [((x0, y0, w, h), oracle.enumerate_blocks(Cn, w, h, nres, cb, cb, 1)) for x0, y0, w, h in mc.tiles_of(W, H, tile)]


def count_needed(oracle, g, area, r):
    """(needed, total, resolutions with a needed block) over the frame, from the definition and the oracle's block list alone"""
    (W, H, Cn, _prec, tile, nres), wavelet = g[0], g[2]
    out_rect, rects, L = output_rect(area, r), mc.reduced_rects(W, H, tile, r), mc.levels_of(nres)
    needed = total = 0
    res = set()
    for t, ((_, _, w, h), blocks) in enumerate(tile_blocks(oracle, g)):
        need = need_blocks(blocks, w, h, L, r, tile_window(out_rect, rects[t]), wavelet)
        needed += int(need.sum()); total += len(blocks)
        res |= {int(b["res"]) for b, n in zip(blocks, need) if n}
    return needed, total, res
