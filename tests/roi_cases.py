"""The yardstick of the region-of-interest encode (roi=(x0, y0, x1, y1), roi_gain=g of encode_blocks(planes=True) / encode_frame_pixels /
encode_pixels_host, the j2k_*_roi calls), importable without a GPU: tests/test_roi_cases.py checks it on the CPU, tests/test_gpu_roi_encode.py
holds the device against it -- the windows exactly, the distortion tables bit for bit.

The rectangle is half-open, in full-resolution frame coordinates, exactly as `area` (tests/area_cases.py); g is an integer in 1 ... 65535.

Footprint.  Per tile the rectangle is cut to the tile and made relative to it (area_cases.tile_window at reduce = 0), and
area_cases.need_rects(w, h, L, 0, win, wavelet) are the rectangles of the plane whose coefficients reconstruct it.  A tile the rectangle does not
meet has no footprint.

One window per block.  A closed-loop block lies in one band rectangle, and per band and level there is one need rectangle, so the footprint inside
block j is a single, possibly empty, window F_j = (fx, fy, fw, fh) relative to the block (all 0 when empty).  block_window asserts it.

Distortion.  With d(s, k) = |v_s| - |coarse(v_s, k)| the table is D_roi[p] = sum_s m_s d(s, nb - p)^2, m_s = g inside F_j and 1 outside, in wrapping
uint64 arithmetic as rate_cases.distortion: D_roi = D + (g - 1) D_in (mod 2^64), D_in the same sum over F_j alone.  g = 1 or an empty F_j gives
rate_cases.distortion exactly; a block wholly inside the footprint gives g D mod 2^64.

Nothing else changes: the R tables, the band weights, the hull, the bisection, the layer normalisation, the packets and every decode rule are those
of rate_cases / layer_cases, which run on D_roi.  g weighs energy: g = 4^s gives the rectangle about s bit planes of priority."""
import numpy as np

import area_cases as ac
import mallat_cases as mc
import rate_cases as rc

GAIN_MAX = 65535
GAINS = (1, 2, 16, 65535)


# ---- windows ----------------------------------------------------------------------------------------------------------------------------------
def tile_rects(W, H, tile, nres, roi, wavelet):
    """per tile: the need rectangles (plane coordinates) of the rectangle's part in that tile; [] where they do not meet"""
    L = mc.levels_of(nres)
    out = []
    for x, y, w, h in mc.reduced_rects(W, H, tile, 0):
        win = ac.tile_window(ac.output_rect(roi, 0), (x, y, w, h))
        out.append([] if win is None else ac.need_rects(w, h, L, 0, win, wavelet))
    return out


def block_window(rects, x0, y0, w, h):
    """F_j of the block window (x0, y0, w, h) of a plane whose need rectangles are `rects`: (fx, fy, fw, fh) relative to the block, zeros if empty"""
    hits = []
    for qx0, qy0, qx1, qy1 in rects:
        ix0, iy0, ix1, iy1 = max(qx0, x0), max(qy0, y0), min(qx1, x0 + w), min(qy1, y0 + h)
        if ix0 < ix1 and iy0 < iy1:
            hits.append((ix0 - x0, iy0 - y0, ix1 - ix0, iy1 - iy0))
    assert len(hits) <= 1, "a block met two need rectangles: it does not lie in one band"
    return hits[0] if hits else (0, 0, 0, 0)


def frame_windows(blocks, Cn, W, H, tile, nres, roi, wavelet):
    """int32 [jobs, 4] of a plan (plan.blocks(): plane = tile * Cn + component, x0, y0, w, h)"""
    rects = tile_rects(W, H, tile, nres, roi, wavelet)
    return np.array([block_window(rects[int(b["plane"]) // Cn], int(b["x0"]), int(b["y0"]), int(b["w"]), int(b["h"])) for b in blocks], np.int32).reshape(-1, 4)


def tile_windows(jobs, rects):
    """the same for oracle.enumerate_blocks(..., windows=1)'s jobs of ONE tile and that tile's need rectangles"""
    return [block_window(rects, int(b["x0"]), int(b["y0"]), int(b["w"]), int(b["h"])) for b in jobs]


# ---- distortion -------------------------------------------------------------------------------------------------------------------------------
def distortion_roi(v, nb, F, g):
    """D_roi[0 ... nb] as Python ints (mod 2^64) of an int32 block v [h, w] with numBPS = nb, footprint F = (fx, fy, fw, fh), gain g"""
    assert 1 <= int(g) <= GAIN_MAX
    v = np.asarray(v)
    D = rc.distortion(v, nb)
    fx, fy, fw, fh = (int(x) for x in F)
    if g == 1 or fw <= 0 or fh <= 0:
        return D
    assert 0 <= fx and 0 <= fy and fx + fw <= v.shape[1] and fy + fh <= v.shape[0]
    Din = rc.distortion(np.ascontiguousarray(v[fy:fy + fh, fx:fx + fw]), nb)
    return [(d + (int(g) - 1) * di) & rc.MASK64 for d, di in zip(D, Din)]


def distortion_roi_direct(v, nb, F, g):
    """the same by a plain loop over the samples, each weighted by its own m_s (tests/test_roi_cases.py)"""
    v = np.asarray(v)
    fx, fy, fw, fh = (int(x) for x in F)
    out = []
    for p in range(nb + 1):
        k, s = nb - p, 0
        for y in range(v.shape[0]):
            for x in range(v.shape[1]):
                m = abs(int(v[y, x]))
                hi = m >> k << k
                rec = hi | (1 << (k - 1)) if (hi and k >= 1) else hi
                s += (int(g) if (fx <= x < fx + fw and fy <= y < fy + fh) else 1) * (m - rec) ** 2
        out.append(s & rc.MASK64)
    return out


def frame_distortion(block_values, nbs, wins, g, stride=rc.STRIDE):
    """uint64 [jobs, stride]: D_roi of every block (block_values[j]: int32 [h, w]); entries above numBPS are 0, as on the device"""
    out = np.zeros((len(nbs), stride), np.uint64)
    for j, (v, nb) in enumerate(zip(block_values, nbs)):
        nb = min(int(nb), stride - 1)
        if nb > 0:
            out[j, :nb + 1] = np.array(distortion_roi(v, nb, wins[j], g), np.uint64)
    return out


# ---- the effect: squared error inside / outside the rectangle after a cut ------------------------------------------------------------------------
def split_error(got, want, roi):
    """(squared error inside the rectangle, outside it) of two frames [C, H, W] or pictures [H, W]"""
    d = (np.asarray(got).astype(np.int64) - np.asarray(want).astype(np.int64)) ** 2
    x0, y0, x1, y1 = roi
    inside = int(d[..., y0:y1, x0:x1].sum())
    return inside, int(d.sum()) - inside


# ---- the cases of the issue ---------------------------------------------------------------------------------------------------------------------
# (W, H, components, precision, tile, resolutions), code-block size -- each for the 5-3 and the 9-7
GEOMETRIES = (
    ((130, 70, 3, 8, (64, 32), 3), 16),
    ((64, 48, 1, 8, (0, 0), 3), 8),
    ((33, 17, 1, 8, (0, 0), 2), 64),
)
WAVELETS = ("53", "97")


def geometry_id(g):
    return mc.case_id(g[0]) + "-cb%d" % g[1]


def rectangles(W, H):
    """area_cases.windows cut to the frame where a fixed one leaves it, plus one pixel in the middle, plus the whole frame (in windows already)"""
    out = []
    for x0, y0, x1, y1 in ac.windows(W, H) + ((W // 2, H // 2, W // 2 + 1, H // 2 + 1), (0, 0, W, H)):
        q = (max(x0, 0), max(y0, 0), min(x1, W), min(y1, H))
        if q[0] < q[2] and q[1] < q[3] and q not in out:
            out.append(q)
    return out


# the frame of the effect test: closed_loop_ref.pixel_frame gray 8-bit, seed 7, noise 16; 3 resolutions, cb 8, 5-3
EFFECT = dict(case=(64, 48, 1, 8, (0, 0), 3), cb=8, seed=7, noise=16, roi=(20, 12, 44, 36), budgets=(0.25, 0.5), gains=(1, 16))
