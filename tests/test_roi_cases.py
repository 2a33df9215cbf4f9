"""CPU: the yardstick of the region-of-interest encode (tests/roi_cases.py) checked against itself and the oracle -- every block's footprint is one
window of area_cases.need_rects, the weighted distortion against a direct per-sample loop and its equalities (g = 1, a block wholly inside, the
wrapping case), the effect of the weight on a real frame through the unchanged allocation (the error inside the rectangle falls, outside it does
not) -- and the new names in the header and the binding."""
import functools
import os
import re

import numpy as np
import pytest

import area_cases as ac
import coarse_cases as cc
import layer_cases as lc
import mallat_cases as mc
import rate_cases as rc
import roi_cases as roi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("j2k_plan_roi_windows", "j2k_plan_encode_blocks_planes_roi", "j2k_plan_encode_frame_pixels_roi", "j2k_encode_pixels_host_roi")


# ---- windows ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", roi.WAVELETS)
@pytest.mark.parametrize("g", roi.GEOMETRIES, ids=[roi.geometry_id(g) for g in roi.GEOMETRIES])
def test_one_window_per_block(oracle, g, wavelet):
    """F_j from need_rects: at most one non-empty intersection per block (block_window asserts it), inside the block, and together the windows of a
    tile-component cover exactly the need rectangles"""
    (W, H, Cn, _prec, tile, nres), cb = g
    tiles = mc.tiles_of(W, H, tile)
    jobs = [oracle.enumerate_blocks(Cn, w, h, nres, cb, cb, 1) for _, _, w, h in tiles]
    rects_of = roi.rectangles(W, H)
    assert (0, 0, W, H) in rects_of and any(q[2] - q[0] == 1 and q[3] - q[1] == 1 for q in rects_of)
    partial = 0
    for q in rects_of:
        rects = roi.tile_rects(W, H, tile, nres, q, wavelet)
        assert len(rects) == len(tiles)
        for t, (tx, ty, w, h) in enumerate(tiles):
            meets = q[0] < tx + w and tx < q[2] and q[1] < ty + h and ty < q[3]
            assert bool(rects[t]) == meets                           # a tile the rectangle does not meet has no footprint
            wins = roi.tile_windows(jobs[t], rects[t])
            want = np.zeros((h, w), np.int32)
            for x0, y0, x1, y1 in rects[t]:
                want[y0:y1, x0:x1] += 1
            assert want.max(initial=0) <= 1                          # the need rectangles of one plane do not overlap
            got = np.zeros((Cn, h, w), np.int32)
            for b, (fx, fy, fw, fh) in zip(jobs[t], wins):
                bw, bh = int(b["w"]), int(b["h"])
                if fw == 0 or fh == 0:
                    assert (fx, fy, fw, fh) == (0, 0, 0, 0)
                    continue
                assert 0 <= fx and 0 <= fy and fx + fw <= bw and fy + fh <= bh
                partial += (fw, fh) != (bw, bh)
                got[int(b["comp"]), int(b["y0"]) + fy:int(b["y0"]) + fy + fh, int(b["x0"]) + fx:int(b["x0"]) + fx + fw] += 1
            for c in range(Cn):
                assert np.array_equal(got[c], want), (q, t, c)
        if q == (0, 0, W, H):                                        # the whole frame: every block wholly inside
            for t in range(len(tiles)):
                for b, F in zip(jobs[t], roi.tile_windows(jobs[t], rects[t])):
                    assert F == (0, 0, int(b["w"]), int(b["h"]))
    assert partial > 0, "vacuous: no block is cut by a footprint"


def test_frame_windows_follow_the_plane_numbering(oracle):
    """frame_windows on records numbered like plan.blocks() (plane = tile * Cn + component) agrees with the per-tile form"""
    (W, H, Cn, _prec, tile, nres), cb = roi.GEOMETRIES[0]
    recs = []
    for t, (_, _, w, h) in enumerate(mc.tiles_of(W, H, tile)):
        recs += [dict(plane=t * Cn + int(b["comp"]), x0=b["x0"], y0=b["y0"], w=b["w"], h=b["h"]) for b in oracle.enumerate_blocks(Cn, w, h, nres, cb, cb, 1)]
    q = (37, 11, 90, 40)
    wins = roi.frame_windows(recs, Cn, W, H, tile, nres, q, "53")
    rects = roi.tile_rects(W, H, tile, nres, q, "53")
    assert wins.shape == (len(recs), 4) and wins.dtype == np.int32
    for r, F in zip(recs, wins):
        assert tuple(F) == roi.block_window(rects[r["plane"] // Cn], int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"]))
    assert 0 < int((wins[:, 2] > 0).sum()) < len(recs)


# ---- distortion -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,sparse", [(1, False), (4, False), (8, True), (16, False), (31, True)])
@pytest.mark.parametrize("g", roi.GAINS)
def test_distortion_against_direct_loop(bits, sparse, g):
    rng = np.random.default_rng(bits)
    v = cc.samples(rng, 9, 7, bits, sparse).reshape(7, 9)
    for F in ((2, 1, 4, 3), (0, 0, 1, 1), (8, 6, 1, 1), (0, 3, 9, 2)):
        D = roi.distortion_roi(v, bits, F, g)
        assert D == roi.distortion_roi_direct(v, bits, F, g), F
        assert len(D) == bits + 1 and D[bits] == 0
    if g > 1 and bits < 31:
        assert roi.distortion_roi(v, bits, (2, 1, 4, 3), g) != rc.distortion(v, bits)


def test_gain_one_and_no_footprint_are_the_plain_table():
    rng = np.random.default_rng(11)
    v = cc.samples(rng, 9, 7, 12).reshape(7, 9)
    D = rc.distortion(v, 12)
    assert roi.distortion_roi(v, 12, (2, 1, 4, 3), 1) == D
    assert roi.distortion_roi(v, 12, (0, 0, 0, 0), 65535) == D
    assert roi.distortion_roi_direct(v, 12, (0, 0, 0, 0), 65535) == D


@pytest.mark.parametrize("g", roi.GAINS)
def test_fully_inside_multiplies(g):
    rng = np.random.default_rng(12)
    v = cc.samples(rng, 9, 7, 16).reshape(7, 9)
    assert roi.distortion_roi(v, 16, (0, 0, 9, 7), g) == [(g * d) & rc.MASK64 for d in rc.distortion(v, 16)]


def test_distortion_wraps_like_numpy():
    """rate_cases' wrapping case with the largest gain: 65535 * 4096 * (2^31 - 1)^2 mod 2^64, whole block and a part of it"""
    v = np.full((64, 64), (1 << 31) - 1, np.int32)
    e = ((1 << 31) - 1) ** 2
    D = roi.distortion_roi(v, 31, (0, 0, 64, 64), 65535)
    assert D[0] == (65535 * 4096 * e) & rc.MASK64
    D = roi.distortion_roi(v, 31, (5, 60, 59, 4), 65535)
    assert D[0] == ((4096 + 65534 * 59 * 4) * e) & rc.MASK64
    small = np.full((3, 5), (1 << 31) - 1, np.int32)                 # the direct loop on a block it can afford
    assert roi.distortion_roi(small, 31, (1, 1, 3, 2), 65535) == roi.distortion_roi_direct(small, 31, (1, 1, 3, 2), 65535)


# ---- effect -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _effect_tables():
    import oracle as orc
    E = roi.EFFECT
    tab = lc.golden_tables(dict(case=E["case"], cb=E["cb"], seed=E["seed"]), orc)     # (noise = 2^prec / 16 = 16)
    W, H, Cn, prec, tile, nres = E["case"]
    jobs = orc.enumerate_blocks(Cn, W, H, nres, E["cb"], E["cb"], 1)
    return tab, jobs


def _effect_errors(orc, g, frac):
    """(inside, outside, chosen bytes, budget) of the effect frame cut to `frac` of its body bytes with gain g"""
    E = roi.EFFECT
    W, H, Cn, prec, tile, nres = E["case"]
    (pix, tiles, datas, nbs, Rs, Ds, ws, ctiles), jobs = _effect_tables()
    wins = roi.tile_windows(jobs, roi.tile_rects(W, H, tile, nres, E["roi"], "53")[0])
    Dr = [roi.distortion_roi(lc.np_block(ctiles[0], b), nbs[j], wins[j], g) for j, b in enumerate(jobs)]
    budget = int(sum(int(R[nb]) for R, nb in zip(Rs, nbs)) * frac)
    ps, chosen = rc.allocate(Rs, Dr, nbs, ws, budget)
    cut = ctiles[0].copy()
    for j, b in enumerate(jobs):
        ys, xs = slice(int(b["y0"]), int(b["y0"]) + int(b["h"])), slice(int(b["x0"]), int(b["x0"]) + int(b["w"]))
        cut[int(b["comp"]), ys, xs] = cc.coarse(ctiles[0][int(b["comp"]), ys, xs], nbs[j] - ps[j])
    full = mc.inverse_frame(orc, ctiles, W, H, tile, prec, nres)
    got = mc.inverse_frame(orc, [cut], W, H, tile, prec, nres)
    return roi.split_error(got, full, E["roi"]) + (chosen, budget)


def test_effect_on_a_frame(oracle):
    """gray 8-bit 64 x 48, 3 resolutions, cb 8, 5-3, roi (20, 12, 44, 36): at 25 % and 50 % of the uncut body bytes the squared error inside the
    rectangle is smaller with g = 16 than with g = 1 and the error outside is not; the chosen bytes stay within the budget.  (Measured with the
    oracle's codewords and shortest_rates: inside 25 267 -> 8 928 at 25 %, 4 520 -> 1 744 at 50 %; outside 92 342 -> 131 197 at 25 %.)"""
    for frac in roi.EFFECT["budgets"]:
        in1, out1, c1, b1 = _effect_errors(oracle, 1, frac)
        in16, out16, c16, b16 = _effect_errors(oracle, 16, frac)
        print("budget %.0f %%: inside %d -> %d, outside %d -> %d, bytes %d / %d of %d" % (100 * frac, in1, in16, out1, out16, c1, c16, b1))
        assert c1 <= b1 and c16 <= b16
        assert in16 < in1, frac
        assert out16 >= out1, frac


# ---- names ------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "j2kgfx.h")).read()
    libpy = open(os.path.join(ROOT, "go-jpeg2000_amd", "j2kgfx", "_lib.py")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert '"%s"' % s in libpy, s
