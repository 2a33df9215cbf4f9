"""CPU: the definition of the region decode's need set (tests/area_cases.py) against the unchanged oracle.

  sufficiency     with every coefficient outside the need rectangles zeroed (stricter than whole blocks), and with the windows of the blocks
                  that are not needed zeroed, the window of the inverse equals the window of the full inverse bit for bit -- float64
                  included, before any rounding -- on the issue's geometries and windows and on a seeded slice of random tile geometries
  insufficiency   a margin one smaller fails, for either wavelet: the margins are not loose by a whole step
  vacuity         the conditions the GPU test relies on, from the definition and the oracle's block list alone"""
import numpy as np
import pytest

import area_cases as ac
import mallat_cases as mc


def _coefs(rng, C, h, w, lossless):
    c = rng.integers(-(1 << 12), 1 << 12, (C, h, w)).astype(np.int32)
    c[rng.random((C, h, w)) < 0.3] = 0
    return c


def _same_window(oracle, coefs, masked, L, r, win, lossless):
    """the window of the synthesis of `masked` = that of `coefs`, every component, bit for bit (float64 for the 9-7)"""
    C, h, w = coefs.shape
    x0, y0, x1, y1 = win
    for c in range(C):
        a = ac.synthesize(oracle, coefs[c], w, h, L, r, lossless)[y0:y1, x0:x1]
        b = ac.synthesize(oracle, masked[c], w, h, L, r, lossless)[y0:y1, x0:x1]
        if a.tobytes() != b.tobytes():
            return False
    return True


@pytest.mark.parametrize("g", ac.GEOMETRIES, ids=ac.geometry_id)
def test_sufficient_on_the_case_list(oracle, g):
    (W, H, Cn, prec, tile, nres), cb, wavelet, q = g
    lossless = wavelet == "53"
    L = mc.levels_of(nres)
    rng = np.random.default_rng(W * 1000 + H)
    tb = ac.tile_blocks(oracle, g)
    coefs = [_coefs(rng, Cn, h, w, lossless) for (_, _, w, h), _ in tb]
    met = 0
    for area, r in ac.window_cases(W, H):
        assert r in mc.admissible(W, H, tile, nres)
        out_rect, rects = ac.output_rect(area, r), mc.reduced_rects(W, H, tile, r)
        for t, ((_, _, w, h), blocks) in enumerate(tb):
            win = ac.tile_window(out_rect, rects[t])
            need = ac.need_blocks(blocks, w, h, L, r, win, wavelet)
            if win is None:
                assert not need.any()
                continue
            met += 1
            assert _same_window(oracle, coefs[t], ac.mask_coefficients(coefs[t], w, h, L, r, win, wavelet), L, r, win, lossless), (area, r, t)
            by_blocks = ac.mask_blocks(coefs[t], blocks, need)
            assert _same_window(oracle, coefs[t], by_blocks, L, r, win, lossless), (area, r, t)
            # ... and through the whole tile inverse (dequantiser, rounding, inverse colour transform, DC shift): mallat_cases.inverse_tile
            kw = dict(lossless=lossless, quality=q, dequantize=not lossless, reduce=r)
            x0, y0, x1, y1 = win
            full = mc.inverse_tile(oracle, coefs[t], prec, nres, **kw)[:, y0:y1, x0:x1]
            assert np.array_equal(mc.inverse_tile(oracle, by_blocks, prec, nres, **kw)[:, y0:y1, x0:x1], full), (area, r, t)
    assert met >= len(ac.window_cases(W, H))


def _random_cases(seed, count):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        nres = int(rng.integers(1, 7))
        L = mc.levels_of(nres)
        C = int(rng.choice([1, 3]))
        for r in range(L + 1):
            wr, hr = mc.dims(w, h, L)[r]
            if rng.random() < 0.5:                                           # a one-pixel window
                x0, y0 = int(rng.integers(0, wr)), int(rng.integers(0, hr))
                win = (x0, y0, x0 + 1, y0 + 1)
            else:
                x0, y0 = int(rng.integers(0, wr)), int(rng.integers(0, hr))
                win = (x0, y0, int(rng.integers(x0 + 1, wr + 1)), int(rng.integers(y0 + 1, hr + 1)))
            yield rng, C, w, h, L, r, win


@pytest.mark.parametrize("wavelet", ["53", "97"])
def test_sufficient_and_tight_on_random_tiles(oracle, wavelet):
    lossless = wavelet == "53"
    tiles = short = 0
    for rng, C, w, h, L, r, win in _random_cases(20261 + int(wavelet), 40):
        coefs = _coefs(rng, C, h, w, lossless)
        assert _same_window(oracle, coefs, ac.mask_coefficients(coefs, w, h, L, r, win, wavelet), L, r, win, lossless), (w, h, L, r, win)
        tiles += 1
        if r < L and not _same_window(oracle, coefs, ac.mask_coefficients(coefs, w, h, L, r, win, wavelet, margin=ac.MARGIN[wavelet] - 1), L, r, win, lossless):
            short += 1
    assert tiles >= 80
    assert short >= tiles // 10, "a margin one smaller was expected to fail often: %d of %d" % (short, tiles)


def test_output_rect_and_empty_rectangles():
    assert ac.output_rect((3, 5, 9, 12), 0) == (3, 5, 9, 12)
    assert ac.output_rect((3, 5, 9, 12), 1) == (2, 3, 5, 6)
    assert ac.output_rect((3, 5, 9, 12), 2) == (1, 2, 3, 3)
    assert not ac.area_ok((199, 0, 200, 10), 200, 150, 1)                   # x0 = W - 1 at r = 1 with W even: empty after reduce
    assert ac.area_ok((198, 0, 200, 10), 200, 150, 1)
    for bad in ((5, 5, 5, 9), (9, 5, 5, 9), (-1, 0, 4, 4), (0, 0, 201, 4), (0, 0, 4, 151)):
        assert not ac.area_ok(bad, 200, 150, 0)
    for g in ac.GEOMETRIES:
        W, H = g[0][:2]
        assert len(ac.window_cases(W, H)) + len(ac.empty_cases(W, H)) == 7 * len(ac.REDUCES)
        assert ((W - 1, H - 1, W, H), 1) in ac.empty_cases(W, H)          # the refusal test has a case on every geometry


def test_vacuity_conditions(oracle):
    for gi, g in enumerate(ac.GEOMETRIES):
        (W, H, Cn, prec, tile, nres) = g[0]
        counts = {a: ac.count_needed(oracle, g, a, 0) for a in ac.windows(W, H)}
        total = counts[(0, 0, W, H)][1]
        assert counts[(0, 0, W, H)][0] == total                              # the whole frame needs every block
        # some window needs fewer than a third of the blocks.  The issue asks this of every geometry and, in the same table, counts 10 of 26
        # for the one-pixel window of the gray16 geometry (32 x 32 blocks, four resolutions: ten blocks is one per band); no window of its
        # list needs fewer, so that geometry is held to the count of the issue's table instead -- the other three to the third
        fewest = min(n for n, _, _ in counts.values())
        if gi == 2:
            assert (fewest, total) == (10, 26)
        else:
            assert fewest * 3 < total
        assert any(res == set(range(nres)) for _, _, res in counts.values())   # some window needs a block in every resolution
        for r in (1, 2):                                                       # the resolutions `reduce` drops are never needed
            for a, rr in ac.window_cases(W, H):
                if rr == r:
                    assert max(ac.count_needed(oracle, g, a, r)[2]) <= nres - 1 - r
    for (gi, a, r), (needed, total) in ac.COUNTS.items():
        got = ac.count_needed(oracle, ac.GEOMETRIES[gi], a, r)
        assert got[0] == needed and got[1] == total, (gi, a, r, got)
