"""CPU: the yardstick of tests/mallat_cases.py checked against the oracle itself -- the composition around the levels is the oracle's
(swap the per-level step for the oracle's multi-level call and oracle.preprocess comes out bit for bit), lossless round trips, reduced tiles
cover the reduced frame exactly once, reduced frames are pictures, lossy frames decode to the picture, and the Mallat coefficients code
smaller than the prefix layout's with both coders.  The figures in the docstrings were measured with the oracle alone."""
import hashlib
import json
import os

import numpy as np
import pytest

import closed_loop_ref as ref
import dequantize_cases as dq
import mallat_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))


def _prefix_equals_preprocess(oracle, frm, tile, prec, nres, lossless, quality):
    _, H, W = frm.shape
    got = mc.forward_frame(oracle, frm, tile, prec, nres, lossless, quality, prefix=True)
    for t, (x0, y0, w, h) in enumerate(mc.tiles_of(W, H, tile)):
        sub = [np.ascontiguousarray(frm[c, y0:y0 + h, x0:x0 + w]).astype(np.int32) for c in range(frm.shape[0])]
        want = np.stack(oracle.preprocess(sub, w, h, prec, lossless, nres, quality))
        assert np.array_equal(got[t], want), t


@pytest.mark.parametrize("case", mc.LOSSLESS, ids=mc.case_id)
def test_glue_is_the_oracles_lossless(oracle, case):
    W, H, Cn, prec, tile, nres = case
    for family in ("noise", "impulse"):
        _prefix_equals_preprocess(oracle, mc.lossless_frame(case, family), tile, prec, nres, True, 0)


@pytest.mark.parametrize("case", mc.LOSSY + tuple(dq.FRAMES), ids=mc.case_id)
def test_glue_is_the_oracles_lossy(oracle, case):
    W, H, Cn, prec, tile, nres, q = case
    _prefix_equals_preprocess(oracle, ref.frame_n(W, H, Cn, prec, 41), tile, prec, nres, False, q)


@pytest.mark.parametrize("case", mc.LOSSLESS, ids=mc.case_id)
def test_lossless_round_trip_and_contrast(oracle, case):
    """forward then inverse at reduce 0 returns the source; with two levels or more the coefficients are not encoder.preprocess's"""
    W, H, Cn, prec, tile, nres = case
    frm = mc.lossless_frame(case, "noise")
    tiles = mc.forward_frame(oracle, frm, tile, prec, nres)
    assert np.array_equal(mc.inverse_frame(oracle, tiles, W, H, tile, prec, nres), frm)
    if mc.levels_of(nres) >= 2:
        prefix = mc.forward_frame(oracle, frm, tile, prec, nres, prefix=True)
        assert any(not np.array_equal(a, b) for a, b in zip(tiles, prefix))


@pytest.mark.parametrize("case", mc.LOSSLESS + mc.LOSSY, ids=mc.case_id)
def test_reduced_tiles_cover_the_reduced_frame_once(case):
    W, H, tile, nres = case[0], case[1], case[4], case[5]
    rs = mc.admissible(W, H, tile, nres)
    assert rs[0] == 0 and (tile != (0, 0) or rs == list(range(mc.levels_of(nres) + 1)))
    for r in rs:
        cover = np.zeros((mc.shr(H, r), mc.shr(W, r)), np.int32)
        for x, y, w, h in mc.reduced_rects(W, H, tile, r):
            cover[y:y + h, x:x + w] += 1
        assert (cover == 1).all(), r


def test_admissible_follows_the_tile_and_the_batch():
    assert mc.admissible(260, 44, (128, 32), 4) == [0, 1, 2, 3]
    assert mc.admissible(200, 150, (64, 64), 6) == [0, 1, 2, 3, 4, 5]
    assert mc.admissible(260, 88, (128, 32), 4, frame_rows=44) == [0, 1, 2]          # 44 = 4 * 11
    assert mc.admissible(100, 60, (40, 24), 6) == [0, 1, 2, 3]                        # 40 = 8 * 5, 24 = 8 * 3
    for r in (1, 2):
        cover = np.zeros((mc.shr(88, r), mc.shr(260, r)), np.int32)
        for x, y, w, h in mc.reduced_rects(260, 88, (128, 32), r, frame_rows=44):
            cover[y:y + h, x:x + w] += 1
        assert (cover == 1).all()


@pytest.mark.parametrize("W,H,tile,nres", mc.PICTURES, ids=lambda v: str(v))
def test_lossless_reduced_frames_are_pictures(oracle, W, H, tile, nres):
    """closed_loop_ref.frame(W, H, 3, 16): the clamped reduced frame stays within 32 of the 2^r x 2^r box mean of the source (measured: 11.5 ... 24.9;
    the frame's noise is +-16 and the 5-3 low-pass is not a box filter).  130 x 70 at reduce 1: samples leave 0 ... 255 before the clamp."""
    frm = ref.frame(W, H, 3, 16).astype(np.int32)
    tiles = mc.forward_frame(oracle, frm, tile, 8, nres)
    seen = 0
    for r in mc.admissible(W, H, tile, nres):
        if mc.shr(W, r) < 16 or mc.shr(H, r) < 5:
            continue
        got = mc.inverse_frame(oracle, tiles, W, H, tile, 8, nres, reduce=r)
        if r == 0:
            assert np.array_equal(got, frm)
        if (W, H, r) == (130, 70, 1):
            assert np.count_nonzero((got < 0) | (got > 255)) > 0          # the case for the pack's clamp
        err = np.abs(np.clip(got, 0, 255) - mc.box_mean(frm, r)).max()
        assert err <= mc.PICTURE_BOUND, (r, err)
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("i,f", list(enumerate(dq.FRAMES)), ids=[dq.frame_id(f) for f in dq.FRAMES])
def test_lossy_dequantised_frames_decode_to_the_picture(oracle, i, f):
    """max error <= dequantize_cases.MAX_ERR (measured 1 ... 8; the prefix layout gives 1 ... 9)"""
    W, H, Cn, prec, tile, nres, q = f
    frm = dq.source_frame(f, i)
    tiles = mc.forward_frame(oracle, frm, tile, prec, nres, False, q)
    back = mc.inverse_frame(oracle, tiles, W, H, tile, prec, nres, False, q, dequantize=True)
    err = int(np.abs(back.astype(np.int64) - frm.astype(np.int64)).max())
    print("%s: max abs err %d" % (dq.frame_id(f), err))
    assert err <= dq.MAX_ERR


@pytest.mark.parametrize("noise", [0, 16])
def test_mallat_coefficients_code_smaller(oracle, noise):
    """closed-loop windows, 256 x 256 RGB, 6 resolutions, 64 x 64 blocks: fewer MQ bytes and fewer HT bytes than encoder.preprocess's coefficients
    (measured, prefix -> Mallat: noise 0 MQ 33 312 -> 5 321, HT 113 522 -> 94 456; noise 16 MQ 146 038 -> 140 324)"""
    frm = ref.frame(256, 256, 7, noise).astype(np.int32)
    mal = mc.forward_frame(oracle, frm, (0, 0), 8, 6)
    pre = mc.forward_frame(oracle, frm, (0, 0), 8, 6, prefix=True)
    for coder in (0, 1):
        a, b = mc.stream_bytes(oracle, mal, 6, 64, coder), mc.stream_bytes(oracle, pre, 6, 64, coder)
        print("noise %d coder %d: prefix %d bytes, Mallat %d bytes" % (noise, coder, b, a))
        assert a < b, (coder, a, b)


# ---- the byte format, pinned ---------------------------------------------------------------------------------------------------------------
GOLDEN = json.load(open(os.path.join(HERE, "golden", mc.GOLDEN_FILE)))


def test_golden_file_covers_the_cases():
    assert sorted(GOLDEN) == sorted(c["name"] for c in mc.GOLDEN_CASES)


@pytest.mark.parametrize("case", mc.GOLDEN_CASES, ids=[c["name"] for c in mc.GOLDEN_CASES])
def test_oracle_composes_the_pinned_tile_parts(oracle, case):
    import t2ref
    frm, want, stream = mc.golden_stream(case, oracle, t2ref)
    g = GOLDEN[case["name"]]
    assert len(stream) == g["bytes"] and stream[:24].hex() == g["head"]
    assert hashlib.sha256(stream).hexdigest() == g["sha256"]
    # and the MQ stream decodes back to the source through the yardstick's inverse
    if case["coder"] == 0:
        tiles = mc.decoded_tiles(oracle, want, 3, case["nres"], case["cb"], 0)
        assert np.array_equal(mc.inverse_frame(oracle, tiles, case["W"], case["H"], case["tile"], 8, case["nres"]), frm.astype(np.int32))
