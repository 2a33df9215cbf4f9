"""CPU: tests/pass_cases.py, the definition of pass-level rate control, checked against itself and against the plane-level definitions it extends
(coarse_cases.coarse, rate_cases.distortion / floors_from_header / passes_of); the new entry points are declared and bound."""
import os
import re

import numpy as np
import pytest

import coarse_cases as cc
import pass_cases as pc
import rate_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(w, h, c) for (w, h) in ((1, 1), (5, 7), (8, 8), (16, 16), (9, 33)) for c in pc.CONTENTS]


def _blocks():
    for w, h, c in CASES:
        v = pc.block(w, h, c)
        yield w, h, c, v, pc.numbps_of(v)


def test_families_are_what_they_say():
    for w, h, c, v, nb in _blocks():
        assert v.shape == (h, w) and v.dtype == np.int32
        if c == "zero":
            assert nb == 0
        if c == "deep":
            assert nb == 31 and pc.points(nb) == 91
        if c == "sparse":
            assert 1 <= np.count_nonzero(v) <= max(3, (w * h) // 20)
    big = pc.block(64, 64, "sparse")
    assert 0.003 < np.count_nonzero(big) / big.size < 0.03


def test_pass_index_is_the_headers_convention():
    for p in range(1, 32):
        assert pc.split(rc.passes_of(p)) == (p, 0)
    assert [pc.split(q) for q in (1, 2, 3, 4, 5)] == [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1)]
    assert pc.points(0) == 0 and pc.points(1) == 1 and pc.points(31) == 91 and pc.points(40) == 91
    for nb in (1, 2, 5, 31):
        for q in range(pc.points(nb) + 1):
            f = pc.pfloor_of(nb, q)
            assert pc.q_of(nb, f) == q
            k, part = pc.decode_plan(f)
            if q >= 1:
                p, s = pc.split(q)
                assert (nb - k, part) == (p, s), (nb, q)
            # the header round trip: a block of nb planes cut at q
            if q >= 1:
                pf, numbps = pc.pfloor_from_header(31 - nb, q)
                assert (pf, numbps) == (f, nb)
                assert rc.floors_from_header(31 - nb, q) == (nb - pc.split(q)[0], nb)          # the older reader: p whole planes, s ignored


def test_sp_mask_model_equals_the_plain_loop():
    seen = 0
    for w, h, c, v, nb in _blocks():
        a, b = pc.sp_mask(v, nb), pc.sp_mask_direct(v, nb)
        assert np.array_equal(a, b), (w, h, c)
        assert not a[v == 0].any()
        seen += int(a.sum())
        words = pc.sp_words(a)
        assert words.shape == (64,) and not words[h:].any()
        for y in range(h):
            assert int(words[y]) == sum(1 << x for x in range(w) if a[y, x])
    assert seen > 100
    # a lone sample never has a significant neighbour; its right-hand and lower neighbours of a smaller magnitude do
    v = np.zeros((3, 3), np.int32); v[1, 1] = 8; v[1, 2] = 2; v[0, 0] = 1; v[2, 2] = 1
    sp = pc.sp_mask(v, 4)
    assert sp.tolist() == [[True, False, False], [False, False, True], [False, False, True]]


def test_coarse_pass_at_whole_planes_is_coarse():
    for w, h, c, v, nb in _blocks():
        sp = pc.sp_mask(v, nb)
        assert not pc.coarse_pass(v, nb, 0, sp).any()
        for p in range(1, nb + 1):
            assert np.array_equal(pc.coarse_pass(v, nb, 3 * p - 2, sp), cc.coarse(v, nb - p)), (w, h, c, p)
        if nb:
            assert np.array_equal(pc.coarse_pass(v, nb, pc.points(nb), sp), v)


def test_coarse_pass_inside_a_plane():
    """by hand: nb = 4; after plane 3 (q = 1) only the 8 is there; plane 2's SigProp (q = 2) visits the neighbours of the 8: the 5 turns, the 4 two
    columns away waits for Cleanup; its MagRef (q = 3) refines the 8 alone"""
    v = np.array([[13, -5, 0, 4]], np.int32)
    sp = pc.sp_mask(v, 4)
    assert sp.tolist() == [[False, True, False, False]]
    assert pc.coarse_pass(v, 4, 1, sp).tolist() == [[12, 0, 0, 0]]
    assert pc.coarse_pass(v, 4, 2, sp).tolist() == [[12, -6, 0, 0]]          # 13 still at floor 3, -5 at floor 2
    assert pc.coarse_pass(v, 4, 3, sp).tolist() == [[14, -6, 0, 0]]          # 13 refined to floor 2
    assert pc.coarse_pass(v, 4, 4, sp).tolist() == [[14, -6, 0, 6]]
    assert pc.floors_pass(v, 4, 2, sp).tolist() == [[3, 2, 3, 3]]


def test_distortion_ties_to_the_plane_tables_and_falls():
    for w, h, c, v, nb in _blocks():
        sp = pc.sp_mask(v, nb)
        D = pc.distortion_passes(v, nb, sp)
        assert len(D) == pc.points(nb) + 1 and D[-1] == 0
        D32 = rc.distortion(v, nb)
        for p in range(1, nb + 1):
            assert D[3 * p - 2] == D32[p], (w, h, c, p)
        assert D[0] == D32[0]
        if c != "deep":                                              # (no wrap below 2^64): SigProp and Cleanup only move samples closer -- a MagRef pass
            for p in range(1, nb):                                   # may move one away (a magnitude that sat on the coarser midpoint)
                assert D[3 * p - 2] >= D[3 * p - 1] and D[3 * p] >= D[3 * p + 1], (w, h, c, p)


def test_check_tables_accepts_and_refuses():
    R = np.zeros(96, np.uint32); D = np.zeros(96, np.uint64)
    R[1:] = 7; D[0] = 9
    pc.check_tables(R, D, 1, 7)
    R2 = R.copy(); R2[50] = 6
    with pytest.raises(AssertionError):
        pc.check_tables(R2, D, 1, 7)
    D2 = D.copy(); D2[1] = 1
    with pytest.raises(AssertionError):
        pc.check_tables(R, D2, 1, 7)


def test_allocation_runs_on_pass_tables():
    """rate_cases.allocate unchanged, the point count in nb's place: kept is a pass index, chosen <= budget, more budget never keeps less"""
    rng = np.random.default_rng(5)
    Rs, Ds, pts = [], [], []
    for j in range(12):
        nb = int(rng.integers(0, 9))
        last = pc.points(nb)
        R = np.zeros(96, np.int64); D = np.zeros(96, np.int64)
        steps = rng.integers(0, 40, last)
        steps[rng.random(last) < 0.4] = 0                           # empty passes: equal rates
        R[1:last + 1] = np.cumsum(steps)
        R[last:] = R[last]
        D[:last] = np.sort(rng.integers(1, 1 << 20, last))[::-1] if last else []
        Rs.append(R); Ds.append(D); pts.append(last)
    ws = [1.0] * 10 + [0.0, 2.5]
    total = sum(int(Rs[j][pts[j]]) for j in range(12))
    prev = None
    for budget in (0, 1, total // 10, total * 35 // 100, total * 8 // 10, total - 1, total, total + 1):
        kept, chosen = rc.allocate(Rs, Ds, pts, ws, budget)
        assert chosen <= budget
        assert all(0 <= kept[j] <= pts[j] for j in range(12))
        assert chosen == sum(int(Rs[j][kept[j]]) for j in range(12))
        if prev is not None:
            assert all(a <= b for a, b in zip(prev, kept))
        prev = kept
    assert prev == pts


NEW_SYMBOLS = (
    "j2k_plan_encode_blocks_passes", "j2k_plan_rate_allocate_passes", "j2k_plan_rate_allocate_quality_passes", "j2k_plan_encode_tile_parts_kept_passes",
    "j2k_plan_decode_tile_parts_pfloors", "j2k_plan_decode_blocks_pfloors", "j2k_plan_encode_frame_pixels_passes", "j2k_plan_decode_frame_pixels_passes",
    "j2k_encode_pixels_host_passes", "j2k_decode_pixels_host_passes",
)


def test_symbols_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "j2kgfx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from j2kgfx import _lib
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), "include/j2kgfx.h does not declare %s" % name
        assert name in _lib.SYMBOLS
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) >= 7, name
