"""CPU: the yardstick of the rate-limited MQ encode (tests/rate_cases.py) checked against itself -- distortions against a direct loop, the
hull and the bisection on hand-made tables (equal slopes, no more bytes, distortion that rises again), the budget, monotony in the budget,
optimality against brute force, the packet-header rule for floors, the default weights against impulse energies -- and the new names in
the header, the library's symbol list and the binding."""
import itertools
import os
import re

import numpy as np
import pytest

import coarse_cases as cc
import rate_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("j2k_plan_encode_blocks_planes", "j2k_plan_rate_allocate", "j2k_plan_get_rate_weights", "j2k_plan_set_rate_weights")


# ---- distortion ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,sparse", [(1, False), (4, False), (8, True), (16, False), (31, True)])
def test_distortion_against_direct_loop(bits, sparse):
    rng = np.random.default_rng(bits)
    v = cc.samples(rng, 9, 7, bits, sparse)
    D = rc.distortion(v, bits)
    assert D == rc.distortion_direct(v, bits)
    assert D[bits] == 0 and len(D) == bits + 1
    if bits < 31:                                                    # no wrap below 2^64: keeping nothing costs the block's energy
        assert D[0] == int((v.astype(np.int64) ** 2).sum())


def test_distortion_wraps_like_numpy():
    v = np.full((64, 64), (1 << 31) - 1, np.int32)                   # 4096 * (2^31 - 1)^2 > 2^64
    D = rc.distortion(v, 31)
    assert D[0] == (4096 * ((1 << 31) - 1) ** 2) & rc.MASK64 and D == rc.distortion_direct(v, 31)


# ---- hull ---------------------------------------------------------------------------------------------------------------------------------
def test_hull_plain_convex():
    pts, sl = rc.hull([0, 10, 20, 40], [1000, 400, 100, 0], 3, 1.0)
    assert pts == [0, 1, 2, 3] and sl[1:] == [60.0, 30.0, 5.0]


def test_hull_equal_slopes_pop_the_middle():
    pts, sl = rc.hull([0, 10, 20], [200, 100, 0], 2, 1.0)
    assert pts == [0, 2] and sl[1:] == [10.0]


def test_hull_concave_point_is_skipped():
    pts, _ = rc.hull([0, 10, 11, 30], [1000, 900, 100, 0], 3, 1.0)
    assert pts == [0, 2, 3]


def test_hull_no_more_bytes_replaces_predecessor():
    pts, sl = rc.hull([0, 10, 10, 30], [1000, 500, 400, 0], 3, 2.0)
    assert pts == [0, 2, 3] and sl[1:] == [2.0 * 600 / 10, 2.0 * 400 / 20]
    pts, sl = rc.hull([0, 0, 8], [50, 40, 0], 2, 1.0)                # ... the start itself
    assert pts == [1, 2] and sl[1:] == [5.0]


def test_hull_rising_distortion_is_never_a_point():
    pts, _ = rc.hull([0, 5, 9, 12], [100, 120, 100, 0], 3, 1.0)
    assert pts == [0, 3]
    pts, _ = rc.hull([0, 5, 9], [100, 40, 60], 2, 1.0)
    assert pts == [0, 1]


def test_hull_zero_weight():
    pts, sl = rc.hull([0, 5, 9], [100, 40, 0], 2, 0.0)
    assert pts == [0, 2] and sl[1:] == [0.0]


def test_pick():
    h = rc.hull([0, 10, 20, 40], [1000, 400, 100, 0], 3, 1.0)
    assert [rc.pick(h, lam) for lam in (0.0, 5.0, 5.5, 30.0, 60.0, 61.0, float("inf"), float("nan"))] == [3, 3, 2, 2, 1, 0, 0, 0]


# ---- allocation ---------------------------------------------------------------------------------------------------------------------------
def _random_tables(rng, n, maxnb=6):
    Rs, Ds, nbs, ws = [], [], [], []
    for _ in range(n):
        nb = int(rng.integers(0, maxnb + 1))
        R = np.concatenate([[0], np.cumsum(rng.integers(0, 40, nb))]).astype(np.int64)
        D = np.sort(rng.integers(0, 5000, nb + 1))[::-1].astype(np.int64)
        D[nb] = 0
        if nb >= 3 and rng.random() < 0.3:
            D[1] = D[0] + 7                                          # distortion that rises first
        Rs.append([int(x) for x in R]); Ds.append([int(x) for x in D]); nbs.append(nb)
        ws.append(float(rng.choice([0.25, 1.0, 1.0, 3.5])))
    return Rs, Ds, nbs, ws


def test_nothing_cut_when_it_fits():
    Rs, Ds, nbs, ws = _random_tables(np.random.default_rng(3), 20)
    total = sum(R[nb] for R, nb in zip(Rs, nbs))
    for budget in (total, total + 1, 10 * total):
        assert rc.allocate(Rs, Ds, nbs, ws, budget) == (nbs, total)


def test_budget_respected_and_monotone():
    Rs, Ds, nbs, ws = _random_tables(np.random.default_rng(4), 40)
    total = sum(R[nb] for R, nb in zip(Rs, nbs))
    last = -1
    for budget in sorted({0, 1, total // 10, total // 3, total // 2, total - 1, total}):
        ps, b = rc.allocate(Rs, Ds, nbs, ws, budget)
        assert b <= budget and b == sum(Rs[j][ps[j]] for j in range(len(ps)))
        assert all(0 <= p <= nb for p, nb in zip(ps, nbs))
        assert b >= last
        last = b
    assert rc.allocate(Rs, Ds, nbs, ws, 0)[1] == 0


def test_lambda_is_the_smallest_that_fits():
    """one block, hull slopes 60 / 30 / 5: a budget of 25 bytes admits the point at 20 bytes, so lam* is the first double above 5"""
    ps, b = rc.allocate([[0, 10, 20, 40]], [[1000, 400, 100, 0]], [3], [1.0], 25)
    assert (ps, b) == ([2], 20)
    assert rc.allocate([[0, 10, 20, 40]], [[1000, 400, 100, 0]], [3], [1.0], 19) == ([1], 10)
    assert rc.allocate([[0, 10, 20, 40]], [[1000, 400, 100, 0]], [3], [1.0], 9) == ([0], 0)


@pytest.mark.parametrize("seed", range(12))
def test_brute_force_three_blocks(seed):
    """3 blocks x <= 4 points: no combination with at most the chosen bytes has a lower weighted distortion"""
    Rs, Ds, nbs, ws = _random_tables(np.random.default_rng(100 + seed), 3, maxnb=3)
    total = sum(R[nb] for R, nb in zip(Rs, nbs))
    for budget in range(0, total + 2, max(1, total // 9)):
        ps, b = rc.allocate(Rs, Ds, nbs, ws, budget)
        mine = rc.weighted_distortion(Ds, ws, ps)
        for combo in itertools.product(*[range(nb + 1) for nb in nbs]):
            if sum(Rs[j][combo[j]] for j in range(3)) <= b:
                assert rc.weighted_distortion(Ds, ws, combo) >= mine, (budget, ps, combo)


# ---- packet headers -----------------------------------------------------------------------------------------------------------------------
def test_floors_from_header():
    for nb in range(0, 32):
        for p in range(0, nb + 1):
            floor, numbps = rc.floors_from_header(31 - nb, rc.passes_of(p))
            if p == 0:
                assert numbps == floor                               # nothing coded: the block is zeros whatever the floor
            else:
                assert (floor, numbps) == (nb - p, nb)
    assert rc.floors_from_header(31, 5) == (0, 2)                    # an inconsistent header: more passes than planes -- the floor stays >= 0
    assert rc.passes_of(0) == 0 and rc.passes_of(1) == 1 and rc.passes_of(4) == 10


# ---- weights ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lossless", [True, False], ids=["53", "97"])
def test_default_weights_against_impulse_energies(lossless):
    """an impulse of 2^24 in the middle of every band of a 3-level Mallat plane through the inverse: its energy over 2^48 is the band's weight
    within 1e-2 (integer lifting rounds by < 1 per sample and step: below 1e-3 of the energy; neighbouring bands differ by factors near 2)"""
    import oracle as orc
    W, H, L = 128, 96, 3
    w = rc.default_weights(1, L + 1, lossless)
    assert w.shape == (1, L + 1, 4)
    for res in range(L + 1):
        for band in ((0,) if res == 0 else (1, 2, 3)):
            e = rc.impulse_energy(orc, W, H, L, res, band, lossless)
            assert abs(e - w[0, res, band]) <= 1e-2 * e, (res, band, e, w[0, res, band])
    assert np.all(rc.default_weights(3, 4, lossless, mallat=False) == 1.0)


def test_band_rects_partition_the_plane():
    W, H, L = 130, 70, 3
    seen = np.zeros((H, W), np.int32)
    for res in range(L + 1):
        for band in ((0,) if res == 0 else (1, 2, 3)):
            x0, y0, bw, bh = rc.band_rect(W, H, L, res, band)
            seen[y0:y0 + bh, x0:x0 + bw] += 1
    assert np.all(seen == 1)


# ---- the prefix property on the oracle's own encoder: the whole codeword and nothing ---------------------------------------------------------
def test_prefix_property_ends():
    import oracle as orc
    rng = np.random.default_rng(9)
    v = cc.samples(rng, 17, 5, 8)
    data, nb = orc.t1_encode(v, 17, 5, 1)
    assert nb == 8
    assert rc.prefix_ok(orc, data, len(data), nb, 1, v, nb)
    assert rc.prefix_ok(orc, data, 0, nb, 1, v, 0)
    assert not rc.prefix_ok(orc, data, 1, nb, 1, v, nb)


# ---- names --------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "j2kgfx.h")).read()
    libpy = open(os.path.join(ROOT, "go-jpeg2000_amd", "j2kgfx", "_lib.py")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert '"%s"' % s in libpy, s
