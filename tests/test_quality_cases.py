"""CPU: the properties of tests/quality_cases.py, the definition of the quality-targeted MQ encode -- the fixed-order float64 sum, the
bisection on the distortion sum, its duality with rate_cases.allocate, monotonicity, the boundary cases."""
import math

import numpy as np
import pytest

import layer_cases as lc
import quality_cases as qc
import rate_cases as rc


@pytest.fixture(scope="module")
def tables():
    return {s: qc.random_tables(*s) for s in qc.TABLE_SETS}


def _total(Rs, nbs):
    return sum(int(R[nb]) for R, nb in zip(Rs, nbs))


def _start_sum(Ds, nbs, ws, Rs):
    H = qc.Hulls(Rs, Ds, nbs, ws)
    return H.choice((1 << 63) - 1)


def test_sum_order():
    """the numpy sum is the lane-by-lane one, and the order is observable: float64 terms of mixed size do not add up the same in index order"""
    rng = np.random.default_rng(11)
    differs = False
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 2500):
        t = rng.integers(0, 1 << 62, n).astype(np.float64) * rng.choice([1.0, 0.5316, 1.9657], n)
        s = qc.wg_sum_f64(t)
        assert qc.float_bits(s) == qc.float_bits(qc.wg_sum_f64_plain(list(t)))
        assert s == pytest.approx(math.fsum(t), rel=1e-12)
        plain = 0.0
        for x in t:
            plain = plain + float(x)
        differs |= qc.float_bits(plain) != qc.float_bits(s)
    assert differs, "vacuous: no term set tells the order from a plain loop"
    assert qc.wg_sum_f64([]) == 0.0


def test_vector_choice_is_picks_choice(tables):
    """Hulls.choice (slopes counted with numpy) = rate_cases.pick block by block, at patterns around every kind of lambda"""
    for key in ((1, 10), (3, 144), (6, 1203)):
        Rs, Ds, nbs, ws = tables[key]
        H = qc.Hulls(Rs, Ds, nbs, ws)
        slopes = sorted({float(s) for _, sl in H.hulls for s in sl[1:]})
        pats = [0, 1, (1 << 63) - 1, 0x7FF0000000000000, 0x7FF0000000000001]
        for s in slopes[:: max(1, len(slopes) // 12)]:
            b = qc.float_bits(s)
            pats += [b - 1, b, b + 1] if b else [b, b + 1]
        for b in pats:
            a, c = H.choice(b), H.choice_plain(b, Rs, Ds, ws)
            assert a[0] == c[0] and a[1] == c[1] and qc.float_bits(a[2]) == qc.float_bits(c[2]), hex(b)


def test_plain_search_agrees():
    Rs, Ds, nbs, ws = qc.random_tables(21, 70)
    _, _, s0 = _start_sum(Ds, nbs, ws, Rs)
    for T in (0.0, s0 / 7, s0 / 2, s0, s0 * 2):
        a, b = qc.allocate_quality(Rs, Ds, nbs, ws, T), qc.allocate_quality_plain(Rs, Ds, nbs, ws, T)
        assert a[0] == b[0] and a[1] == b[1] and qc.float_bits(a[2]) == qc.float_bits(b[2])


@pytest.mark.parametrize("key", qc.TABLE_SETS, ids=lambda k: "n%d" % k[1])
def test_duality_with_rate_allocate(tables, key):
    """for every byte budget B that cuts: T := S(allocate(B)) gives the same S, no more bytes, and the identical cuts"""
    Rs, Ds, nbs, ws = tables[key]
    total = _total(Rs, nbs)
    cut = 0
    for f in (0.0, 0.03, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99):
        B = int(total * f)
        ps, bytes_b = rc.allocate(Rs, Ds, nbs, ws, B)
        if ps == [int(nb) for nb in nbs]:
            continue
        cut += 1
        T = qc.weighted_distortion(Ds, ws, ps)
        qs, bytes_q, S = qc.allocate_quality(Rs, Ds, nbs, ws, T)
        assert qc.float_bits(S) == qc.float_bits(T), f
        assert bytes_q <= bytes_b <= B, f
        assert qs == ps, f
    assert cut >= 6


def test_monotone_in_target(tables):
    """a smaller target: no fewer bytes, no more distortion, no block keeps fewer planes"""
    for key in ((2, 63), (6, 1203)):
        Rs, Ds, nbs, ws = tables[key]
        _, _, s0 = _start_sum(Ds, nbs, ws, Rs)
        last = None
        for f in (2.0, 1.0, 0.5, 0.1, 0.01, 1e-4, 1e-8, 0.0):
            ps, b, S = qc.allocate_quality(Rs, Ds, nbs, ws, s0 * f)
            assert S <= s0 * f
            if last:
                assert b >= last[1] and S <= last[2] and all(p >= q for p, q in zip(ps, last[0])), f
            last = (ps, b, S)
        assert last[1] > 0


def test_layers_monotone_and_normalise(tables):
    Rs, Ds, nbs, ws = tables[(3, 144)]
    _, _, s0 = _start_sum(Ds, nbs, ws, Rs)
    targets = [s0 * 2.0 ** -l for l in range(qc.MAX_LAYERS)]
    kept, chosen, achieved = qc.allocate_quality_layers(Rs, Ds, nbs, ws, targets)
    assert len(kept) == 32 and chosen == sorted(chosen) and achieved == sorted(achieved, reverse=True)
    assert all(a <= t for a, t in zip(achieved, targets))
    for l, T in enumerate(targets):
        assert kept[l] == qc.allocate_quality(Rs, Ds, nbs, ws, T)[0]
    for j in range(len(nbs)):                           # the cuts feed the layer normalisation as byte-budget cuts do
        Q = lc.normalise(Rs[j], [kept[l][j] for l in range(32)])
        assert Q == sorted(Q) and Q[-1] <= nbs[j]
    with pytest.raises(AssertionError):
        qc.allocate_quality_layers(Rs, Ds, nbs, ws, [1.0, 2.0])
    with pytest.raises(AssertionError):
        qc.allocate_quality_layers(Rs, Ds, nbs, ws, [0.0] * 33)


def test_target_zero_and_large(tables):
    """T = 0: every plane of every block of positive weight that lowers its distortion, a weight-0 block dropped entirely; a target at or
    above the start-point sum: the start points; +inf and negative targets are refused"""
    for key in ((1, 10), (5, 1152)):
        Rs, Ds, nbs, ws = tables[key]
        ps, b, S = qc.allocate_quality(Rs, Ds, nbs, ws, 0.0)
        assert S == 0.0
        assert any(w == 0.0 and nb > 0 for w, nb in zip(ws, nbs)) or key == (1, 10)
        for j, (p, nb, w) in enumerate(zip(ps, nbs, ws)):
            if w == 0.0:                                # (its start point: plane 0, or a later one that costs no byte)
                assert int(Rs[j][p]) == 0 and p == rc.hull(list(map(int, Rs[j])), list(map(int, Ds[j])), nb, w)[0][0], j
            else:
                assert int(Ds[j][p]) == 0 and (p == nb or int(Ds[j][p]) == int(Ds[j][nb])), j
        ps0, b0, s0 = _start_sum(Ds, nbs, ws, Rs)
        for T in (s0, s0 * 4, 1e300):
            qs, bq, Sq = qc.allocate_quality(Rs, Ds, nbs, ws, T)
            assert qs == ps0 and bq == b0 and qc.float_bits(Sq) == qc.float_bits(s0)
        below = float(np.nextafter(s0, 0.0))
        assert qc.allocate_quality(Rs, Ds, nbs, ws, below)[2] < s0
        for bad in (float("inf"), -1.0, float("nan")):
            with pytest.raises(AssertionError):
                qc.allocate_quality(Rs, Ds, nbs, ws, bad)


def test_boundary_is_inclusive(tables):
    """T exactly an attainable S is met with that S; the float64 just below it is not"""
    Rs, Ds, nbs, ws = tables[(4, 700)]
    H = qc.Hulls(Rs, Ds, nbs, ws)
    slopes = sorted({float(s) for _, sl in H.hulls for s in sl[1:] if s > 0.0})
    seen = 0
    for s in slopes[:: len(slopes) // 9]:
        ps, b, S = H.choice(qc.float_bits(s))
        if S == 0.0:
            continue
        got = qc.allocate_quality(Rs, Ds, nbs, ws, S)
        assert qc.float_bits(got[2]) == qc.float_bits(S) and got[0] == ps
        under = qc.allocate_quality(Rs, Ds, nbs, ws, float(np.nextafter(S, 0.0)))
        assert under[2] < S and under[1] >= b
        seen += 1
    assert seen >= 5


def test_distortions_near_2_63():
    """uint64 -> float64 rounds above 2^53: the term is float(w) * float(D) with D converted once, round to nearest even"""
    assert qc.term(1.0, (1 << 63) - 1) == 2.0 ** 63 and qc.term(1.0, (1 << 63) - 1025) == 2.0 ** 63 - 1024.0
    assert qc.term(1.0, (1 << 63) - 1536) == 2.0 ** 63 - 2048.0 and qc.term(1.0, (1 << 63) - 1535) == 2.0 ** 63 - 1024.0      # the tie goes to even
    assert qc.term(1.0, (1 << 53) + 1) == 2.0 ** 53 and qc.term(1.0, (1 << 53) + 3) == 2.0 ** 53 + 4.0
    assert qc.term(1.0, np.uint64((1 << 64) - 1)) == 2.0 ** 64
    for seed, n in ((31, 40), (32, 1100)):
        Rs, Ds, nbs, ws = qc.random_tables(seed, n, big=True)
        assert max(int(D[0]) for D in Ds) > (1 << 63) - (1 << 21)
        total = _total(Rs, nbs)
        for f in (0.2, 0.6):
            ps, bytes_b = rc.allocate(Rs, Ds, nbs, ws, int(total * f))
            T = qc.weighted_distortion(Ds, ws, ps)
            qs, bq, S = qc.allocate_quality(Rs, Ds, nbs, ws, T)
            assert qs == ps and bq <= bytes_b and qc.float_bits(S) == qc.float_bits(T)
        a = qc.allocate_quality(Rs, Ds, nbs, ws, 0.0)
        assert a[2] == 0.0


def test_psnr_distortion():
    """T = N peak^2 q^2 / 10^(dB / 10): 8-bit RGB 64 x 48 lossless at 20 log10(255) dB is one unit of squared error per sample"""
    assert qc.psnr_distortion(64, 48, 3, 8, True, 0, 20 * math.log10(255.0)) == pytest.approx(64 * 48 * 3, rel=1e-12)
    assert qc.psnr_distortion(64, 48, 3, 8, False, 20, 40.0) == pytest.approx(400 * qc.psnr_distortion(64, 48, 3, 8, True, 0, 40.0), rel=1e-12)
    assert qc.psnr_distortion(10, 10, 1, 16, True, 0, 0.0) == 100.0 * 65535.0 ** 2
    assert qc.psnr(0, 100, 255) == float("inf") and qc.psnr(100, 100, 255) == pytest.approx(20 * math.log10(255.0))
