"""CPU: the case lists of tests/lossy97_cases.py before the GPU sees them (tests/test_gpu_lossy97_oracle.py).

* The C oracle and oracle/pyref.py agree bit for bit on every float64 case (pyref.forward97 / inverse97, the literal restatement of
  dwt.go:161-262, over whole rows and columns at a time; pyref.decompose97 / reconstruct97 themselves on the planes small enough for the
  scalar walk), on every `outrange` forward frame and on every other forward tile of 3000 samples and fewer (pyref.preprocess is a scalar
  walk: the forward comparison is partial, 489 of 822 tiles): two independent restatements, so a case on which they differed would be a
  finding about the oracle, not about a kernel.
* Each family does what its name says.  The reference's conversions are restated in numpy on the oracle's float64 results only to COUNT
  the ones that take Go's out-of-range int32(float64); the restatement's integers are asserted equal to the oracle's own on every case.

Counts (printed by the tests; -s shows them):
  forward cases 216 (x families = 724 frames, 489 tiles of them also through pyref.preprocess), inverse cases 160 (x families = 422
      coefficient sets), float64 planes 63 shapes x 4 families (24 shapes also through pyref's scalar multi-level calls) and 13 lengths
  forward `outrange` frames 64: 8 ... 9808 out-of-range conversions per frame, 5 ... 36 rows without one, 4 conversions per frame whose
      rounded sum is 2^31 exactly (the Cr samples built for it)
  inverse `outrange` tiles 119: 24 ... 125 out-of-range conversions per tile, 7 ... 36 output rows without one (the inverse has no sum of
      exactly 2^31: its conversions follow the lifting steps, whose results no input pins to half an integer)
  `huge`: every output of the oracle finite; `subnormal`: 16 ... 16782 subnormal non-zero outputs per plane and call;
  `overflow`: a non-finite output in every plane of two samples and more; +-inf in 225 and NaN (inf - inf) in 251 of the 252 (plane, call)
This file found oracle/pyref.py returning the low 32 bits of a wider integer for an out-of-range int32(float64) (pyref._trunc32) where Go on
amd64 -- and the C oracle -- give 0x80000000; `nw0-16x19-t0x0-p16-r6-q4097` `outrange` is the case that showed it."""
import numpy as np
import pytest

import lossy97_cases as lc
import pyref


def _frames(case, family, seed=1):
    """[(x0, y0, crop [3, h, w])] of the frame a forward case encodes"""
    nrs = (case.nw - 3, lc.defaults()["band_prows_97"])
    frame = lc.int_frame(family, case.W, case.H, 3, case.prec, seed, nrs)
    return frame, [(x0, y0, np.ascontiguousarray(frame[:, y0:y0 + h, x0:x0 + w])) for x0, y0, w, h in lc.tiles_of(case.W, case.H, case.tile)]


def test_shape_sets_follow_the_code():
    d = lc.defaults()
    assert set(d) == {"l0_wg97", "l0_wg97_inv", "plane_wg97", "band_prows_97"} and all(v > 0 for v in d.values())
    assert d["l0_wg97"] in lc.FWD_WAVES and d["l0_wg97_inv"] in lc.INV_WAVES and d["plane_wg97"] in lc.PLANE_WAVES
    ws = lc.march_widths()
    for s in (124, 128, 248, 252, 256, 504, 508):          # the advance and the strip width of both marching forms, and twice / four times
        assert {s - 1, s, s + 1, s + 2} <= set(ws)
    assert {w for w, _ in lc.march_shapes()} == set(ws)
    hs = lc.march_heights()
    b = d["band_prows_97"]
    assert set(hs) == {1, 2, 3, 2 * b - 1, 2 * b, 2 * b + 1, 4 * b - 1, 4 * b, 4 * b + 1}
    for h in hs:
        assert sum(1 for _, hh in lc.march_shapes() if hh == h) >= 3
    for nw in set(lc.FWD_WAVES + lc.INV_WAVES + lc.PLANE_WAVES) - {0}:
        nr = nw - 3
        halves = {(h + 1) // 2: set() for _, h in lc.wg_shapes(nw)}
        for _, h in lc.wg_shapes(nw):
            halves[(h + 1) // 2].add(h & 1)
        assert set(halves) == {1, 2, nr - 1, nr, nr + 1, 2 * nr, 2 * nr + 1}
        assert all(p == {0, 1} for p in halves.values())                       # both parities of h
        assert {w for w, _ in lc.wg_shapes(nw)} == set(lc.WG_WIDTHS)
    for w, h in lc.float_shapes():
        assert w * h <= 800 * 80
    # every width of a form meets every quality, precision and resolution count somewhere
    for nw in lc.FWD_WAVES:
        cs = [c for c in lc.forward_cases() if c.nw == nw]
        assert {c.quality for c in cs} == set(lc.QUALITIES) and {c.prec for c in cs} == set(lc.PRECISIONS) and {c.nres for c in cs} == set(lc.NRES)
        assert all(sum(1 for c in cs if c.quality == q) >= 3 for q in lc.QUALITIES)
    for nw in lc.INV_WAVES:
        cs = [c for c in lc.inverse_cases() if c.nw == nw]
        assert {(c.prec, c.nres) for c in cs} == {(p, r) for p in lc.PRECISIONS for r in lc.NRES}
    assert sum("outrange" in c.families for c in lc.forward_cases() if c.nw not in (0, d["l0_wg97"])) > 0
    # a case for a workgroup width is a frame the form admits: no width quietly runs the marching kernels instead
    for c in lc.forward_cases() + lc.inverse_cases():
        assert not c.nw or lc.wg_admitted(c.W, c.H, c.tile), c.id
    assert not lc.wg_admitted(520, 13, (256, 128)) and not lc.wg_admitted(24, 1, (0, 0)) and lc.wg_admitted(536, 13, (256, 128))
    # the same seed gives the same case
    assert np.array_equal(lc.int_frame("outrange", 24, 12, 3, 12, 5), lc.int_frame("outrange", 24, 12, 3, 12, 5))
    assert lc.same_floats(lc.float_plane("overflow", 24, 12, 5), lc.float_plane("overflow", 24, 12, 5))


def test_int_families_are_what_they_say():
    w, h, prec = 504, 33, 12
    top, mid = (1 << prec) - 1, 1 << (prec - 1)
    nrs = (5, 8)
    f = lc.int_frame("impulse", w, h, 3, prec, 0, nrs)
    nz = np.argwhere((f != mid).any(axis=0))
    assert {tuple(p) for p in nz} == set(lc.impulse_points(w, h, nrs))
    assert ((f != mid).sum(axis=0) <= 1).all()                                 # one component per point
    pts = set(lc.impulse_points(w, h, nrs))
    assert {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)} <= pts
    for c in (123, 124, 247, 248, 251, 252, 255, 256, 371, 372, 495, 496, 503):
        assert any(x == c for _, x in pts), c
    for r in (9, 10, 15, 16, 19, 20, 29, 30, 31, 32):                            # 2 * 5 k and 2 * 8 k, and the row before
        assert any(y == r for y, _ in pts), r
    s = lc.int_frame("step", w, h, 3, prec)
    assert set(np.unique(s)) == {0, top} and (s[0][:, :w // 2] == 0).all() and (s[0][:, w // 2:] == top).all()
    assert (s[1][:h // 2] == 0).all() and (s[1][h // 2:] == top).all()
    assert (lc.int_frame("const", w, h, 3, prec) == top).all()
    c = lc.int_frame("checker", w, h, 3, prec)
    assert (c[0][::2, ::2] == 0).all() and (c[0][::2, 1::2] == top).all() and (c[0] + c[1] == top).all()
    o = lc.int_frame("outrange", w, h, 3, prec)
    assert ((o[:, [0] + list(range(2, h))] >= 0) & (o[:, [0] + list(range(2, h))] <= top)).all()
    assert (o[:, 1] == 2 ** 31 - 1).any() and (o[:, 1] == -2 ** 31).any()
    k = lc.coeff_plane("outrange", w, h)
    r0 = (h + 1) // 2
    assert np.abs(np.delete(k, r0, axis=0).astype(np.int64)).max() <= 1 << 12
    assert (k[r0] == 2 ** 31 - 1).any() and (k[r0] == -2 ** 31).any()
    ki = lc.coeff_plane("impulse", w, h, 0, nrs)
    assert {tuple(p) for p in np.argwhere(ki)} == pts


def test_forward_cases_oracle_pyref_and_outrange_counts(oracle):
    """oracle.preprocess == the counting restatement on every forward case and family; == pyref.preprocess on the small tiles; what `outrange`
    reaches"""
    cases = lc.forward_cases()
    nframes = npy = 0
    oor, clean, exact = [], [], []
    for case in cases:
        for family in case.families:
            nframes += 1
            _, crops = _frames(case, family)
            for x0, y0, crop in crops:
                _, h, w = crop.shape
                want = np.stack(oracle.preprocess([crop[c] for c in range(3)], w, h, case.prec, False, case.nres, case.quality))
                got, rows, ex = lc.forward_counts(oracle, crop, case.prec, case.nres, case.quality)
                assert np.array_equal(got, want), (case.id, family, x0, y0)
                if family == "outrange":
                    assert len(crops) == 1
                    assert rows.sum() >= 1, (case.id, "no conversion leaves int32")
                    assert (rows == 0).any(), (case.id, "no row keeps the fast path")
                    assert ex >= 1, (case.id, "no rounded sum of exactly 2^31")
                    oor.append(int(rows.sum())); clean.append(int((rows == 0).sum())); exact.append(ex)
                elif case.prec <= 16 and case.quality < 8192:
                    assert rows.sum() == 0, (case.id, family)               # the plan's claim for samples inside the precision
                if family == "outrange" or w * h <= 3000:                   # every `outrange` frame; the others where the scalar walk stays quick
                    npy += 1
                    py = pyref.preprocess([crop[c].reshape(-1).tolist() for c in range(3)], w, h, case.prec, False, case.nres, case.quality)
                    assert np.array_equal(np.array(py, np.int64).reshape(3, h, w), want), (case.id, family, "pyref")
    print("forward cases %d, frames %d (pyref.preprocess on %d tiles); outrange frames %d: out-of-range conversions %d ... %d, clean rows %d ... %d, "
          "sums of exactly 2^31 %d ... %d" % (len(cases), nframes, npy, len(oor), min(oor), max(oor), min(clean), max(clean), min(exact), max(exact)))
    assert len(oor) >= 40 and npy >= 400


@pytest.mark.parametrize("quality,seed", lc.MARKSTEIN_FRAMES)
def test_markstein_frames_need_the_correction(oracle, quality, seed):
    """on each frame the uncorrected product v * RN(1 / step) rounds to another integer than the reference's v / step somewhere, and
    oracle.preprocess is the true division's"""
    W, H, prec, nres = lc.MARKSTEIN_SHAPE
    frame = lc.markstein_frame(quality, seed)
    want = np.stack(oracle.preprocess([frame[c] for c in range(3)], W, H, prec, False, nres, quality))
    got, rows, _ = lc.forward_counts(oracle, frame, prec, nres, quality)
    assert np.array_equal(got, want) and rows.sum() == 0
    step = 1.0 / quality
    rstep = 1.0 / step
    s = np.stack([oracle.dc_shift_fwd(frame[c].reshape(-1), prec).reshape(H, W) for c in range(3)])
    y = oracle.ict_fwd(*[s[c].astype(np.float64).reshape(-1) for c in range(3)])
    differ = 0
    for c in range(3):
        f = oracle.decompose97(lc.round_half_away(y[c].reshape(H, W))[0].astype(np.float64), W, H, 1)
        assert np.array_equal(lc.round_half_away(f / step)[0], want[c])
        differ += int(np.count_nonzero(lc.round_half_away(f * rstep)[0] != want[c]))
    assert differ >= 1


def test_inverse_cases_counting_restatement_and_outrange_counts(oracle):
    """the decode-side composition (tcd.ApplyInverseDWT, InverseICT, DC shift) == the counting restatement on every inverse case and family;
    what `outrange` reaches"""
    cases = lc.inverse_cases()
    nsets = 0
    oor, clean = [], []
    for case in cases:
        nrs = (case.nw - 3, lc.defaults()["band_prows_97"])
        for family in case.families:
            nsets += 1
            for x0, y0, w, h in lc.tiles_of(case.W, case.H, case.tile):
                coefs = np.stack([lc.coeff_plane(family, w, h, 3 * (x0 + y0) + c, nrs) for c in range(3)])
                want = lc.expect_inverse(oracle, coefs, case.prec, case.nres)
                got, rows = lc.inverse_counts(oracle, coefs, case.prec, case.nres)
                assert np.array_equal(got, want), (case.id, family, x0, y0)
                if family == "outrange" and h >= lc.OUTRANGE_MIN_H:
                    assert rows.sum() >= 1, (case.id, "no conversion leaves int32")
                    assert (rows == 0).any(), (case.id, "no row keeps the fast path")
                    oor.append(int(rows.sum())); clean.append(int((rows == 0).sum()))
                elif family != "outrange":
                    assert rows.sum() == 0, (case.id, family)
    print("inverse cases %d, coefficient sets %d; outrange tiles %d: out-of-range conversions %d ... %d, clean rows %d ... %d"
          % (len(cases), nsets, len(oor), min(oor), max(oor), min(clean), max(clean)))
    assert len(oor) >= 60


def _subnormal_count(a):
    a = np.abs(np.asarray(a, np.float64))
    return int(np.count_nonzero((a > 0) & (a < 2.0 ** -1022)))


@pytest.mark.parametrize("family", lc.FLOAT_FAMILIES)
def test_float_cases_oracle_vs_pyref(oracle, family):
    """dwt.Forward2D97 / Inverse2D97 / DecomposeMultiLevel97 / ReconstructMultiLevel97 (levels 1 and 3) and Forward97 / Inverse97: C oracle ==
    pyref, bit patterns and NaN-ness, on every shape; the family's own property on the oracle's output"""
    sub, infs, nans, scalar = [], 0, 0, 0
    with np.errstate(all="ignore"):
        for w, h in lc.float_shapes():
            x = lc.float_plane(family, w, h)
            assert not np.isnan(x).any()
            outs = {"fwd": oracle.fwd97_2d(x, w, h), "inv": oracle.inv97_2d(x, w, h),
                    "dec3": oracle.decompose97(x, w, h, 3), "rec3": oracle.reconstruct97(x, w, h, 3)}
            assert lc.same_floats(outs["fwd"], oracle.decompose97(x, w, h, 1)) and lc.same_floats(outs["inv"], oracle.reconstruct97(x, w, h, 1))
            assert lc.same_floats(outs["fwd"], lc.pyref_2d(pyref, x, w, h, False)), (w, h, "Forward2D97")
            assert lc.same_floats(outs["inv"], lc.pyref_2d(pyref, x, w, h, True)), (w, h, "Inverse2D97")
            assert lc.same_floats(outs["dec3"], lc.pyref_multilevel(pyref, x, w, h, 3, False)), (w, h, "DecomposeMultiLevel97")
            assert lc.same_floats(outs["rec3"], lc.pyref_multilevel(pyref, x, w, h, 3, True)), (w, h, "ReconstructMultiLevel97")
            if w * h <= 800:                                                   # pyref's own entry points, the scalar walk
                scalar += 1
                d = x.tolist(); pyref.decompose97(d, w, h, 3)
                assert lc.same_floats(outs["dec3"], d)
                d = x.tolist(); pyref.reconstruct97(d, w, h, 3)
                assert lc.same_floats(outs["rec3"], d)
            for name, o in outs.items():
                if family == "huge":
                    assert np.isfinite(o).all(), (w, h, name)
                if family == "subnormal":
                    n = _subnormal_count(o)
                    assert n >= 1, (w, h, name)
                    sub.append(n)
                if family == "overflow" and w * h >= 2:
                    assert not np.isfinite(o).all(), (w, h, name)                # +-inf, or NaN where two of them met
                    infs += int(np.isinf(o).any())
                    nans += int(np.isnan(o).any())
                if family == "noise":
                    assert np.isfinite(o).all()
        for n in lc.LENGTHS_1D:
            x = lc.float_plane(family, n, 1)
            f, i = oracle.fwd97_1d(x), oracle.inv97_1d(x)
            d = x.tolist(); pyref.forward97(d, n)
            assert lc.same_floats(f, d), (n, "Forward97")
            d = x.tolist(); pyref.inverse97(d, n)
            assert lc.same_floats(i, d), (n, "Inverse97")
            if family == "huge":
                assert np.isfinite(f).all() and np.isfinite(i).all()
            if family == "overflow" and n >= 2:
                assert not np.isfinite(f).all() and not np.isfinite(i).all()
    print("%s: %d shapes (%d also through pyref's scalar multi-level calls), %d lengths; subnormal outputs per plane %s; planes with inf %d, with NaN %d"
          % (family, len(lc.float_shapes()), scalar, len(lc.LENGTHS_1D), (min(sub), max(sub)) if sub else "-", infs, nans))
    if family == "overflow":
        assert nans >= 10 and infs >= 10                                                       # inf - inf arises, and both sides must say so
