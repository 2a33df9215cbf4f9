"""CPU: the definition of tests/signed_cases.py checked on the oracle alone, before tests/test_gpu_signed.py holds the device against it.

  the oracle's flag      postprocess(is_signed=True) == postprocess(is_signed=False) - 2^(prec - 1) in wrapping int32, on every case and family
  the case lists         every inverse form label the generators of lossless53_cases / lossy97_cases can produce has a signed case: a new kernel
                         form without a signed case fails here
  signedrange            a condition on the INPUTS of the pixel tests, not a measurement: at least 30 % of the signed reconstruction clamps to 0 and
                         at least 30 % lies strictly between 0 and maxVal, per precision"""
import numpy as np
import pytest

import lossless53_cases as ll
import lossy97_cases as l9
import mallat_cases as mc
import signed_cases as sc


def _coeffs53(case, family):
    seam = ll.seams(case.route)
    for x0, y0, w, h in ll.tiles_of(case.W, case.H, case.tile):
        cols, rows = seam.get((x0, y0), ((), ()))
        yield np.stack([ll.coeff_plane(family, w, h, 3 * (x0 + y0) + c, cols, rows) for c in range(case.C)])


@pytest.mark.parametrize("case", sc.cases_53(), ids=lambda c: c.id)
def test_oracle_flag_53(oracle, case):
    for family in sc.COEFF_FAMILIES_53:
        for co in _coeffs53(case, family):
            signed = sc.expect_inverse53(oracle, co, case.prec, case.nres)
            unsigned = ll.expect_inverse(oracle, co, case.prec, case.nres)
            assert np.array_equal(signed, sc.wrap_sub(unsigned, case.prec)), family
            assert not np.array_equal(signed, unsigned)


@pytest.mark.parametrize("case", sc.cases_97(), ids=lambda c: c.id)
def test_oracle_flag_97(oracle, case):
    nrs = (case.nw - 3, l9.defaults()["band_prows_97"])
    for family in case.families:
        co = np.stack([l9.coeff_plane(family, case.W, case.H, c, nrs) for c in range(3)])
        signed = sc.expect_inverse97(oracle, co, case.prec, case.nres, case.quality, case.dequantize)
        unsigned = sc.expect_inverse97(oracle, co, case.prec, case.nres, case.quality, case.dequantize, is_signed=False)
        assert np.array_equal(signed, sc.wrap_sub(unsigned, case.prec)), family
        if not case.dequantize:
            assert np.array_equal(unsigned, l9.expect_inverse(oracle, co, case.prec, case.nres))      # the keyword left the existing result alone


@pytest.mark.parametrize("m", sc.MALLAT, ids=sc.mallat_id)
def test_oracle_flag_mallat(oracle, m):
    W, H, Cn, prec, tile, nres = m[:6]
    levels = mc.levels_of(nres)
    assert mc.admissible(W, H, tile, nres) == list(range(levels + 1))        # every reduce, the one without a level (mallat_ll_kernel) included
    assert any(w < tile[0] for _, _, w, _ in mc.tiles_of(W, H, tile)) and any(h < tile[1] for _, _, _, h in mc.tiles_of(W, H, tile))
    for family in ("noise", "signedrange"):
        tiles = sc.mallat_tiles(m, family)
        for r in range(levels + 1):
            signed = sc.mallat_frame(oracle, m, tiles, r)
            unsigned = sc.mallat_frame(oracle, m, tiles, r, is_signed=False)
            assert signed.shape == (Cn, mc.shr(H, r), mc.shr(W, r))
            assert np.array_equal(signed, sc.wrap_sub(unsigned, prec)), (family, r)


def test_every_inverse_form_of_the_generators_has_a_signed_case():
    want = set()
    for gen in sc.GENERATORS_53:
        for c in gen():
            want |= sc.inverse_labels(c)
    have = set()
    for c in sc.cases_53():
        have |= sc.inverse_labels(c)
    assert want and want <= have, sorted(want - have)
    # the families of forms the issue names, by the labels of forms()
    for cpl in (2, 4, 8):
        for nc in (1, 3):
            assert "march<cpl%d,nc%d,vec>" % (cpl, nc) in have
    assert {"march<cpl2,nc1,scalar>", "march<cpl2,nc3,scalar>", "tail", "deep_flat", "deep_inv<nomid>"} <= have
    assert {"deep_inv<mid0>", "deep_inv<mid2>"} <= have and any(lab.startswith("deep_inv<mid1") for lab in have)
    for nw in (4, 8):
        for strips in ("single", "multi"):
            assert "plane_wg<nw%d,nc1,io0,%s>" % (nw, strips) in have
    assert {c.C for c in sc.cases_53()} >= {1, 3, 4}
    assert {c.prec for c in sc.cases_53()} >= {8, 12, 16, 31}
    want97 = {sc.label_97(c) for c in l9.inverse_cases()}
    have97 = {sc.label_97(c) for c in sc.cases_97()}
    assert want97 == have97 == {"inv97_march"} | {"inv97_wg<nw%d>" % n for n in l9.INV_WAVES if n}
    for lab in have97:
        mine = [c for c in sc.cases_97() if sc.label_97(c) == lab]
        assert {(c.quality, c.dequantize) for c in mine} == set(sc.QUANT_VARIANTS)
    assert {c.prec for c in sc.cases_97()} >= {8, 12, 16}


def test_pixel_cases_reach_every_pixel_writing_inverse_of_an_unsigned_plan():
    want = set()
    for c in ll.packed_cases() + ll.rgba8_cases():
        want |= sc.pixel_inverse_routes(c)
    have = set(sc.pixel_routes_covered())
    assert want and want == have
    labels = {f for f, _ in have}
    assert any(f.startswith("rgba8_wg_inv") for f in labels)
    assert any(f.startswith("plane_wg") and io == "gray16" for f, io in have) and any(f.startswith("plane_wg") and io == "rgba64" for f, io in have)
    assert {c.fmt for c in sc.pixel_cases()} == set(range(6))
    assert len(sc.pixel_cases_97()) == 3 and all(l9.wg_admitted(W, H, tile) and W % 8 == 0 for W, H, tile, _ in sc.pixel_cases_97())


@pytest.mark.parametrize("prec", sc.PIXEL_PRECISIONS)
def test_signedrange_clamps_a_third_and_keeps_a_third(oracle, prec):
    """the signed reconstruction of `signedrange` coefficients is the uniform frame minus 2^(prec - 1): the shares, from the oracle alone"""
    for w, h, C, nres in ((16, 3, 1, 2), (64, 40, 3, 3), (24, 5, 4, 6)):
        co, frame = sc.signedrange_set(w, h, C, prec, nres, seed=prec)
        signed = sc.expect_inverse53(oracle, np.array(co), prec, nres)
        assert np.array_equal(signed, sc.wrap_sub(frame, prec))
        clamped, inside = sc.clamp_shares(signed, prec)
        print("signedrange p%d %dx%dx%d: clamped to 0 %.3f, strictly inside %.3f" % (prec, w, h, C, clamped, inside))
        assert clamped >= sc.SIGNEDRANGE_MIN_SHARE and inside >= sc.SIGNEDRANGE_MIN_SHARE
        if prec in (8, 16):
            pix = sc.pixels(oracle, signed, prec)
            assert not np.array_equal(pix, sc.pixels(oracle, np.array(frame), prec))
