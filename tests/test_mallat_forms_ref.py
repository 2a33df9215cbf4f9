"""CPU: the cases of tests/mallat_forms_cases.py are what their comments claim -- so that a wrong case shows here, without a GPU -- and the
yardstick (tests/mallat_cases.py) round-trips every one of them."""
import numpy as np
import pytest

import lossless53_cases as ll
import mallat_cases as mc
import mallat_forms_cases as fc


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_round_trip(oracle, case):
    W, H, Cn, prec, tile, nres = case
    for family in ("noise", "impulse"):
        frm = fc.frame(case, family)
        tiles = mc.forward_frame(oracle, frm, tile, prec, nres)
        assert np.array_equal(mc.inverse_frame(oracle, tiles, W, H, tile, prec, nres), frm), family


def _only(case):
    d = fc.level_dims(case)
    assert len(d) == 1
    return next(iter(d.values()))


def test_case_table_is_complete():
    assert len(fc.CASES) == len(fc.FUSED) == 10
    for case, fused in zip(fc.CASES, fc.FUSED):
        assert (fused is None) == (fc.pix_format(case) is None), case
        assert case[0] % 8 == 0          # every frame row is whole 16-byte lanes of eight pixels: nothing but the tables decides FUSED


def test_case1_rgba8_level0():
    case = fc.CASES[0]
    d = _only(case)
    assert d[:5] == [(384, 30), (192, 15), (96, 8), (48, 4), (24, 2)] and mc.levels_of(case[5]) == 5
    assert ll.pick_cpl(d[0][0]) == 8 and fc.wg_contract(*d[0]) and d[0][0] <= 512
    dflt = ll.defaults()
    halfH = (d[0][1] + 1) // 2
    assert halfH == 15
    fwd = [min(dflt["l0_wg"] - 1, halfH - q) for q in range(0, halfH, dflt["l0_wg"] - 1)]
    assert fwd == [7, 7, 1]
    assert dflt["l0_wg_invw"] - 1 == 3 and halfH % 3 == 0
    assert d[1][1] % 2 == 1                                           # level 1: odd height
    assert fc.DISPATCHES_CASE1[1] == fc.DISPATCHES_CASE1[3] == mc.levels_of(case[5]) - 1          # one launch per level below level 0


def test_case2_all_lanes_odd_height():
    d = _only(fc.CASES[1])
    assert d[0] == (512, 35) and d[0][0] // 8 == 64 and d[0][1] % 2 == 1
    assert fc.wg_contract(*d[0])


def test_case3_edge_tiles():
    case = fc.CASES[2]
    d = fc.level_dims(case)
    assert sorted((w, h) for _, _, w, h in d) == [(16, 12), (16, 32), (384, 12), (384, 32)]
    assert all(fc.wg_contract(*v[0]) and v[0][0] <= 512 for v in d.values())          # level 0: every plane in the RGBA8 workgroup table
    w1 = sorted({v[1][0] for v in d.values()})
    assert w1 == [8, 192]                                                              # level 1: an 8-wide plane
    assert all(w % 4 == 0 for _, _, w, _ in d)                                         # ... and the general Mallat launches take the vector path
    assert mc.admissible(case[0], case[1], case[4], case[5]) == [0, 1, 2, 3, 4]


def test_case4_no_rgba8_table():
    d = fc.level_dims(fc.CASES[3])
    assert sorted(w for _, _, w, _ in d) == [8, 384] and not fc.wg_contract(8, 20)
    assert fc.FUSED[3] == (0, 0)


def test_case5_three_strips():
    d = _only(fc.CASES[4])
    assert d[0] == (1040, 10) and fc.wg_contract(*d[0])
    assert [min(512, 1040 - c) for c in range(0, 1040, 512)] == [512, 512, 16]
    assert d[1] == (520, 5)                                                        # level 1: odd height
    assert 512 in fc.seam_map(fc.CASES[4])[(0, 0)][0]


def test_case6_idle_lanes_odd_height():
    case = fc.CASES[5]
    d = _only(case)
    assert d[0] == (64, 21) and d[0][0] // 8 < 64 and fc.wg_contract(*d[0])
    assert d[0][1] % 2 == 1 and d[1] == (32, 11) and d[2] == (16, 6)


def test_cases_7_to_10():
    for i, dims0 in ((6, (64, 20)), (7, (384, 12)), (8, (64, 12)), (9, (384, 16))):
        d = _only(fc.CASES[i])
        assert d[0] == dims0 and fc.wg_contract(*d[0])
    assert fc.pix_format(fc.CASES[6]) == 3 and fc.pix_format(fc.CASES[7]) == 4 and fc.pix_format(fc.CASES[8]) == 5
    assert fc.pix_format(fc.CASES[9]) is None                                          # 12 bit: no Go image type
