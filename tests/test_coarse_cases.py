"""CPU: the yardstick of the quality-scalable MQ decode (tests/coarse_cases.py) -- the properties of coarse(), what the block families
of tests/test_gpu_coarse_decode.py must contain for the floor to cut running decodes and to skip blocks whole, the deep-block recipe's
preconditions (all with the oracle alone), and the four new names in the header, the library and the binding."""
import os
import re
import subprocess

import numpy as np
import pytest

import coarse_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("j2k_decode_blocks_coarse", "j2k_plan_decode_blocks_coarse", "j2k_plan_decode_frame_pixels_coarse", "j2k_decode_pixels_host_coarse")


def _values():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.integers(-(1 << 31) + 1, 1 << 31, 4000), rng.integers(-70, 71, 4000), np.arange(-40, 41),
                        np.array([0, 1, -1, (1 << 31) - 1, -(1 << 31) + 1, 1 << 30, -(1 << 30)])])
    return v.astype(np.int32)


@pytest.mark.parametrize("k", range(32))
def test_coarse_properties(k):
    v = _values()
    c = cc.coarse(v, k)
    assert c.dtype == np.int32
    if k == 0:
        assert np.array_equal(c, v)
    assert np.array_equal(cc.coarse(c, k), c)                                   # idempotent
    small = np.abs(v.astype(np.int64)) < (1 << k)
    assert not c[small].any() and c[~small].all()                                # zero exactly where |v| < 2^k
    assert np.array_equal(np.sign(c[~small]), np.sign(v[~small]))
    a, m = np.abs(c.astype(np.int64)), np.abs(v.astype(np.int64))
    assert np.array_equal(a[~small] >> k, m[~small] >> k)                        # the decoded planes are the full decode's
    if k >= 1:
        assert np.all((a[~small] & ((1 << k) - 1)) == 1 << (k - 1))              # the midpoint of what was left
        assert np.all(np.abs(a[~small] - m[~small]) <= 1 << (k - 1))


def test_coarse_by_hand():
    v = np.array([0, 1, -1, 5, -5, 12, -13, 255, -256, 1 << 20], np.int32)
    assert cc.coarse(v, 1).tolist() == [0, 0, 0, 5, -5, 13, -13, 255, -257, (1 << 20) + 1]
    assert cc.coarse(v, 3).tolist() == [0, 0, 0, 0, 0, 12, -12, 252, -260, (1 << 20) + 4]
    assert cc.coarse(v, 31).tolist() == [0] * 10
    with pytest.raises(AssertionError):
        cc.coarse(np.array([-(1 << 31)], np.int64), 1)


@pytest.fixture(scope="module")
def families(oracle):
    return {name: make(oracle) for name, (make, _ks) in cc.FAMILIES.items()}


@pytest.mark.parametrize("name", sorted(cc.FAMILIES))
def test_families_let_the_floor_cut_and_skip(families, name):
    """for every floor k >= 1 a family is run with: at least a quarter of its blocks have numBPS > k (the floor cuts a running decode) and at
    least one has 0 < numBPS <= k (a block is skipped whole).  (k = 0 is the full decode: nothing to cut or skip.)"""
    blocks = families[name]
    nbs = np.array([b["nb"] for b in blocks])
    for k in cc.FAMILIES[name][1]:
        if k == 0:
            continue
        if (name, k) in cc.QUARTER_EXEMPT:
            above = [b for b in blocks if b["nb"] > k]
            assert len(above) == 4 and sum(1 for b in above if b.get("deep")) == 3 and sum(1 for b in above if b["w"] > 64) == 1
        else:
            assert (nbs > k).sum() * 4 >= len(blocks), (name, k)
        assert ((nbs > 0) & (nbs <= k)).any(), (name, k)
    groups = cc.by_numbps(blocks)
    assert len(groups) >= 3 and all(groups.values())


def test_family_shapes(families):
    one, st, big = families["one_launch"], families["stepped"], families["big"]
    assert {(b["w"], b["h"]) for b in one} == set(cc.ONE_LAUNCH_SHAPES) and {b["band"] for b in one} == {0, 1, 2, 3}
    assert any(b["data"].size == 0 and b["nb"] > 0 for b in one) and {0, 31} <= {b["nb"] for b in one}
    small = [b for b in st if b["w"] <= 64 and not b.get("deep")]
    assert len(small) == 100 and all(b["w"] <= 32 and b["h"] <= 32 for b in small)
    assert {b["nb"] for b in small[:50]} == set(range(15)) and {b["nb"] for b in small[50:]} == set(range(15))
    assert len(st) == 104 and 64 < len(st) < 128 and len(st) % 64                # two groups of 64 lanes, the second ragged
    assert {(b["w"], b["h"]) for b in big} == set(cc.BIG_SHAPES)


def test_deep_block_recipe(families, oracle):
    """numBPS >= 32, and the oracle's full decode stays inside |v| < 2^31 (so coarse() is defined on it, and the sign survived int32)"""
    deep = [b for f in families.values() for b in f if b.get("deep")]
    assert len(deep) >= 27
    for b in deep:
        assert b["nb"] >= 32
        v = cc.full_decode(oracle, b).astype(np.int64)
        assert np.abs(v).max() < 1 << 31 and v.any()
        cc.coarse(v, 5)


def test_every_family_block_is_inside_the_formula(families, oracle):
    for f in families.values():
        for b in f:
            assert np.abs(cc.full_decode(oracle, b).astype(np.int64)).max() < 1 << 31


def test_the_four_names_are_there():
    """header, library and binding carry the new entries (tests/test_abi_symbols.py checks that the three agree on everything)"""
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "go-jpeg2000_amd")])
    from j2kgfx import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "j2kgfx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(j2k_[a-z0-9_]+)\s*\(", txt))
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in declared and n in _lib.SYMBOLS and hasattr(L, n), n
        assert getattr(L, n).argtypes is not None
