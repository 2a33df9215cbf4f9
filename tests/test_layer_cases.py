"""CPU: the yardstick of the quality layers (tests/layer_cases.py) checked against itself on blocks coded by the oracle -- the layers' segments
are the prefixes of the codeword, every prefix decodes its planes, the cuts are monotone, compose -> read gives the tables back, one layer is the
existing closed-loop composition -- and the host-only C call j2k_tile_parts_keep_layers against the yardstick's keep_layers, the pinned streams
of tests/golden/closed_loop_layers_v1.json, and the new names in the header, the library's symbol list and the binding."""
import functools
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import coarse_cases as cc
import layer_cases as lc
import rate_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("j2k_plan_rate_allocate_layers", "j2k_plan_encode_tile_parts_layers", "j2k_plan_decode_tile_parts_layers", "j2k_plan_frame_bound_layers",
               "j2k_plan_encode_frame_pixels_layers", "j2k_plan_decode_frame_pixels_layers", "j2k_encode_pixels_host_layers",
               "j2k_decode_pixels_host_layers", "j2k_tile_parts_keep_layers")
GOLDEN = json.load(open(os.path.join(HERE, "golden", lc.GOLDEN_FILE)))


@functools.lru_cache(None)
def _golden(name):
    import oracle as orc
    import t2ref
    case = next(c for c in lc.GOLDEN_CASES if c["name"] == name)
    return lc.golden_stream(case, orc, t2ref)


# ---- cuts on hand-made tables ---------------------------------------------------------------------------------------------------------------
def test_normalise_and_segments():
    R = [0, 0, 4, 4, 9]                                              # plane 1 costs nothing, plane 3 costs nothing
    assert lc.normalise(R, [1, 2, 3, 4]) == [0, 2, 2, 4]
    segs, first = lc.segments(R, [1, 2, 3, 4])
    assert first == 1 and segs == [(0, 0, 0), (0, 4, rc.passes_of(2)), (4, 4, 0), (4, 9, rc.passes_of(4) - rc.passes_of(2))]
    assert lc.segments(R, [0, 0]) == ([(0, 0, 0), (0, 0, 0)], 2)    # in no layer: first = L
    assert lc.segments(R, [4]) == ([(0, 9, rc.passes_of(4))], 0)
    assert lc.segments(R, [1]) == ([(0, 0, 0)], 1)                   # one layer, no bytes: today's "in no layer" = 1
    assert lc.segments(R, [2, 2, 2]) == ([(0, 4, 4), (4, 4, 0), (4, 4, 0)], 0)      # a repeated cut: empty later layers


def test_allocate_layers_is_allocate_per_budget_and_monotone():
    rng = np.random.default_rng(7)
    Rs, Ds, nbs, ws = [], [], [], []
    for _ in range(30):
        nb = int(rng.integers(0, 7))
        Rs.append([int(x) for x in np.concatenate([[0], np.cumsum(rng.integers(0, 40, nb))])])
        D = np.sort(rng.integers(0, 5000, nb + 1))[::-1].astype(np.int64); D[nb] = 0
        Ds.append([int(x) for x in D]); nbs.append(nb); ws.append(float(rng.choice([0.25, 1.0, 3.5])))
    total = sum(R[nb] for R, nb in zip(Rs, nbs))
    budgets = [0, total // 20, total // 20, total // 3, total, 1 << 62]
    kept, chosen = lc.allocate_layers(Rs, Ds, nbs, ws, budgets)
    for l, b in enumerate(budgets):
        assert (kept[l], chosen[l]) == rc.allocate(Rs, Ds, nbs, ws, b)
        assert chosen[l] <= b
    assert kept[1] == kept[2] and kept[-1] == nbs and kept[-2] == nbs
    with pytest.raises(AssertionError):
        lc.allocate_layers(Rs, Ds, nbs, ws, [10, 5])
    with pytest.raises(AssertionError):
        lc.allocate_layers(Rs, Ds, nbs, ws, [])


# ---- blocks coded by the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,band,shape", [(8, 0, (9, 7)), (5, 1, (16, 16)), (12, 3, (5, 13)), (1, 2, (8, 8))])
def test_segments_are_prefixes_that_decode(oracle, bits, band, shape):
    rng = np.random.default_rng(bits * 10 + band)
    v = cc.samples(rng, shape[1], shape[0], bits)
    h, w = v.shape
    data, nb = oracle.t1_encode(v, w, h, band)
    R = lc.shortest_rates(oracle, data, nb, band, v)
    assert R[0] == 0 and R[nb] == len(data) and all(a <= b for a, b in zip(R, R[1:]))
    for cuts in ([nb], [0, nb], [nb // 3, nb // 3, 2 * nb // 3, nb, nb], list(range(0, nb + 1))):
        segs, first = lc.segments(R, cuts)
        Q = lc.normalise(R, cuts)
        assert all(a <= b for a, b in zip(Q, Q[1:])) and all(q <= p for q, p in zip(Q, cuts))
        for k in range(1, len(cuts) + 1):
            cat = b"".join(bytes(bytearray(data[lo:hi])) for lo, hi, _ in segs[:k])
            assert cat == bytes(bytearray(data[:R[Q[k - 1]]]))
            assert sum(s[2] for s in segs[:k]) == rc.passes_of(Q[k - 1])
            assert rc.prefix_ok(oracle, data, R[Q[k - 1]], nb, band, v, Q[k - 1])
            # Q drops only planes that cost no bytes: the prefix decodes the caller's cut as well
            assert rc.prefix_ok(oracle, data, R[Q[k - 1]], nb, band, v, cuts[k - 1]) or R[cuts[k - 1]] == R[Q[k - 1]]
        assert first == next((l for l, s in enumerate(segs) if s[1] > s[0]), len(cuts))


@pytest.mark.parametrize("name", [c["name"] for c in lc.GOLDEN_CASES])
def test_compose_then_read_returns_the_tables(oracle, name):
    import t2ref
    case = next(c for c in lc.GOLDEN_CASES if c["name"] == name)
    pix, (_, tiles, datas, nbs, Rs, Ds, ws, _ct), kept, (stream, toffs, loffs) = _golden(name)
    L, n = len(kept), len(datas)
    assert all(kept[l][j] <= kept[l + 1][j] for l in range(L - 1) for j in range(n))                      # monotone cuts
    assert len(toffs) == len(tiles) + 1 and len(loffs) == len(tiles) * L and toffs[-1] == len(stream)
    assert all(loffs[t * L + L - 1] == toffs[t + 1] for t in range(len(tiles)))
    assert any(0 < kept[0][j] < nbs[j] for j in range(n)) or kept[0] == [0] * n
    for k in range(1, L + 1):
        got = lc.read_layers(t2ref, stream, toffs, tiles, k, case["marks"], case["marks"])
        for j in range(n):
            q = lc.normalise(Rs[j], [kept[l][j] for l in range(L)])[k - 1]
            g = got[j]
            cat = b"".join(stream[o:o + ln] for o, ln in g["segs"])
            assert cat == datas[j][:Rs[j][q]], (k, j)
            if q:
                assert (g["zbp"], g["passes"]) == (31 - nbs[j], rc.passes_of(q)) and (g["floor"], g["numbps"]) == (nbs[j] - q, nbs[j]), (k, j)
            else:
                assert (g["passes"], g["floor"], g["numbps"]) == (0, 0, 0), (k, j)
    with pytest.raises(t2ref.EOF):                                  # more layers than the stream holds
        lc.read_layers(t2ref, stream, toffs, tiles, L + 1, case["marks"], case["marks"])


@pytest.mark.parametrize("name", [c["name"] for c in lc.GOLDEN_CASES])
@pytest.mark.parametrize("marks", [False, True], ids=["bare", "sop_eph"])
def test_one_layer_is_the_existing_composition(oracle, name, marks):
    import t2ref
    pix, (_, tiles, datas, nbs, Rs, Ds, ws, _ct), kept, _ = _golden(name)
    for ps in kept + [[0] * len(nbs)]:
        one, toffs, loffs = lc.compose(t2ref, tiles, datas, nbs, Rs, [ps], marks, marks)
        assert one == lc.compose_kept(t2ref, tiles, datas, nbs, Rs, ps, marks, marks)
        assert loffs == toffs[1:]


# ---- j2k_tile_parts_keep_layers: the C ABI without a device ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codestream():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "go-jpeg2000_amd")])
    from j2kgfx import codestream as cs
    return cs


@pytest.mark.parametrize("name", [c["name"] for c in lc.GOLDEN_CASES])
def test_keep_layers_c_call_against_the_yardstick(oracle, codestream, name):
    import t2ref
    from j2kgfx import _lib
    case = next(c for c in lc.GOLDEN_CASES if c["name"] == name)
    pix, (_, tiles, datas, nbs, Rs, Ds, ws, _ct), kept, (stream, toffs, loffs) = _golden(name)
    L = len(kept)
    for k in range(1, L + 1):
        want, wtoffs = lc.keep_layers(stream, toffs, loffs, L, k)
        got, gtoffs = codestream.keep_layers(stream, toffs, loffs, k)
        assert got == want and [int(x) for x in gtoffs] == wtoffs, k
        if k == L:
            assert got == stream and wtoffs == toffs
        # the cut stream read with layers = k is the whole stream read with layers = k (offsets apart)
        a = lc.read_layers(t2ref, want, wtoffs, tiles, k, case["marks"], case["marks"])
        b = lc.read_layers(t2ref, stream, toffs, tiles, k, case["marks"], case["marks"])
        for j in a:
            assert (a[j]["zbp"], a[j]["passes"], [n for _, n in a[j]["segs"]]) == (b[j]["zbp"], b[j]["passes"], [n for _, n in b[j]["segs"]])
        with pytest.raises(t2ref.EOF):
            lc.read_layers(t2ref, want, wtoffs, tiles, k + 1, case["marks"], case["marks"])
    for bad in (0, L + 1, -1):
        with pytest.raises(_lib.J2KError) as e:
            codestream.keep_layers(stream, toffs, loffs, bad)
        assert e.value.status == _lib.ERR_INVALID_ARG
    with pytest.raises(_lib.J2KError) as e:                          # a layer end outside its tile-part
        codestream.keep_layers(stream, toffs, [len(stream) + 1] * len(loffs), 1)
    assert e.value.status == _lib.ERR_INVALID_ARG


# ---- the pinned streams -----------------------------------------------------------------------------------------------------------------------
def test_golden_file_covers_the_cases():
    assert sorted(GOLDEN) == sorted(c["name"] for c in lc.GOLDEN_CASES) and len(GOLDEN) == 2


@pytest.mark.parametrize("name", [c["name"] for c in lc.GOLDEN_CASES])
def test_yardstick_composes_the_pinned_streams(oracle, name):
    pix, tab, kept, (stream, toffs, loffs) = _golden(name)
    g = GOLDEN[name]
    assert len(stream) == g["bytes"] and stream[:24].hex() == g["head"] and hashlib.sha256(stream).hexdigest() == g["sha256"]
    assert [int(x) for x in loffs] == g["layer_offs"] and len(kept) == g["layers"]


# ---- names --------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "j2kgfx.h")).read()
    libpy = open(os.path.join(ROOT, "go-jpeg2000_amd", "j2kgfx", "_lib.py")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert '"%s"' % s in libpy, s
