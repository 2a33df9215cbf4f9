"""CPU: the case lists of tests/ht_stream_cases.py -- HT block streams the encoder never writes -- before the GPU sees them
(tests/test_gpu_ht_decode_streams.py).  On every case the C oracle (orc_ht_decode) and the Python restatement (pyref.HTDecoder) agree: two
independent restatements of ht.go:93-864, so a case on which they differed would be a finding about the oracle, not about a kernel.  And the
lists hold what they are meant to hold: every (bucket x shape) cell of M is filled, the streams with a u of 32 and more come with few and
many 0xFF bytes and with short and long MagSgn segments, V's written-down expectations are the reference's, and the random streams do not
all decode to zero."""
import collections

import numpy as np
import pytest

import ht_stream_cases as hc


@pytest.fixture(scope="module")
def decoded(oracle):
    """{group: [(case, Info, oracle's decode)]}; C oracle == pyref asserted on the way, once for all tests of this file"""
    out = {}
    for name, make in hc.GROUPS.items():
        rows = []
        for c in make():
            info, py = hc.classify(c.data, c.w, c.h, want_out=True)
            want = oracle.ht_decode(np.frombuffer(c.data, np.uint8), c.w, c.h)
            assert np.array_equal(py, want), "the C oracle and pyref disagree on %s (%dx%d, %d bytes)" % (c.label, c.w, c.h, len(c.data))
            rows.append((c, info, want))
        out[name] = rows
    return out


def test_oracles_agree_on_every_case_and_group_sizes(decoded):
    sizes = {g: len(rows) for g, rows in decoded.items()}
    assert sizes["G"] == 4 * len(hc.G_SHAPES)
    assert sizes["E"] == len(hc.E_SHAPES) * len(hc.E_AMPS) * hc.E_VARIANTS
    assert sizes["S"] == len(hc.S_LENGTHS) * len(hc.S_CONTENTS)
    assert 1300 <= sizes["M"] <= 1700, sizes
    print("cases per group:", sizes)


def test_builders_round_trip():
    rng = np.random.default_rng(5)
    suf = hc.random_suffix(rng, 300)
    assert hc.scup_of(suf) == 300 and suf[-2] >> 4 == hc.with_scup(suf, 0xABC)[-2] >> 4
    assert hc.with_scup(suf, 0xABC)[-1] == 0xBC and hc.with_scup(suf, 0xABC)[-2] & 0x0F == 0x0A
    for mag in (b"", b"\xff", bytes(range(200))):
        assert hc.split(hc.splice(mag, suf)) == (mag, suf)
    # the same seed gives the same lists (no clock, no global random state)
    hc.group_S.cache_clear()
    a = hc.group_S()
    hc.group_S.cache_clear()
    assert a == hc.group_S()


def test_m_every_bucket_and_shape_cell_is_filled_and_the_suffix_alone_fixes_u(decoded):
    cells = hc.m_suffixes()
    counts = {(s, b): len(cells[(s, b)]) for s in hc.M_SHAPES for b in hc.BUCKETS}
    msg = "suffixes per (shape, bucket): %s; draws per shape: %s" % (counts, cells["draws"])
    print(msg)
    assert all(n >= 6 for n in counts.values()), msg
    for s in hc.M_SHAPES:
        for b in hc.BUCKETS:
            for suf in cells[(s, b)]:
                assert hc.bucket_of(hc.classify(suf, s[0], s[1]).max_u) == b
    # whatever MagSgn segment stands in front: the same largest u, and the classifier's segment length and 0xFF count are those of the segment
    used = collections.Counter()
    u_of = {(s, suf): hc.classify(suf, s[0], s[1]).max_u for s in hc.M_SHAPES for b in hc.BUCKETS for suf in cells[(s, b)]}
    for c, info, _ in decoded["M"]:
        mag, suf = hc.split(c.data)
        assert info.reject == "none" and hc.bucket_of(info.max_u) == c.bucket, c.label
        assert info.max_u == u_of[((c.w, c.h), suf)], c.label
        assert (info.seg_len, info.n_ff) == (len(mag), mag.count(0xFF))
        used[((c.w, c.h), c.bucket)] += 1
    assert all(used[(s, b)] >= 84 for s in hc.M_SHAPES for b in hc.BUCKETS), used       # every (length, content) met every cell
    # every length with random content, every content at the five lengths
    have = {(c.label.split(",")[0]) for c, _, _ in decoded["M"]}
    for n in hc.M_LENGTHS:
        assert "M random x %d" % n in have
    for n in hc.M_ALL_CONTENT_LENGTHS:
        for kind in hc.M_CONTENTS:
            assert "M %s x %d" % (kind, n) in have


def test_m_streams_with_u_of_32_and_more_come_in_all_three_magsgn_situations(decoded):
    counts = collections.Counter()
    for c, info, _ in decoded["M"]:
        if info.n_ff <= 64 and info.seg_len <= 4240:
            counts[(c.bucket, "0xFF <= 64 and segment <= 4240")] += 1
        if info.n_ff > 64:
            counts[(c.bucket, "0xFF > 64")] += 1
        if info.seg_len > 4240:
            counts[(c.bucket, "segment > 4240")] += 1
        for edge in (63, 64, 65):
            if info.n_ff == edge and info.seg_len <= 4240:
                counts[(c.bucket, "0xFF == %d" % edge)] += 1
        for edge in (4239, 4240, 4241):
            if info.seg_len == edge:
                counts[(c.bucket, "segment == %d" % edge)] += 1
    msg = "M streams per (bucket, situation): %s" % dict(sorted(counts.items()))
    print(msg)
    for b in ("=32", ">=33"):
        for what in ("0xFF <= 64 and segment <= 4240", "0xFF > 64", "segment > 4240"):
            assert counts[(b, what)] >= 10, msg
        for what in ("0xFF == 63", "0xFF == 64", "0xFF == 65", "segment == 4239", "segment == 4240", "segment == 4241"):
            assert counts[(b, what)] >= 1, msg


def test_v_written_down_expectations_hold(decoded):
    seen = collections.Counter()
    for c, info, want in decoded["V"]:
        assert c.expect, c.label
        assert info.reject == c.expect, (c.label, info)
        if c.expect != "none":
            assert not want.any()
        seen[((c.w, c.h), c.expect)] += 1
    print("V cases per (shape, expectation):", dict(seen))
    for shape in ((16, 16), (64, 64)):
        for exp in ("len<2", "scup<2", "scup>len", "mel", "none"):
            assert seen[(shape, exp)] >= 2, seen


def test_random_streams_do_not_all_decode_to_zero(decoded):
    """at most 10 % of the streams with a random suffix, on blocks of 16 samples and more, decode to all-zero: the GPU test cannot pass on
    `everything came out zero`"""
    for g in ("G", "M", "S"):
        rows = [(c, want) for c, _, want in decoded[g] if c.rand and c.w * c.h >= 16]
        zero = sum(1 for _, want in rows if not want.any())
        msg = "%s: %d of %d random-suffix streams decode to zero" % (g, zero, len(rows))
        print(msg)
        assert len(rows) >= 40 and zero * 10 <= len(rows), msg


def test_groups_feed_every_route_by_the_streams_properties(decoded):
    """route counts from the streams alone (shape rules of the issue's table written as geometry, not taken from a kernel)"""
    n = collections.Counter()
    for g, rows in decoded.items():
        for c, info, want in rows:
            coded = ((c.h + 3) // 4) * c.w
            pairs = ((c.h + 3) // 4) * ((((c.w + 3) // 4) + 1) // 2)
            if coded > 1024 or pairs > 128:
                n[(g, "large by geometry")] += 1
            elif info.reject != "none":
                n[(g, "refused: " + info.reject)] += 1
            else:
                n[(g, "u " + hc.bucket_of(info.max_u))] += 1
    print("blocks per (group, kind):", dict(sorted(n.items())))
    assert n[("G", "large by geometry")] >= 16            # (65,60) (64,68) (1028,4) (4,516) (129,32): four streams each, and more
    for kind in ("u <=31", "u =32", "u >=33"):
        assert n[("G", kind)] + n[("S", kind)] + n[("E", kind)] >= 5, (kind, n)
    for why in ("len<2", "scup<2", "scup>len", "mel"):
        assert n[("V", "refused: " + why)] >= 4
    assert n[("E", "refused: scup>len")] >= 15 and n[("E", "refused: scup<2")] >= 15


@pytest.mark.parametrize("geo", hc.PLANS, ids=["328x211_cb64", "200x150_cb16_tile64"])
@pytest.mark.parametrize("windows", [0, 1])
def test_the_lists_can_supply_the_plans_of_the_gpu_tests(oracle, geo, windows):
    """the plan (windows = 0) and closed-loop (windows = 1) tests replace every job's body by a case of its shape: on the job lists of their two
    geometries (the oracle's enumeration, tile by tile) bodies_for() hands out at least 5 blocks of each kind the tests ask for -- known here,
    not found out on the device.  Only M's suffixes supply u = 32 in quantity: per shape of M, each bucket holds far more than 5 streams"""
    m = collections.Counter(((c.w, c.h), c.bucket) for c in hc.group_M())
    assert all(m[(s, b)] >= 84 for s in ((64, 64), (16, 16)) for b in hc.BUCKETS), m
    tw, th = geo["tile"][0] or geo["W"], geo["tile"][1] or geo["H"]
    shapes = []
    for y0 in range(0, geo["H"], th):
        for x0 in range(0, geo["W"], tw):
            jobs = oracle.enumerate_blocks(3, min(tw, geo["W"] - x0), min(th, geo["H"] - y0), geo["nres"], geo["cb"], geo["cb"], windows)
            shapes += [(int(j["w"]), int(j["h"])) for j in jobs]
    for seed in (0x6300 + geo["W"], 0x6400 + geo["W"]):
        kinds = hc.kinds(hc.bodies_for(shapes, seed))
        print("%s windows %d: %d jobs, %s" % (geo, windows, len(shapes), kinds))
        assert all(kinds[k] >= 5 for k in ("refused", "<=31", "=32", ">=33", "far")), kinds
