"""CPU: tests/pass_stream_cases.py checked against the oracle and against pass_cases / coarse_cases -- decode_passes pinned three ways, the
pass-granular shortest-prefix tables, and every foreign pass family on the streams the GPU test uses (so that the device comparison stands on
expectations that were themselves checked)."""
import numpy as np
import pytest

import coarse_cases as cc
import pass_cases as pc
import pass_stream_cases as ps
import stream_reader_cases as sr

SMALL = [(w, h) for (w, h) in pc.SHAPES if w <= 16 and h <= 16]


def _u8(data):
    return np.ascontiguousarray(np.asarray(data, np.uint8))


# ---- decode_passes --------------------------------------------------------------------------------------------------------------------------
def test_decode_passes_with_nothing_left_out_is_the_oracle(oracle):
    """f = 0: intact codewords in every band, damaged and arbitrary ones, empty data, numbps above and below the block's own"""
    rng = np.random.default_rng(31)
    seen = 0
    for (w, h) in SMALL:
        for content in pc.CONTENTS:
            v = pc.block(w, h, content)
            for band in cc.BANDS:
                data, nb = oracle.t1_encode(v, w, h, band)
                nb = int(nb)
                for d, n in ((data, nb), (data[:len(data) // 2], nb), (data[:0], max(nb, 3)), (data, min(nb + 2, 31)), (data, max(nb - 1, 0))):
                    assert np.array_equal(ps.decode_passes(bytes(bytearray(d)), n, band, w, h, 0), oracle.t1_decode(_u8(d), n, band, w, h).reshape(h, w)), (w, h, content, band)
                    seen += 1
            g = cc.arbitrary(rng, w, h, 0, 6)
            assert np.array_equal(ps.decode_passes(bytes(g["data"]), 6, 1, w, h, 0), oracle.t1_decode(g["data"], 6, 1, w, h).reshape(h, w)), (w, h, content)
    assert seen >= 300
    assert not ps.decode_passes(b"\x12\x34", 0, 0, 5, 7, 0).any() and ps.decode_passes(b"", 0, 2, 5, 7, 4).shape == (7, 5)


def test_decode_passes_at_whole_planes_is_coarse_of_the_oracle(oracle):
    """f = 3 k on intact codewords: coarse_cases.coarse of oracle.t1_decode's output, k beyond the block's planes included"""
    for (w, h) in SMALL:
        for content in pc.CONTENTS:
            v = pc.block(w, h, content)
            band = (w + h) % 4
            data, nb = oracle.t1_encode(v, w, h, band)
            nb = int(nb)
            full = oracle.t1_decode(_u8(data), nb, band, w, h).reshape(h, w)
            assert np.array_equal(full, v)
            for k in sorted({0, 1, 2, nb // 2, max(nb - 1, 0), nb, min(nb + 1, 31), 31}):
                assert np.array_equal(ps.decode_passes(bytes(bytearray(data)), nb, band, w, h, 3 * k), cc.coarse(full, k)), (w, h, content, k)


@pytest.mark.parametrize("content", pc.CONTENTS)
def test_decode_passes_on_shortest_prefixes_is_coarse_pass(oracle, content):
    """every q of every small shape: the prefix R[q] decoded points - q passes short is coarse_pass(v, nb, q, sp), and so is the whole codeword; R
    keeps the table's invariants; f beyond the block's passes gives zeros"""
    loose_shorter = inside = 0
    for (w, h) in SMALL:
        v = pc.block(w, h, content)
        data, nb = oracle.t1_encode(v, w, h, 0)
        nb, data = int(nb), _u8(data)
        sp = pc.sp_mask(v, nb)
        last = pc.points(nb)
        R = ps.shortest_rates_pass(oracle, data, nb, 0, v, sp)
        loose = ps.shortest_rates_pass(oracle, data, nb, 0, v, sp, strict=False)
        assert len(R) == last + 1 and R[0] == 0 and R[last] == len(data) and all(a <= b for a, b in zip(R, R[1:]))
        assert all(a >= b for a, b in zip(R, loose))
        loose_shorter += sum(a > b for a, b in zip(R, loose))
        for q in range(last + 1):
            want = pc.coarse_pass(v, nb, q, sp)
            assert pc.prefix_ok_pass(oracle, data, R[q], nb, 0, v, q, sp), (w, h, q)
            assert np.array_equal(ps.decode_passes(bytes(data[:R[q]]), nb, 0, w, h, last - q), want), (w, h, q)
            assert np.array_equal(ps.decode_passes(bytes(data), nb, 0, w, h, last - q), want), (w, h, q)
            inside += int(q >= 1 and pc.split(q)[1] > 0 and not np.array_equal(want, pc.coarse_pass(v, nb, q - 1, sp)))
        for f in (last + 1, last + 2, 93, 255):
            assert not ps.decode_passes(bytes(data), nb, 0, w, h, f).any(), (w, h, f)
    print("%s: %d table entries longer than pass_cases.prefix_ok_pass alone asks; %d passes inside a plane that change a sample" % (content, loose_shorter, inside))
    if content in ("noise", "gradient", "sparse"):
        assert inside > 0, "vacuous: no pass inside a plane changed anything"


def test_the_record_is_not_the_magnitude():
    """the midpoint comes from who the partial plane touched: a hand-made case where the two samples of one magnitude class differ"""
    import oracle as orc
    v = np.array([[13, -5, 0, 4]], np.int32)                          # pass_cases' hand-made block: after q = 2 the 13 stands at floor 3, the -5 at floor 2
    data, nb = orc.t1_encode(v, 4, 1, 0)
    sp = pc.sp_mask(v, 4)
    for q, want in ((1, [[12, 0, 0, 0]]), (2, [[12, -6, 0, 0]]), (3, [[14, -6, 0, 0]]), (4, [[14, -6, 0, 6]])):
        assert ps.decode_passes(bytes(bytearray(data)), int(nb), 0, 4, 1, pc.points(4) - q).tolist() == want == pc.coarse_pass(v, 4, q, sp).tolist()


# ---- tables and families --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", sorted(sr.GEOMETRIES))
def test_pass_tables_tie_to_the_plane_tables(oracle, geom):
    T = ps.pass_tables(geom)
    _, tiles, datas, nbs, Rs, _ = sr.tables(geom)
    assert T["tiles"] == tiles and T["nbs"] == nbs
    for j, nb in enumerate(nbs):
        R = T["Rs"][j]
        assert len(R) == pc.points(nb) + 1 and R[0] == 0 and R[-1] == len(datas[j]) and all(a <= b for a, b in zip(R, R[1:]))
        for p in range(1, nb + 1):                                   # behind Cleanup the two definitions ask the same; the pass table is monotone over more points
            assert R[3 * p - 2] >= Rs[j][p], (j, p)


def test_big_pass_tables(oracle):
    T = ps.pass_tables("b", True)
    assert sorted(set(T["nbs"])) == [0, 1, 31]
    cuts = []
    for rnd in range(ps.BIG_ROUNDS):
        F = ps.big_family(rnd)
        cuts += [q for q, nb in zip(F["qs"], T["nbs"]) if nb == 31]
    assert sorted(cuts) == sorted(ps.BIG_CUTS)


@pytest.mark.parametrize("fam", ps.PASS_FAMILIES)
@pytest.mark.parametrize("geom", sorted(sr.GEOMETRIES))
def test_families_are_foreign_and_decode_to_coarse_pass(oracle, geom, fam):
    """what the family says it is; the yardstick reads both marker forms to the tables of the cuts; decode_passes of what it reads is coarse_pass
    for every block the header is honest about"""
    import t2ref
    T = ps.pass_tables(geom)
    nbs, n = T["nbs"], len(T["nbs"])
    F = ps.pass_family(geom, fam)
    qs = F["qs"]
    if fam in ("P-random", "P-claims"):
        have = [q for j, q in enumerate(qs) if j not in F["claims"]]
        assert 0 in have and any(q == pc.points(nb) for q, nb in zip(qs, nbs)) and any(pc.split(q)[1] for q in have if q)
        if fam == "P-random":
            assert qs[:3] == [0, 1, 2] and qs[3] == pc.points(nbs[3]) - 1 and qs[4] == pc.points(nbs[4])
    if fam in ("P-s1", "P-s2"):
        assert all(pc.split(q)[1] == int(fam[-1]) for q, nb in zip(qs, nbs) if nb >= 2) and sum(nb >= 2 for nb in nbs) >= n // 2
    if fam == "P-long":
        longer = sum(F["lengths"][j] > T["Rs"][j][qs[j]] for j in range(n))
        print("%s P-long: %d of %d bodies longer than R[q], %d moved to the next length, %d fell back" % (geom, longer, n, F["moved"], F["fallback"]))
        assert 20 * F["fallback"] <= n and 2 * longer >= n
    if fam == "P-claims":
        assert set(F["claims"].values()) == {"passes", "zbp"}
        assert all(any(F["claims"].get(j) == "passes" for j in pk) for packets in T["tiles"] for pk in packets if any(nbs[j] and T["datas"][j] for j in pk))
    partial = 0
    for marks in (False, True):
        stream, toffs, _ = ps.pass_stream(geom, fam, marks)
        for offs in (toffs, None):
            got = sr.read_tiles(t2ref, stream, offs, T["tiles"], 1, marks, marks)
            assert sr.frame_ok(got), [v["why"] for v in got]
        tab = sr.block_tables_pass(stream, got)
        coeffs = ps.expected_coeffs(T, tab)
        for j in range(n):
            data, pfloor, numbps = tab[j]
            assert data == T["datas"][j][:F["lengths"][j]], (geom, fam, j)
            if j in F["claims"]:
                continue
            assert (pfloor, numbps) == ((pc.pfloor_of(nbs[j], qs[j]), nbs[j]) if data else (0, 0)), (geom, fam, j)
            assert np.array_equal(coeffs[j], pc.coarse_pass(T["vs"][j], nbs[j], qs[j] if data else 0, T["sps"][j])), (geom, fam, j)
        partial += len(ps.partial_blocks(tab))
        # behind a lone SigProp pass of plane k - 1 a block holds samples of both kinds -- older ones at floor k and ones the pass turned at
        # floor k - 1: a decoder that gave every sample the same midpoint would differ from these expectations
        older = turned = 0
        for j in ps.partial_blocks(tab):
            k, part = pc.decode_plan(tab[j][1])
            if part == 1:
                a = np.abs(coeffs[j].astype(np.int64))
                older += int((a >= 1 << k).sum())
                turned += int(((a > 0) & (a < 1 << k)).sum())
        if fam in ("P-random", "P-s1"):
            assert older > 0 and turned > 0, (geom, fam, older, turned)
        # the older reader's expectation on the same stream: the whole planes of every cut
        whole = ps.whole_plane_coeffs(T, sr.block_tables(stream, got))
        for j in range(n):
            if j not in F["claims"] and tab[j][0]:
                p = pc.split(qs[j])[0]
                assert np.array_equal(whole[j], cc.coarse(T["vs"][j], nbs[j] - p)), (geom, fam, j)
    assert partial > 0 or fam == "P-long"


@pytest.mark.parametrize("rnd", range(ps.BIG_ROUNDS))
def test_big_family_decodes_to_coarse_pass(oracle, rnd):
    import t2ref
    T = ps.pass_tables("b", True)
    stream, toffs, F = ps.big_stream(rnd, bool(rnd & 1))
    got = sr.read_tiles(t2ref, stream, toffs, T["tiles"], 1, bool(rnd & 1), bool(rnd & 1))
    assert sr.frame_ok(got)
    tab = sr.block_tables_pass(stream, got)
    coeffs = ps.expected_coeffs(T, tab)
    for j, nb in enumerate(T["nbs"]):
        assert (tab[j][1], tab[j][2]) == ((pc.pfloor_of(nb, F["qs"][j]), nb) if tab[j][0] else (0, 0)), j
        assert np.array_equal(coeffs[j], pc.coarse_pass(T["vs"][j], nb, F["qs"][j] if tab[j][0] else 0, T["sps"][j])), j
