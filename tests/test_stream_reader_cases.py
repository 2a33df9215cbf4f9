"""CPU: tests/stream_reader_cases.py checked against layer_cases / rate_cases on the streams the GPU test uses -- read_tiles on every cut family,
geometry and layer count, the damaged copies' verdicts (so that the device comparison cannot be vacuous), and the host-only C call
j2k_tile_parts_keep_layers on 32-layer streams and on hostile offset tables."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import layer_cases as lc
import stream_reader_cases as sr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MARKS = [False, True]
MARK_IDS = ["bare", "sop_eph"]


def _ks(L):
    return [k for k in sr.LAYER_COUNTS if k <= L]


# ---- the families are what they say ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", sorted(sr.GEOMETRIES))
def test_families_are_foreign_cuts(oracle, geom):
    _, tiles, datas, nbs, Rs, _ = sr.tables(geom)
    n = len(nbs)
    kept = sr.family("L32-mod5", tiles, nbs, Rs)
    firsts = [lc.segments(Rs[j], [kept[l][j] for l in range(32)]) for j in range(n)]
    assert any(f == 31 for _, f in firsts) and any(f == 32 for _, f in firsts)                       # first contribution in the last layer; never
    in_0_5_31 = [[l for l, (lo, hi, _) in enumerate(s) if hi > lo] for s, _ in firsts]
    assert [0, 5, 31] in in_0_5_31
    assert any(len(ls) == nbs[j] and ls == list(range(nbs[j])) for j, ls in enumerate(in_0_5_31) if j % 5 == 3)    # a plane a layer
    kept = sr.family("L1-random", tiles, nbs, Rs)
    assert 0 in kept[0] and any(p == nb for p, nb in zip(kept[0], nbs)) and any(0 < p < nb for p, nb in zip(kept[0], nbs))
    kept = sr.family("L2-empty0-tile", tiles, nbs, Rs)
    assert all(kept[0][j] == 0 for pk in tiles[0] for j in pk) and kept[1] == list(nbs) and (len(tiles) == 1 or any(kept[0]))
    assert not any(sr.family("L2-empty0-all", tiles, nbs, Rs)[0])
    kept = sr.family("L3-free-planes", tiles, nbs, Rs)
    free = [j for j in range(n) if any(Rs[j][p] == Rs[j][p - 1] for p in range(1, nbs[j] + 1))]
    assert all(lc.normalise(Rs[j], [kept[l][j] for l in range(3)]) != [kept[l][j] for l in range(3)] for j in free)       # normalise folds each of them
    assert free or geom == "b"
    kept = sr.family("L32-all-in-0", tiles, nbs, Rs)
    assert all(row == list(nbs) for row in kept)


def test_big_tables_hold_31_planes(oracle):
    _, tiles, datas, nbs, Rs, ctiles = sr.tables("b", True)
    assert sorted(set(nbs)) == [0, 1, 31] and len(tiles) == 1
    assert all(R[0] == 0 and R[nb] == len(d) for R, nb, d in zip(Rs, nbs, datas))


# ---- read_tiles on intact streams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("marks", MARKS, ids=MARK_IDS)
@pytest.mark.parametrize("fam", sr.FAMILIES)
@pytest.mark.parametrize("geom", sorted(sr.GEOMETRIES))
def test_read_tiles_returns_the_tables(oracle, geom, fam, marks):
    import t2ref
    _, tiles, datas, nbs, Rs, _ = sr.tables(geom)
    stream, toffs, loffs, kept = sr.base_stream(geom, fam, marks)
    L = len(kept)
    assert toffs[-1] == len(stream) and len(loffs) == len(tiles) * L
    if L == 1:
        assert stream == lc.compose_kept(t2ref, tiles, datas, nbs, Rs, kept[0], marks, marks)
    for k in _ks(L):
        want = sr.expected(Rs, nbs, kept, k)
        ref_ = lc.read_layers(t2ref, stream, toffs, tiles, k, marks, marks)
        for offs in (toffs, None):
            got = sr.read_tiles(t2ref, stream, offs, tiles, k, marks, marks)
            assert sr.frame_ok(got) and len(got) == len(tiles), [v["why"] for v in got]
            tab = sr.block_tables(stream, got)
            for v in got:
                for j, s in v["blocks"].items():
                    lens, passes, floor, numbps, nbytes = want[j]
                    assert ([ln for _, ln in s["segs"]], s["passes"], s["floor"], s["numbps"]) == (lens, passes, floor, numbps), (k, j)
                    assert s["zbp"] == (31 - nbs[j] if lens else s["zbp"]) and not s["dropped"]
                    assert tab[j][0] == datas[j][:nbytes], (k, j)
                    r = ref_[j]
                    assert (s["segs"], s["zbp"], s["floor"], s["numbps"]) == (r["segs"], r["zbp"], r["floor"], r["numbps"]), (k, j)
                    assert s["passes"] == r["passes"]
    if L < 32:                                                      # more layers than the stream holds: refused, every tile
        got = sr.read_tiles(t2ref, stream, toffs, tiles, L + 1, marks, marks)
        assert not any(v["ok"] for v in got)


def test_read_tiles_head_rules(oracle):
    """the refusal rules of the tile-part head one by one, on geometry a (tile-part 1 of 6)"""
    import t2ref
    _, tiles, datas, nbs, Rs, _ = sr.tables("a")
    stream, toffs, loffs, kept = sr.base_stream("a", "L2-empty0-tile", True)
    a = toffs[1]

    def verdicts(edit, offs=toffs, n=None):
        bad = bytearray(stream)
        edit(bad)
        return sr.read_tiles(t2ref, bytes(bad[:n]), offs, tiles, 2, True, True)

    def setb(i, v):
        return lambda bad: bad.__setitem__(a + i, v)
    for edit in (setb(0, 0xFE), setb(1, 0x91), setb(3, 11), setb(5, 2), setb(13, 0x94), setb(6, 0x40)):
        with_offs, serial = verdicts(edit), verdicts(edit, None)
        assert [v["ok"] for v in with_offs] == [True, False, True, True, True, True], [v["why"] for v in with_offs]
        assert [v["ok"] for v in serial] == [True] + [False] * 5
        assert with_offs[1]["why"].startswith("head") or "run out" in with_offs[1]["why"]
    # a Psot that runs into the next tile-part: with offsets the tile is read (what follows the layers read is ignored), without them the next one is lost
    def psot(v):
        return lambda bad: bad.__setitem__(slice(a + 6, a + 10), v.to_bytes(4, "big"))
    grow = toffs[2] - a + 3
    assert [v["ok"] for v in verdicts(psot(grow))] == [True] * 6
    assert [v["ok"] for v in verdicts(psot(grow), None)] == [True, True] + [False] * 4
    assert [v["ok"] for v in verdicts(psot(13))] == [True, False, True, True, True, True]
    # TPsot / TNsot are not looked at
    assert sr.frame_ok(verdicts(setb(10, 7))) and sr.frame_ok(verdicts(setb(11, 9)))
    # Psot = 0 in the last tile-part: "to the end of the stream"
    def psot0(bad):
        bad[toffs[5] + 6:toffs[5] + 10] = bytes(4)
    assert sr.frame_ok(verdicts(psot0)) and sr.frame_ok(verdicts(psot0, None))
    # a stream cut inside tile-part 4: the parts before it are read, with and without offsets
    n = toffs[4] + 20
    for offs in (toffs, None):
        assert [v["ok"] for v in verdicts(lambda bad: None, offs, n)] == [True] * 4 + [False] * 2
    # hostile offsets: each refuses its own tile only
    for hostile in (len(stream), len(stream) + 12345, 2 ** 62, 2 ** 64 - 1, len(stream) - 13):
        offs = list(toffs); offs[2] = hostile
        assert [v["ok"] for v in verdicts(lambda bad: None, offs)] == [True, True, False, True, True, True]


# ---- the damaged copies ---------------------------------------------------------------------------------------------------------------------
def _all_read(c):
    return all(v["ok"] for v in c["verdicts"])


def _dropped(c):
    return [j for v in c["verdicts"] for j, s in v["blocks"].items() if s["dropped"]]


@pytest.mark.parametrize("reader", sorted(sr.READERS))
def test_body_damage_reads_to_the_same_tables(oracle, reader):
    import t2ref
    fam, k = sr.READERS[reader]
    _, tiles, datas, nbs, Rs, _ = sr.tables("a")
    seen = 0
    for c in sr.damaged_copies(reader):
        if c["kind"] != "body":
            continue
        stream, toffs, loffs, kept = sr.base_stream("a", fam, c["marks"])
        intact = sr.read_tiles(t2ref, stream, toffs, tiles, k, c["marks"], c["marks"])
        assert c["stream"] != stream and c["n"] == len(stream) and sr.frame_ok(c["verdicts"])
        for v, w in zip(c["verdicts"], intact):
            assert v["blocks"] == w["blocks"]
        assert sr.block_tables(c["stream"], c["verdicts"]) != sr.block_tables(stream, intact)       # (the codewords did change)
        seen += 1
    assert seen >= sr.COPIES // len(sr.KINDS)


def test_damaged_copies_verdict_shares(oracle):
    """the comparison of the GPU test is not vacuous: enough frames accepted, enough refused, a dropped block in a frame otherwise read, frames
    with tiles read beside tiles refused.  The counts are printed (pytest -s) for the pull request's notes."""
    copies = [c for r in sorted(sr.READERS) for c in sr.damaged_copies(r)]
    assert len(copies) == len(sr.READERS) * (sr.COPIES + sr.CRAFTED) and {c["kind"] for c in copies} == set(sr.KINDS) | {"passes"}
    for c in copies:
        if c["kind"] == "passes":                                    # the crafted ones: everything read, exactly that block dropped
            assert _all_read(c) and _dropped(c) == [c["block"]] and not sr.frame_ok(c["verdicts"])
    hdr = [c for c in copies if c["kind"] in ("header", "head64", "runs")]
    accepted = sum(_all_read(c) for c in hdr)
    over31 = [(r, c["it"], _dropped(c)) for r in sorted(sr.READERS) for c in sr.damaged_copies(r) if _all_read(c) and _dropped(c)]
    mixed = [(r, c["it"]) for r in sorted(sr.READERS) for c in sr.damaged_copies(r) if any(v["ok"] for v in c["verdicts"]) and not _all_read(c)]
    zero_len = [(r, c["it"]) for r in sorted(sr.READERS) for c in sr.damaged_copies(r) if any(v["ok"] and v["zero_len"] for v in c["verdicts"])]
    stopped = [(r, c["it"]) for r in sorted(sr.READERS) for c in sr.damaged_copies(r) if any(not v["ok"] and v["done"] for v in c["verdicts"])]
    print("tiles read with a contribution of length 0: %d frames %s; chains that stopped after their first packet: %d frames" % (len(zero_len), zero_len[:12], len(stopped)))
    assert len(zero_len) >= 1 and len(stopped) >= 10
    print("header/head64/runs: %d copies, %d accepted, %d refused; dropped for > 31 planes: %s; tiles read beside tiles refused: %d frames %s"
          % (len(hdr), accepted, len(hdr) - accepted, over31, len(mixed), mixed[:12]))
    assert 4 * accepted >= len(hdr) and 4 * (len(hdr) - accepted) >= len(hdr)
    assert len(over31) >= 1
    assert len(mixed) >= 10
    assert all(not _all_read(c) for c in copies if c["kind"] in ("cut", "noise"))


def test_pass_reader_copies_meet_the_vacuity_conditions(oracle):
    """the pass reader's copies alone, by the yardstick alone: what tests/test_gpu_stream_readers.py::test_damaged_streams[pfloors] counts on the device"""
    import pass_stream_cases as ps
    seen = {"ok": 0, "refused": 0, "dropped": 0, "mixed": 0, "body": 0, "partial": 0}
    for c in sr.damaged_copies("pfloors"):
        good = sr.frame_ok(c["verdicts"])
        seen["ok" if good else "refused"] += 1
        seen["mixed"] += int(any(v["ok"] for v in c["verdicts"]) and not _all_read(c))
        seen["dropped"] += int(_all_read(c) and not good)
        tab = sr.block_tables_pass(c["stream"][:c["n"]], c["verdicts"])
        for j, (data, pfloor, numbps) in tab.items():                 # the invariants the device's tables must keep hold in the yardstick's
            assert numbps <= 31 and pfloor <= max(3 * numbps - 3, 0) and (data or (numbps, pfloor) == (0, 0)), (c["it"], j)
        if c["kind"] == "body":
            seen["body"] += 1
            seen["partial"] += int(bool(ps.partial_blocks(tab)))
    print("pfloors: %s" % seen)
    assert seen["ok"] >= 20 and seen["refused"] >= 20 and seen["dropped"] >= 1 and seen["mixed"] >= 10 and seen["body"] >= 17 and seen["partial"] >= 10, seen


def test_pass_record_rules(oracle):
    """read_tiles' pass-aware record on the two headers no writer makes, and on rule 5"""
    import pass_cases as pc
    import pass_stream_cases as ps
    import t2ref
    for geom in sorted(sr.GEOMETRIES):
        T = ps.pass_tables(geom)
        stream, toffs, F = ps.pass_stream(geom, "P-claims", True)
        got = sr.read_tiles(t2ref, stream, toffs, T["tiles"], 1, True, True)
        assert sr.frame_ok(got)
        blocks = {j: s for v in got for j, s in v["blocks"].items()}
        kinds = set()
        for j, kind in F["claims"].items():
            s, nb = blocks[j], T["nbs"][j]
            kinds.add(kind)
            if kind == "passes":                                     # a. s > 0 below plane 0
                assert s["passes"] in (3 * nb - 1, 3 * nb) and s["zbp"] == 31 - nb
                assert (s["floor"], s["pfloor"], s["numbps"]) == (0, 0, nb), (geom, j)
            else:                                                    # b. mb - zbp < coded
                assert s["passes"] == 3 * nb - 4 and s["zbp"] == 31 - nb + 2 and 31 - s["zbp"] < (s["passes"] + 2) // 3
                assert (s["floor"], s["pfloor"], s["numbps"]) == (0, 0, nb - 1), (geom, j)
        assert kinds == {"passes", "zbp"}
        for j, s in blocks.items():                                  # every other block: the header round trip of pass_cases
            if j not in F["claims"] and s["segs"]:
                assert (s["pfloor"], s["numbps"]) == (pc.pfloor_of(T["nbs"][j], F["qs"][j]), T["nbs"][j]), (geom, j)
            if not s["segs"]:
                assert (s["floor"], s["pfloor"], s["numbps"]) == (0, 0, 0)
    for c in sr.damaged_copies("pfloors"):                           # rule 5 on the crafted copies
        if c["kind"] == "passes":
            s = [v["blocks"][c["block"]] for v in c["verdicts"] if c["block"] in v["blocks"]][0]
            assert s["dropped"] and (s["floor"], s["pfloor"], s["numbps"]) == (0, 0, 0) and s["passes"] > 91


# ---- j2k_tile_parts_keep_layers -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codestream():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "go-jpeg2000_amd")])
    from j2kgfx import codestream as cs
    return cs


@pytest.mark.parametrize("fam", ["L32-mod5", "L32-all-in-0"])
@pytest.mark.parametrize("geom", sorted(sr.GEOMETRIES))
def test_keep_layers_on_32_layer_streams(oracle, codestream, geom, fam):
    import t2ref
    _, tiles, datas, nbs, Rs, _ = sr.tables(geom)
    for marks in MARKS:
        stream, toffs, loffs, kept = sr.base_stream(geom, fam, marks)
        for k in (1, 16, 32):
            want, wtoffs = lc.keep_layers(stream, toffs, loffs, 32, k)
            got, gtoffs = codestream.keep_layers(stream, toffs, loffs, k)
            assert got == want and [int(x) for x in gtoffs] == wtoffs, (marks, k)
            cut = sr.read_tiles(t2ref, got, wtoffs, tiles, k, marks, marks)
            full = sr.read_tiles(t2ref, stream, toffs, tiles, k, marks, marks)
            assert sr.frame_ok(cut) and sr.block_tables(got, cut) == sr.block_tables(stream, full)
            if k < 32:
                assert not any(v["ok"] for v in sr.read_tiles(t2ref, got, wtoffs, tiles, k + 1, marks, marks))


def _keep_raw(cs, toffs, loffs, nt, L, keep, cap):
    """the C call with a caller-owned, sentinel-filled `out` of cap bytes -> (status, out_len, out, out_tile_offs)"""
    from j2kgfx import _lib
    d = np.frombuffer(bytes(cs), np.uint8).copy()
    t = np.asarray([int(x) for x in toffs], dtype=np.uint64)
    lo = np.asarray([int(x) for x in loffs], dtype=np.uint64)
    out = np.full(max(cap, 1) + 16, 0xA5, np.uint8)
    ot = np.full(nt + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    n = C.c_size_t(0xDEAD)
    r = _lib.lib().j2k_tile_parts_keep_layers(d.ctypes.data_as(C.c_void_p), C.c_size_t(d.size), t.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), int(nt), int(L),
                                             int(keep), out.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(n), ot.ctypes.data_as(C.c_void_p))
    return int(r), int(n.value), out, ot


def test_keep_layers_refuses_hostile_offset_tables(oracle, codestream):
    from j2kgfx import _lib
    stream, toffs, loffs, kept = sr.base_stream("a", "L32-mod5", True)
    nt, L, total = len(toffs) - 1, 32, len(stream)
    keep = 4
    r, n, out, ot = _keep_raw(stream, toffs, loffs, nt, L, keep, total)
    want, wtoffs = lc.keep_layers(stream, toffs, loffs, L, keep)
    assert r == _lib.OK and n == len(want) and bytes(out[:n]) == want and ot.tolist() == wtoffs and bool((out[n:] == 0xA5).all())
    e = 2 * L + keep - 1                                             # the end of layer keep - 1 of tile 2
    hostile = {
        "end before its tile start + 14": (toffs, {e: toffs[2] + 13}),
        "end before its tile start": (toffs, {e: toffs[2] - 1}),
        "end beyond len": (toffs[:3] + [total] * (nt - 2), {e: total + 1}),
        "end beyond the next tile's start": (toffs, {e: toffs[3] + 1}),
        "end >= 2^63": (toffs, {e: 2 ** 63}),
        "end 2^64 - 1": (toffs, {e: 2 ** 64 - 1}),
        "tile start not at SOT": (toffs[:2] + [toffs[2] + 1] + toffs[3:], {}),
        "tile start beyond len": (toffs[:2] + [total + 5] + toffs[3:], {}),
    }
    for why, (to, patch) in hostile.items():
        lo = list(loffs)
        for i, v in patch.items():
            lo[i] = v
        r, n, out, ot = _keep_raw(stream, to, lo, nt, L, keep, total)
        assert r == _lib.ERR_INVALID_ARG, why
        assert bool((out == 0xA5).all()) and bool((ot == 0xA5A5A5A5A5A5A5A5).all()), why


def test_keep_layers_capacity(oracle, codestream):
    from j2kgfx import _lib
    stream, toffs, loffs, kept = sr.base_stream("a", "L32-mod5", False)
    nt, L = len(toffs) - 1, 32
    for keep in (1, 16, 32):
        need = len(lc.keep_layers(stream, toffs, loffs, L, keep)[0])
        r, n, out, ot = _keep_raw(stream, toffs, loffs, nt, L, keep, need - 1)
        assert r == _lib.ERR_CAPACITY and n == need, keep
        assert bool((out == 0xA5).all()), keep
        r, n, out, ot = _keep_raw(stream, toffs, loffs, nt, L, keep, need)
        assert r == _lib.OK and n == need and bool((out[need:] == 0xA5).all())
