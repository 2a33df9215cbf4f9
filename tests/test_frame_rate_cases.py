"""CPU: tests/frame_rate_cases.py, the definition of rate control on batch plans ("frame f gets the cuts it would get alone under its own budget"),
checked against itself and against the single-frame definitions it is made of; the frame-range builder of the plan (plan_tables.h:
frame_job_ranges) run under sanitizers by a stand-alone program and compared with frame_ranges; the new entry points declared and bound."""
import os
import re
import subprocess

import pytest

import frame_rate_cases as fr
import layer_cases as lc
import pass_cases as pc
import quality_cases as qc
import rate_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-jpeg2000_amd", "csrc")
# (include/j2kgfx.h names these six; each takes the plan and at least one more argument)
NEW_SYMBOLS = ("j2k_plan_set_rate_per_frame", "j2k_plan_rate_frames", "j2k_plan_rate_allocate_frames", "j2k_plan_rate_allocate_quality_frames",
               "j2k_plan_encode_frame_pixels_rate_frames", "j2k_encode_pixels_host_rate_frames")


def test_symbols_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "j2kgfx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from j2kgfx import _lib
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), "include/j2kgfx.h does not declare %s" % name
        assert name in _lib.SYMBOLS
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) >= 2, name
    assert len(L.j2k_plan_rate_allocate_frames.argtypes) == 9 and len(L.j2k_plan_rate_allocate_quality_frames.argtypes) == 10
    assert len(L.j2k_plan_encode_frame_pixels_rate_frames.argtypes) == 14 and len(L.j2k_encode_pixels_host_rate_frames.argtypes) == 17


# ---- the definition on random tables -----------------------------------------------------------------------------------------------------------
# three frames of unequal size: fewer than 64 blocks, not a multiple of 64, more than 1024 (a thread of the workgroup then owns two blocks)
RANGES = [(0, 40), (40, 1100), (1140, 131)]
N = 1271


@pytest.fixture(scope="module")
def tables():
    return qc.random_tables(77, N)


def _total(Rs, nbs, a, c):
    return sum(int(Rs[j][nbs[j]]) for j in range(a, a + c))


def test_frame_ranges_of_a_tile_list():
    assert fr.frame_ranges([0, 0, 1, 2, 2, 3], 2) == [(0, 3), (3, 3)]
    assert fr.frame_ranges([0, 0, 1, 2, 2, 3], 1) == [(0, 2), (2, 1), (3, 2), (5, 1)]
    assert fr.frame_ranges([0, 0, 0], 1) == [(0, 3)]
    assert fr.frame_ranges([1, 1], 1) == [(0, 0), (0, 2)]                    # a frame without blocks
    assert fr.frame_ranges([], 2, nframes=3) == [(0, 0)] * 3
    with pytest.raises(AssertionError):
        fr.frame_ranges([0, 1, 0], 1)


def test_one_frame_is_the_undivided_call(tables):
    Rs, Ds, nbs, ws = tables
    one = [(0, N)]
    total = _total(Rs, nbs, 0, N)
    for b in (fr.INF, total // 2, total // 10, 0):
        assert fr.allocate_frames(Rs, Ds, nbs, ws, one, b) == (lambda k, c: (k, [c]))(*rc.allocate(Rs, Ds, nbs, ws, b))
        assert fr.allocate_frames(Rs, Ds, nbs, ws, one, [b]) == fr.allocate_frames(Rs, Ds, nbs, ws, one, b)
    ladder = [total // 10, total // 3, fr.INF]
    k, c = lc.allocate_layers(Rs, Ds, nbs, ws, ladder)
    assert fr.allocate_layers_frames(Rs, Ds, nbs, ws, one, ladder) == (k, [[x] for x in c])
    start = qc.weighted_distortion(Ds, ws, [0] * N)
    targets = [start / 4, start / 64, 0.0]
    k, c, a = qc.allocate_quality_layers(Rs, Ds, nbs, ws, targets)
    gk, gc, ga = fr.allocate_quality_layers_frames(Rs, Ds, nbs, ws, one, targets)
    assert (gk, gc) == (k, [[x] for x in c]) and [qc.float_bits(x[0]) for x in ga] == [qc.float_bits(x) for x in a]


def test_a_frame_sees_only_its_own_budget(tables):
    Rs, Ds, nbs, ws = tables
    tot = [_total(Rs, nbs, a, c) for a, c in RANGES]
    base = [tot[0] // 2, tot[1] // 5, tot[2] // 3]
    k0, c0 = fr.allocate_frames(Rs, Ds, nbs, ws, RANGES, base)
    for f, (a, c) in enumerate(RANGES):
        assert (k0[a:a + c], c0[f]) == rc.allocate(Rs[a:a + c], Ds[a:a + c], nbs[a:a + c], ws[a:a + c], base[f])
        assert c0[f] <= base[f]
    # changing frame 1's budget changes nothing of frames 0 and 2
    k1, c1 = fr.allocate_frames(Rs, Ds, nbs, ws, RANGES, [base[0], tot[1] // 50, base[2]])
    a1, n1 = RANGES[1]
    assert k1[:a1] == k0[:a1] and k1[a1 + n1:] == k0[a1 + n1:] and (c1[0], c1[2]) == (c0[0], c0[2])
    assert k1[a1:a1 + n1] != k0[a1:a1 + n1] and c1[1] <= tot[1] // 50
    # a scalar is every frame under the same budget; a budget that holds a frame's full lengths cuts nothing of it
    b = min(tot) // 2 + 1
    ks, cs = fr.allocate_frames(Rs, Ds, nbs, ws, RANGES, b)
    assert (ks, cs) == fr.allocate_frames(Rs, Ds, nbs, ws, RANGES, [b] * 3) and all(x <= b for x in cs)
    kf, cf = fr.allocate_frames(Rs, Ds, nbs, ws, RANGES, [0, fr.INF, tot[2] // 2])
    assert cf[0] == 0 and cf[1] == tot[1] and kf[a1:a1 + n1] == [int(x) for x in nbs[a1:a1 + n1]] and cf[2] <= tot[2] // 2
    # the frames' lambdas differ: one search over all blocks is another choice
    kall, _ = rc.allocate(Rs, Ds, nbs, ws, sum(base))
    assert kall != k0


def test_targets_per_frame_and_the_order_of_the_sum(tables):
    Rs, Ds, nbs, ws = tables
    start = [qc.weighted_distortion(Ds[a:a + c], ws[a:a + c], [0] * c) for a, c in RANGES]
    T = [start[0] / 8, start[1] / 100, 0.0]
    k0, c0, a0 = fr.allocate_quality_frames(Rs, Ds, nbs, ws, RANGES, T)
    for f, (a, c) in enumerate(RANGES):
        ps, b, s = qc.allocate_quality(Rs[a:a + c], Ds[a:a + c], nbs[a:a + c], ws[a:a + c], T[f])
        assert (k0[a:a + c], c0[f]) == (ps, b) and qc.float_bits(a0[f]) == qc.float_bits(s)
        assert a0[f] <= T[f]
        # the sum starts again at the frame's first block: frame-LOCAL thread ownership
        assert qc.float_bits(a0[f]) == qc.float_bits(qc.weighted_distortion(Ds[a:a + c], ws[a:a + c], ps))
    k1, c1, a1 = fr.allocate_quality_frames(Rs, Ds, nbs, ws, RANGES, [T[0], start[1] / 3, T[2]])
    a, n = RANGES[1]
    assert k1[:a] == k0[:a] and k1[a + n:] == k0[a + n:] and k1[a:a + n] != k0[a:a + n]
    assert [qc.float_bits(x) for x in (a1[0], a1[2])] == [qc.float_bits(x) for x in (a0[0], a0[2])]
    # a ladder for every frame
    lad = [min(start) / 4, min(start) / 64, 0.0]
    kl, cl, al = fr.allocate_quality_layers_frames(Rs, Ds, nbs, ws, RANGES, lad)
    assert len(kl) == 3 and all(len(x) == 3 for x in cl) and all(al[l][f] <= lad[l] for l in range(3) for f in range(3))
    assert all(cl[l][f] <= cl[l + 1][f] for l in range(2) for f in range(3))


def test_pass_tables_per_frame():
    """the pass forms run the same functions with 3 nb - 2 points per block"""
    import numpy as np
    rng = np.random.default_rng(78)
    _, _, nbs, ws = qc.random_tables(78, 90)
    Rp, Dp = [], []
    for nb in nbs:                                          # rising R, falling D over the 3 nb - 2 points, 0 behind them
        q = pc.points(nb)
        r = np.zeros(pc.STRIDE, np.uint32); d = np.zeros(pc.STRIDE, np.uint64)
        if q:
            r[1:q + 1] = np.cumsum(rng.integers(0, 25, q))
            r[q:] = r[q]
            d[:q] = np.sort(rng.integers(1, 1 << 24, q).astype(np.uint64))[::-1]
        Rp.append(r); Dp.append(d)
    ranges = [(0, 30), (30, 60)]
    tot = [sum(int(Rp[j][pc.points(nbs[j])]) for j in range(a, a + c)) for a, c in ranges]
    k, c = fr.allocate_frames_passes(Rp, Dp, nbs, ws, ranges, [tot[0] // 2, tot[1] // 4])
    for f, (a, n) in enumerate(ranges):
        pts = [pc.points(nb) for nb in nbs[a:a + n]]
        assert (k[a:a + n], c[f]) == rc.allocate(Rp[a:a + n], Dp[a:a + n], pts, ws[a:a + n], [tot[0] // 2, tot[1] // 4][f])
        assert all(x <= p for x, p in zip(k[a:a + n], pts))
    kq, cq, aq = fr.allocate_quality_frames_passes(Rp, Dp, nbs, ws, ranges, [1.0e6, 0.0])
    assert aq[0] <= 1.0e6 and aq[1] == 0.0 and cq[1] == tot[1] - sum(int(Rp[j][pc.points(nbs[j])]) for j in range(30, 90) if ws[j] == 0.0)


def test_psnr_target_is_one_frames():
    assert fr.psnr_distortion(130, 70, 3, 8, True, 0, 40.0) * 3 == pytest.approx(qc.psnr_distortion(130, 210, 3, 8, True, 0, 40.0), rel=1e-15)


# ---- the frame-range builder under sanitizers --------------------------------------------------------------------------------------------------
def test_frame_range_builder_under_sanitizers(tmp_path, oracle):
    exe = str(tmp_path / "frame_ranges_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "frame_ranges_main.cpp"), os.path.join(CSRC, "plan_tables.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]          # sanitizer reports, invariant violations, tables the builder should have refused
    runs, cur = {}, None
    for line in out.stdout.splitlines():
        if line.startswith("@ "):
            cur = runs.setdefault(line[2:], dict(ranges=[]))
        elif line.startswith("tiles "):
            w = line.split()
            cur["tiles"], cur["tpf"], cur["blocks"] = int(w[1]), int(w[2]), int(w[4])
        elif line.startswith("tile"):
            cur["tile"] = [int(x) for x in line.split()[1:]]
        elif line.startswith("range "):
            cur["ranges"].append(tuple(int(x) for x in line.split()[1:]))
    assert list(runs) == [g[0] for g in fr.RANGE_GEOMETRIES] + ["end"]
    for name, W, H, rows, ncomp, nres, cb, tile in fr.RANGE_GEOMETRIES:
        got = runs[name]
        ntiles, tpf = fr.tiles_of_geometry(W, H, rows, tile)
        F = H // rows if rows else 1
        assert (got["tiles"], got["tpf"]) == (ntiles, tpf), name
        # the plan's block list is the oracle's enumeration of every tile, frame after frame
        want_tiles = fr.expected_block_tiles(oracle, W, H, rows, ncomp, nres, cb, tile)
        assert got["tile"] == want_tiles and got["blocks"] == len(want_tiles), name
        assert got["ranges"] == fr.frame_ranges(want_tiles, tpf, F), name
        assert len(got["ranges"]) == F and sum(c for _, c in got["ranges"]) == got["blocks"]
        if F > 1:                                           # equal frames: equal counts
            assert len({c for _, c in got["ranges"]}) == 1, name
    assert runs["tiled_batch2_partial_rows"]["tpf"] == 6 and runs["one_sample_high"]["ranges"] == [(i * runs["one_sample_high"]["blocks"] // 3, runs["one_sample_high"]["blocks"] // 3) for i in range(3)]
