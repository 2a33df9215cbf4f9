"""GPU: the pass reader (decode_tile_parts(pfloors=True), decode_frame_pixels / decode_pixels_host(pass_cuts=True)) and the pass-stopped block decoder
(decode_blocks(pfloors=)) on intact streams this library's encoder never writes, against tests/pass_stream_cases.py bit for bit: pass cuts no
allocator returns, bodies longer than the cut needs, headers that claim more than the block holds, blocks of 31 planes, and launches whose blocks
stop at different passes.  The tables are the yardstick's (stream_reader_cases.read_tiles), the coefficients are decode_passes of the bytes it reads --
a Python decoder that keeps a record of the partial plane, where the device reads the midpoint off the magnitude.  The damaged copies and the state
a read leaves on a plan are in tests/test_gpu_stream_readers.py (reader "pfloors"), whose plans and helpers this file shares."""
import numpy as np
import pytest

import area_cases as ac
import mallat_cases as mc
import pass_cases as pc
import pass_stream_cases as ps
import stream_reader_cases as sr
import test_gpu_rate_frames as rf
import test_gpu_stream_readers as gs

pytestmark = pytest.mark.gpu
env = gs.env
HOST_FAMILY = "P-long"                                                # the family that also goes through decode_pixels_host


def _pixels(orc, case, ctiles, wins, coeffs, reduce):
    """the oracle's inverse transform of the frame whose block j holds coeffs[j]"""
    W, H, Cn, prec, tile, nres = case
    cut = [t.copy() for t in ctiles]
    for j, (t, c, ys, xs) in enumerate(wins):
        cut[t][c, ys, xs] = coeffs[j]
    return mc.pixels(orc, mc.inverse_frame(orc, cut, W, H, tile, prec, nres, reduce=reduce), prec)


def _read_and_decode(torch, plan, T, stream, toffs, marks, tab, coeffs, wins, tag):
    """decode_tile_parts(pfloors=True) with and without tile_offs: the yardstick's tables; decode_blocks(pfloors=) + place_blocks: decode_passes"""
    cs = gs._in_buffer(torch, plan, stream)
    d_toffs = gs._dev(torch, plan, toffs, np.int64)
    for with_offs in (False, True):
        o, l, nb, pf = plan.decode_tile_parts(cs, len(stream), tile_offs=d_toffs if with_offs else None, sop=marks, eph=marks, pfloors=True)
        plan.frame_status()
        ho, hl, hnb, hpf = gs._host_tables(plan, o, l, nb, pf)
        gs._invariants_pass(ho, hl, hnb, hpf, len(stream), tag)
        gs._check_tables(tab, np.frombuffer(stream, np.uint8), ho, hl, hnb, hpf, tag)
        gs._check_placed(plan, gs._decode_and_place(plan, cs, o, l, nb, pf, passes=True), T["ctiles"], wins, coeffs, tag)
    return cs, d_toffs, (o, l, nb, pf)


# ---- 1. foreign but intact streams ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("marks", gs.MARKS, ids=gs.MARK_IDS)
@pytest.mark.parametrize("fam", ps.PASS_FAMILIES)
@pytest.mark.parametrize("geom", gs.GEOMS)
def test_pass_reader_on_foreign_streams(env, geom, fam, marks):
    import t2ref
    torch, orc, ctx, get_plan = env
    plan = get_plan(geom)
    case = sr.GEOMETRIES[geom]["case"]
    W, H, Cn, prec, tile, nres = case
    T = ps.pass_tables(geom)
    stream, toffs, F = ps.pass_stream(geom, fam, marks)
    total = len(stream)
    verdicts = sr.read_tiles(t2ref, stream, toffs, T["tiles"], 1, marks, marks)
    assert sr.frame_ok(verdicts)
    tab = sr.block_tables_pass(stream, verdicts)
    wins = rf._windows(plan, T["ctiles"], Cn)
    coeffs = {0: ps.expected_coeffs(T, tab), 1: ps.expected_coeffs(T, tab, skip_planes=1)}
    cs, d_toffs, _ = _read_and_decode(torch, plan, T, stream, toffs, marks, tab, coeffs[0], wins, (geom, fam, marks))
    # pixels: the whole frame, a coarser resolution, a plane skipped, a rectangle
    bpp = ac.bytes_per_pixel(Cn, prec)
    area = gs.AREAS[geom]
    for r, k, a in ((0, 0, None), (1, 0, None), (0, 1, None), (0, 0, area), (1, 1, area)):
        assert r in mc.admissible(W, H, tile, nres)
        exp = _pixels(orc, case, T["ctiles"], wins, coeffs[k], r)
        if a is not None:
            exp = ac.crop(exp, a, r, bpp)
        back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, total, back, tile_offs=d_toffs if (r + k) & 1 else None, sop=marks, eph=marks, reduce=r, skip_planes=k, area=a, pass_cuts=True)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp), (geom, fam, marks, r, k, a)
        if fam == HOST_FAMILY:
            host = plan.decode_pixels_host(stream, exp.shape, sop=marks, eph=marks, reduce=r, skip_planes=k, area=a, pass_cuts=True)
            assert np.array_equal(host, exp), (geom, fam, marks, r, k, a, "host")
    # the older reader on the same stream: the whole planes of every header, the passes inside a plane ignored
    exp = _pixels(orc, case, T["ctiles"], wins, ps.whole_plane_coeffs(T, sr.block_tables(stream, verdicts)), 0)
    back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
    plan.decode_frame_pixels(cs, total, back, sop=marks, eph=marks, truncated=True)
    plan.frame_status()
    assert np.array_equal(back.cpu().numpy(), exp), (geom, fam, marks, "truncated")


# ---- 2. blocks of 31 planes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rnd", range(ps.BIG_ROUNDS))
def test_blocks_of_31_planes_at_pass_cuts(env, rnd):
    """geometry b with blocks of 31, 1 and 0 planes, the deep ones cut at pass_stream_cases.BIG_CUTS: the reader's tables, decode_blocks(pfloors=)
    + place_blocks; then the same codewords with every pass but the last few left out (pfloors 88 ... 92: the top plane and beyond)"""
    import t2ref
    torch, orc, ctx, get_plan = env
    plan = get_plan("b")
    marks = bool(rnd & 1)
    T = ps.pass_tables("b", True)
    stream, toffs, F = ps.big_stream(rnd, marks)
    verdicts = sr.read_tiles(t2ref, stream, toffs, T["tiles"], 1, marks, marks)
    assert sr.frame_ok(verdicts)
    tab = sr.block_tables_pass(stream, verdicts)
    assert sum(numbps == 31 for _, _, numbps in tab.values()) == 3
    wins = rf._windows(plan, T["ctiles"], 1)
    cs, d_toffs, (o, l, nb, pf) = _read_and_decode(torch, plan, T, stream, toffs, marks, tab, ps.expected_coeffs(T, tab), wins, ("big", rnd))
    for f in (88, 89, 90, 91, 92):
        high = {j: (data, max(f, pfloor), numbps) for j, (data, pfloor, numbps) in tab.items()}
        d_pf = torch.maximum(pf, torch.full_like(pf, f))
        gs._check_placed(plan, gs._decode_and_place(plan, cs, o, l, nb, d_pf, passes=True), T["ctiles"], wins, ps.expected_coeffs(T, high), ("big", rnd, f))


# ---- 3. one launch, blocks that stop at different passes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,big", [("a", False), ("b", True)], ids=["a", "b-31-planes"])
def test_block_decode_mixed_pfloors(env, geom, big):
    """decode_blocks(pfloors=) on a plan of many blocks (tests/test_gpu_pass_cuts.py::test_block_decode has one block a launch): pfloors[j] random
    in 0 ... 95, values beyond the block's passes among them, blocks without bytes whose pfloors is not 0, and skip_planes beside them"""
    torch, orc, ctx, get_plan = env
    plan = get_plan(geom)
    T = ps.pass_tables(geom, big)
    datas, nbs, n = T["datas"], T["nbs"], len(T["nbs"])
    _, _, _, _, Rs, _ = sr.tables(geom, big)
    d_stream, d_offs, _, d_nbs, _ = gs._upload(torch, plan, datas, nbs, Rs)
    wins = rf._windows(plan, T["ctiles"], sr.GEOMETRIES[geom]["case"][2])
    rng = np.random.default_rng(4100 + int(big))
    pfl = [int(x) for x in rng.integers(0, 96, n)]
    lens = [len(d) for d in datas]
    for j in range(n):
        if j % 6 == 0:
            pfl[j] = pc.points(nbs[j]) + 1 + j % 4                    # beyond the block's passes: nothing to decode
        if j % 5 == 1:
            lens[j], pfl[j] = 0, max(pfl[j], 1)                       # no bytes under a pfloors that is not 0
    if big:                                                          # three blocks of 31 planes: beyond its passes, behind a MagRef pass, no bytes behind a SigProp pass
        assert [nbs[j] for j in (0, 3, 6)] == [31, 31, 31] and pfl[0] == 92
        pfl[3], pfl[6], lens[6] = 43, 44, 0
    assert any(f > pc.points(nb) for f, nb in zip(pfl, nbs)) and any(0 < f <= pc.points(nb) and f % 3 for f, nb in zip(pfl, nbs))
    d_lens, d_pf = gs._dev(torch, plan, lens, np.uint32), gs._dev(torch, plan, pfl, np.uint8)
    for skip in (0, 1):
        coeffs = {}
        for j in range(n):                                           # (a block without bytes still runs its planes: the MQ decoder reads its 0xFF fill)
            h, w = T["vs"][j].shape
            f = max(3 * skip, pfl[j])
            coeffs[j] = ps.decode_passes_cached(datas[j][:lens[j]], nbs[j], T["bands"][j], w, h, f)
            if f > pc.points(nbs[j]):
                assert not coeffs[j].any(), j
        placed = plan.place_blocks(plan.decode_blocks(d_stream, d_offs, d_lens, d_nbs, skip_planes=skip, pfloors=d_pf))
        plan.frame_status()
        gs._check_placed(plan, placed, T["ctiles"], wins, coeffs, (geom, big, skip))
