"""GPU: the closed-loop packet readers (decode_tile_parts(layers=k) / (floors=True) / (pfloors=True), decode_frame_pixels(layers=k) / (truncated=True) /
(pass_cuts=True) / (area=)) on streams this library's encoder never writes, against tests/stream_reader_cases.py bit for bit: hand-made cut families on three small
geometries, a table set with 31 bit planes, damaged copies with a verdict per tile, stale state from frame to frame on one plan, and a dense
buffer that is too small.  One context and one plan per geometry, reused across the cases on purpose: what a frame leaves in the plan's tables
is part of what is tested.  Every input is one the readers claim to read or to refuse safely."""
import numpy as np
import pytest

import area_cases as ac
import coarse_cases as cc
import layer_cases as lc
import mallat_cases as mc
import pass_cases as pc
import pass_stream_cases as ps
import stream_reader_cases as sr
import test_gpu_rate_frames as rf

pytestmark = pytest.mark.gpu
GEOMS = sorted(sr.GEOMETRIES)
MARKS = [False, True]
MARK_IDS = ["bare", "sop_eph"]
AREAS = {"a": (10, 6, 30, 20), "b": (5, 3, 40, 17), "c": (20, 9, 33, 17)}      # a, c: across tile boundaries in both directions
GUARD = 64                                                                      # elements either side of a guarded tensor


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    from j2kgfx import Context
    from j2kgfx.codec import FramePlan
    ctx = Context(0)
    plans = {}

    def plan(geom):
        if geom not in plans:
            g = sr.GEOMETRIES[geom]
            W, H, Cn, prec, tile, nres = g["case"]
            plans[geom] = FramePlan(W, H, Cn, precision=prec, lossless=True, quality=0, num_resolutions=nres, cb=(g["cb"], g["cb"]), tile=tile, coder=0, ctx=ctx,
                                    mallat=True, dequantize=False)
        return plans[geom]
    yield torch, orc, ctx, plan
    for p in plans.values():
        p.close()
    ctx.close()


# ---- helpers --------------------------------------------------------------------------------------------------------------------------------
def _dev(torch, plan, a, dtype):
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    if dtype == np.uint32:
        a = a.view(np.int32)
    if dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).to(plan.device)


def _upload(torch, plan, datas, nbs, Rs):
    """the yardstick's tables as the stage encode takes them: (stream, offs, lens, numbps, rate)"""
    n = len(datas)
    assert n == int(plan.info.blocks)
    rate = np.zeros((n, 32), np.uint32)
    for j in range(n):
        rate[j, :nbs[j] + 1] = Rs[j]
        rate[j, nbs[j] + 1:] = Rs[j][nbs[j]]
    offs = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64)
    d_stream = torch.from_numpy(np.frombuffer(b"".join(datas) + bytes(64), np.uint8).copy()).to(plan.device)
    return (d_stream, _dev(torch, plan, offs, np.int64), _dev(torch, plan, [len(d) for d in datas], np.uint32), _dev(torch, plan, nbs, np.uint8),
            _dev(torch, plan, rate.reshape(-1), np.uint32))


def _guarded(torch, plan, n, dtype, fill):
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=plan.device)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def _in_buffer(torch, plan, stream, guard=4096):
    """the stream inside a larger zeroed device tensor, guard bytes either side -> the view that starts at the stream"""
    buf = torch.zeros(len(stream) + 2 * guard, dtype=torch.uint8, device=plan.device)
    buf[guard:guard + len(stream)] = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(plan.device)
    return buf[guard:]


def _status(plan):
    from j2kgfx import J2KError, _lib
    try:
        plan.frame_status()
        return _lib.OK
    except J2KError as e:
        return e.status


def _host_tables(plan, offs, lens, numbps, floors):
    n = int(plan.info.blocks)
    return (offs.cpu().numpy()[:n].astype(np.uint64), lens.cpu().numpy().view(np.uint32)[:n].astype(np.uint64), numbps.cpu().numpy()[:n].astype(np.int64),
            floors.cpu().numpy()[:n].astype(np.int64))


def _invariants(o, l, nb, fl, size, tag):
    assert ((o + l) <= np.uint64(size)).all() and (o <= np.uint64(size)).all(), tag
    assert (nb <= 31).all() and (fl <= nb).all(), tag
    assert ((nb == 0) & (fl == 0))[l == 0].all(), tag


def _invariants_pass(o, l, nb, pf, size, tag):
    """the pass reader's: pfloors <= max(3 numbps - 3, 0) in the place of floors <= numbps"""
    assert ((o + l) <= np.uint64(size)).all() and (o <= np.uint64(size)).all(), tag
    assert (nb <= 31).all() and (pf <= np.maximum(3 * nb - 3, 0)).all(), tag
    assert ((nb == 0) & (pf == 0))[l == 0].all(), tag


def _check_tables(tab, src, o, l, nb, fl, tag):
    """every block of `tab` ({block: (codeword, floor, numbps)}) has that entry in the device's tables, its bytes in src at its offset"""
    for j, (data, floor, numbps) in tab.items():
        assert (int(l[j]), int(fl[j]), int(nb[j])) == (len(data), floor, numbps), (tag, j)
        assert bytes(src[int(o[j]):int(o[j]) + len(data)]) == data, (tag, j)


def _block_coeffs(orc, plan, tab):
    """{block: int32 [h, w]}: the oracle's decode of every block's codeword in `tab`, coarsened at its floor (an empty block: zeros)"""
    out = {}
    for j, b in enumerate(plan.blocks()):
        w, h = int(b["w"]), int(b["h"])
        if j not in tab or not tab[j][0]:
            out[j] = np.zeros((h, w), np.int32)
            continue
        data, floor, numbps = tab[j]
        out[j] = cc.coarse(orc.t1_decode(np.frombuffer(data, np.uint8), numbps, int(b["band"]), w, h), floor)
    return out


def _check_placed(plan, placed, ctiles, wins, coeffs, tag):
    hp = placed.cpu().numpy()
    exp = [np.zeros_like(t) for t in ctiles]
    mask = [np.zeros(t.shape, bool) for t in ctiles]
    for j, (t, c, ys, xs) in enumerate(wins):
        exp[t][c, ys, xs] = coeffs[j]
        mask[t][c, ys, xs] = True
    for t_, c_, _x0, _y0, w_, h_, off in (tuple(int(v) for v in row) for row in plan.planes()):
        got = hp[off:off + w_ * h_].reshape(h_, w_)
        assert np.array_equal(got[mask[t_][c_]], exp[t_][c_][mask[t_][c_]]), (tag, t_, c_)


def _decode_and_place(plan, src, offs, lens, numbps, floors, sync=True, passes=False):
    """decode_blocks + place_blocks; sync: frame_status() (it raises what the calls found) before the caller reads the result; passes: `floors`
    counts coding passes (decode_blocks(pfloors=))"""
    placed = plan.place_blocks(plan.decode_blocks(src, offs, lens, numbps, **({"pfloors": floors} if passes else {"floors": floors})))
    if sync:
        plan.frame_status()
    return placed


def _yard_floors(tab, nbs):
    """the floor every block is decoded at, for the pixel expectation: an empty block loses all its planes"""
    return [tab[j][1] if tab[j][0] else nbs[j] for j in range(len(nbs))]


# ---- 1. the writer ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("marks", MARKS, ids=MARK_IDS)
@pytest.mark.parametrize("fam", sr.FAMILIES)
@pytest.mark.parametrize("geom", GEOMS)
def test_writer_writes_the_foreign_cuts(env, geom, fam, marks):
    import t2ref
    torch, orc, ctx, get_plan = env
    plan = get_plan(geom)
    _, tiles, datas, nbs, Rs, _ = sr.tables(geom)
    want, wtoffs, wloffs, kept = sr.base_stream(geom, fam, marks)
    L = len(kept)
    d_stream, d_offs, d_lens, d_nbs, d_rate = _upload(torch, plan, datas, nbs, Rs)
    cs, toffs, loffs = plan.encode_tile_parts(d_stream, d_offs, d_lens, d_nbs, sop=marks, eph=marks, kept=_dev(torch, plan, kept, np.uint8), rate=d_rate, layers=L)
    plan.frame_status()
    assert toffs.cpu().numpy().tolist() == wtoffs and loffs.cpu().numpy().tolist() == wloffs
    assert bytes(cs.cpu().numpy()[:wtoffs[-1]]) == want
    if L == 1:
        one, otoffs = plan.encode_tile_parts(d_stream, d_offs, d_lens, d_nbs, sop=marks, eph=marks, kept=_dev(torch, plan, kept[0], np.uint8), rate=d_rate)
        plan.frame_status()
        assert otoffs.cpu().numpy().tolist() == wtoffs
        assert bytes(one.cpu().numpy()[:wtoffs[-1]]) == lc.compose_kept(t2ref, tiles, datas, nbs, Rs, kept[0], marks, marks) == want


# ---- 2. the readers on intact foreign streams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("marks", MARKS, ids=MARK_IDS)
@pytest.mark.parametrize("fam", sr.FAMILIES)
@pytest.mark.parametrize("geom", GEOMS)
def test_readers_on_foreign_streams(env, geom, fam, marks):
    import t2ref
    torch, orc, ctx, get_plan = env
    plan = get_plan(geom)
    g = sr.GEOMETRIES[geom]
    W, H, Cn, prec, tile, nres = g["case"]
    _, tiles, datas, nbs, Rs, ctiles = sr.tables(geom)
    stream, toffs, loffs, kept = sr.base_stream(geom, fam, marks)
    L, n, total = len(kept), len(nbs), len(stream)
    wins = rf._windows(plan, ctiles, Cn)
    cs = _in_buffer(torch, plan, stream)
    d_toffs = _dev(torch, plan, toffs, np.int64)
    bpp = ac.bytes_per_pixel(Cn, prec)
    for k in [k for k in sr.LAYER_COUNTS if k <= L]:
        verdicts = sr.read_tiles(t2ref, stream, toffs, tiles, k, marks, marks)
        assert sr.frame_ok(verdicts)
        tab = sr.block_tables(stream, verdicts)
        want = sr.expected(Rs, nbs, kept, k)
        assert all(tab[j][0] == datas[j][:want[j][4]] for j in range(n))                     # the segments end to end: data[:R[Q]]
        coeffs = {j: cc.coarse(ctiles[t][c, ys, xs], _yard_floors(tab, nbs)[j]) for j, (t, c, ys, xs) in enumerate(wins)}
        for with_offs in (False, True):
            tag = (geom, fam, marks, k, with_offs)
            dense, o, l, nb, fl = plan.decode_tile_parts(cs, total, tile_offs=d_toffs if with_offs else None, sop=marks, eph=marks, layers=k)
            plan.frame_status()
            ho, hl, hnb, hfl = _host_tables(plan, o, l, nb, fl)
            _invariants(ho, hl, hnb, hfl, dense.numel(), tag)
            _check_tables(tab, dense.cpu().numpy(), ho, hl, hnb, hfl, tag)
            _check_placed(plan, _decode_and_place(plan, dense, o, l, nb, fl), ctiles, wins, coeffs, tag)
            plan.frame_status()
            if L == 1:                                               # the truncated format: the same tables, offsets into the stream
                o, l, nb, fl = plan.decode_tile_parts(cs, total, tile_offs=d_toffs if with_offs else None, sop=marks, eph=marks, floors=True)
                plan.frame_status()
                ho, hl, hnb, hfl = _host_tables(plan, o, l, nb, fl)
                _invariants(ho, hl, hnb, hfl, total, tag)
                _check_tables(tab, np.frombuffer(stream, np.uint8), ho, hl, hnb, hfl, tag)
                _check_placed(plan, _decode_and_place(plan, cs, o, l, nb, fl), ctiles, wins, coeffs, tag)
                plan.frame_status()
        if k not in (1, L):
            continue
        # pixels: the whole frame, and one rectangle at reduce 0 and 1
        floors = _yard_floors(tab, nbs)
        readers = [dict(layers=k)] + ([dict(truncated=True)] if L == 1 else [])
        for r in (0, 1):
            assert r in mc.admissible(W, H, tile, nres)
            exp = rf._expected_pixels(orc, g["case"], True, 0, ctiles, wins, floors, r)
            for kw in readers:
                back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
                plan.decode_frame_pixels(cs, total, back, tile_offs=d_toffs if r else None, sop=marks, eph=marks, reduce=r, **kw)
                plan.frame_status()
                assert np.array_equal(back.cpu().numpy(), exp), (geom, fam, marks, k, r, kw)
                h, w = plan.area_shape(AREAS[geom], r)
                part = torch.full((h, w * bpp), 0x5A, dtype=torch.uint8, device=plan.device)
                plan.decode_frame_pixels(cs, total, part, tile_offs=None if r else d_toffs, sop=marks, eph=marks, reduce=r, area=AREAS[geom], **kw)
                plan.frame_status()
                assert np.array_equal(part.cpu().numpy(), ac.crop(exp, AREAS[geom], r, bpp)), (geom, fam, marks, k, r, kw, "area")


@pytest.mark.parametrize("marks", MARKS, ids=MARK_IDS)
@pytest.mark.parametrize("fam", ["L32-mod5", "L1-random", "L3-free-planes"])
def test_blocks_of_31_planes_through_the_stage_calls(env, fam, marks):
    """geometry b with blocks of 31, 1 and 0 bit planes: writer, both readers, decode_blocks + place_blocks against oracle.t1_decode coarsened"""
    import t2ref
    torch, orc, ctx, get_plan = env
    plan = get_plan("b")
    _, tiles, datas, nbs, Rs, ctiles = sr.tables("b", True)
    assert 31 in nbs
    kept = sr.family(fam, tiles, nbs, Rs)
    L = len(kept)
    want, wtoffs, wloffs = lc.compose(t2ref, tiles, datas, nbs, Rs, kept, marks, marks)
    d_stream, d_offs, d_lens, d_nbs, d_rate = _upload(torch, plan, datas, nbs, Rs)
    cs, toffs, loffs = plan.encode_tile_parts(d_stream, d_offs, d_lens, d_nbs, sop=marks, eph=marks, kept=_dev(torch, plan, kept, np.uint8), rate=d_rate, layers=L)
    plan.frame_status()
    assert toffs.cpu().numpy().tolist() == wtoffs and loffs.cpu().numpy().tolist() == wloffs and bytes(cs.cpu().numpy()[:wtoffs[-1]]) == want
    wins = rf._windows(plan, ctiles, 1)
    buf = _in_buffer(torch, plan, want)
    for k in [k for k in sr.LAYER_COUNTS if k <= L]:
        verdicts = sr.read_tiles(t2ref, want, wtoffs, tiles, k, marks, marks)
        assert sr.frame_ok(verdicts)
        tab = sr.block_tables(want, verdicts)
        assert k < L or any(numbps == 31 for _, _, numbps in tab.values())
        coeffs = _block_coeffs(orc, plan, tab)
        for j, (t, c, ys, xs) in enumerate(wins):                    # (the oracle's decode of the prefix is the coarsened block: the prefix property)
            assert np.array_equal(coeffs[j], cc.coarse(ctiles[t][c, ys, xs], _yard_floors(tab, nbs)[j])), (k, j)
        dense, o, l, nb, fl = plan.decode_tile_parts(buf, len(want), sop=marks, eph=marks, layers=k)
        plan.frame_status()
        ho, hl, hnb, hfl = _host_tables(plan, o, l, nb, fl)
        _invariants(ho, hl, hnb, hfl, dense.numel(), (fam, k))
        _check_tables(tab, dense.cpu().numpy(), ho, hl, hnb, hfl, (fam, k))
        _check_placed(plan, _decode_and_place(plan, dense, o, l, nb, fl), ctiles, wins, coeffs, (fam, k))
        plan.frame_status()
        if L == 1:
            o, l, nb, fl = plan.decode_tile_parts(buf, len(want), sop=marks, eph=marks, floors=True)
            plan.frame_status()
            ho, hl, hnb, hfl = _host_tables(plan, o, l, nb, fl)
            _check_tables(tab, np.frombuffer(want, np.uint8), ho, hl, hnb, hfl, (fam, "floors"))
            _check_placed(plan, _decode_and_place(plan, buf, o, l, nb, fl), ctiles, wins, coeffs, (fam, "floors"))
            plan.frame_status()


# ---- 3. damaged streams -----------------------------------------------------------------------------------------------------------------------------
def _read_guarded(torch, plan, reader_k, layered, cs, n, d_toffs, marks, dense_bytes, passes=False):
    """one stage read with every output inside a guarded tensor -> (status, host tables, the bytes the offsets point into, guards intact); passes:
    the pass reader, its pfloors in the place of the floors"""
    nblk = int(plan.info.blocks)
    wo, o = _guarded(torch, plan, nblk + 1, torch.int64, 0x5A5A5A5A5A5A5A5A)
    wl, l = _guarded(torch, plan, nblk, torch.int32, 0x5A5A5A5A)
    wn, nb = _guarded(torch, plan, nblk, torch.uint8, 0x5A)
    wf, fl = _guarded(torch, plan, nblk, torch.uint8, 0x5A)
    if layered:
        wd, dense = _guarded(torch, plan, dense_bytes, torch.uint8, 0xA5)
        plan.decode_tile_parts(cs, n, tile_offs=d_toffs, sop=marks, eph=marks, layers=reader_k, offs=o, lens=l, numbps=nb, floors=fl, dense=dense)
    elif passes:
        plan.decode_tile_parts(cs, n, tile_offs=d_toffs, sop=marks, eph=marks, offs=o, lens=l, numbps=nb, pfloors=fl)
    else:
        plan.decode_tile_parts(cs, n, tile_offs=d_toffs, sop=marks, eph=marks, offs=o, lens=l, numbps=nb, floors=fl)
    st = _status(plan)
    ok = _guards_intact(wo, nblk + 1, 0x5A5A5A5A5A5A5A5A) and _guards_intact(wl, nblk, 0x5A5A5A5A) and _guards_intact(wn, nblk, 0x5A) and _guards_intact(wf, nblk, 0x5A)
    src = None
    if layered:
        ok = ok and _guards_intact(wd, dense_bytes, 0xA5)
        src = dense.cpu().numpy()
    return st, _host_tables(plan, o, l, nb, fl), src, ok, (o, l, nb, fl, dense if layered else None)


@pytest.mark.parametrize("reader", sorted(sr.READERS))
def test_damaged_streams(env, reader):
    """the status is the yardstick's verdict, the tables of every tile it reads are the yardstick's (beside refused tiles too), the invariants hold
    on everything, nothing is written outside the outputs, and a refused stream leaves the caller's pixels alone.  pfloors: the pass reader; its
    body-damaged codewords go through decode_blocks(pfloors=) -- the PASSCUT decoder and t1_pass_mid on codewords that are no prefix of a known
    block -- and must be pass_stream_cases.decode_passes of the same bytes"""
    from j2kgfx import _lib
    torch, orc, ctx, get_plan = env
    plan = get_plan("a")
    fam, k = sr.READERS[reader]
    layered, passcut = reader not in ("floors", "pfloors"), reader == "pfloors"
    g = sr.GEOMETRIES["a"]
    W, H, Cn, prec, tile, nres = g["case"]
    _, tiles, datas, nbs, Rs, ctiles = sr.tables("a")
    wins = rf._windows(plan, ctiles, Cn)
    seen = {"ok": 0, "refused": 0, "dropped": 0, "mixed": 0, "body": 0, "partial": 0}
    for c in sr.damaged_copies(reader):
        tag = (reader, c["it"], c["kind"])
        marks, n, stream = c["marks"], c["n"], c["stream"]
        cs = _in_buffer(torch, plan, stream)
        d_toffs = _dev(torch, plan, np.asarray(c["offs"], dtype=np.uint64), np.uint64) if c["with_offs"] else None
        st, (ho, hl, hnb, hfl), src, guards, dev = _read_guarded(torch, plan, k, layered, cs, n, d_toffs, marks, len(stream) + 64, passes=passcut)
        verdicts = c["verdicts"]
        good = sr.frame_ok(verdicts)
        assert st == (_lib.OK if good else _lib.ERR_INVALID_ARG), (tag, [v["why"] for v in verdicts])
        assert guards, tag
        (_invariants_pass if passcut else _invariants)(ho, hl, hnb, hfl, len(stream) + 64 if layered else n, tag)
        tab = (sr.block_tables_pass if passcut else sr.block_tables)(stream[:n], verdicts)
        _check_tables(tab, src if layered else np.frombuffer(stream, np.uint8), ho, hl, hnb, hfl, tag)
        some, every = any(v["ok"] for v in verdicts), all(v["ok"] for v in verdicts)
        seen["ok" if good else "refused"] += 1
        seen["mixed"] += int(some and not every)
        seen["dropped"] += int(every and not good)
        if c["kind"] == "body":                                      # the damaged codewords decode as the oracle decodes them
            o, l, nb, fl, dense = dev
            placed = _decode_and_place(plan, dense if layered else cs, o, l, nb, fl, sync=False, passes=passcut)
            assert _status(plan) == _lib.OK, tag
            _check_placed(plan, placed, ctiles, wins, ps.expected_coeffs(ps.pass_tables("a"), tab) if passcut else _block_coeffs(orc, plan, tab), tag)
            seen["body"] += 1
            seen["partial"] += int(passcut and bool(ps.partial_blocks(tab)))
        if not good:                                                 # the frame calls: the same status, with and without area, the pixels untouched
            kw = dict(layers=k) if layered else (dict(pass_cuts=True) if passcut else dict(truncated=True))
            back = torch.full((H, W), 0x5A, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, n, back, tile_offs=d_toffs, sop=marks, eph=marks, **kw)
            assert _status(plan) == st and bool((back == 0x5A).all()), tag
            h, w = plan.area_shape(AREAS["a"], 0)
            part = torch.full((h, w), 0x5A, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, n, part, tile_offs=d_toffs, sop=marks, eph=marks, area=AREAS["a"], **kw)
            assert _status(plan) == st and bool((part == 0x5A).all()), tag
    print("%s: %s" % (reader, seen))
    assert seen["ok"] >= 20 and seen["refused"] >= 20 and seen["dropped"] >= 1 and seen["mixed"] >= 10 and seen["body"] >= 17, seen
    assert seen["partial"] >= 10 or not passcut, seen


# ---- 4. what a frame leaves behind ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reader", ["layers32", "floors", "pfloors"])
def test_stale_state_on_one_plan(env, reader):
    """busy, cut short inside the first tile's first layer, flat, noise, busy again -- on one plan and one layer count, so every frame meets the
    entries the one before left in the plan's packet tables.  pfloors: the pass reader on a stream of random pass cuts, and between two of its
    reads a plane-cut stream through floors=True ("planes"): neither reader may find what the other left"""
    import t2ref
    from j2kgfx import _lib
    torch, orc, ctx, get_plan = env
    plan = get_plan("a")
    layered, passcut = reader == "layers32", reader == "pfloors"
    k = 32 if layered else 1
    L = k
    _, tiles, datas, nbs, Rs, _ = sr.tables("a")
    n = len(nbs)
    busy_kept = sr.family("L32-mod5" if layered else "L1-random", tiles, nbs, Rs)
    if not layered:
        busy_kept = [list(nbs)]
    flat_kept = [[(nbs[j] if (j % 7 == 0 and l >= 3 * int(layered)) else 0) for j in range(n)] for l in range(L)]
    rng = np.random.default_rng(77)
    for marks in MARKS:
        busy, btoffs, bloffs = lc.compose(t2ref, tiles, datas, nbs, Rs, busy_kept, marks, marks)
        flat, ftoffs, floffs = lc.compose(t2ref, tiles, datas, nbs, Rs, flat_kept, marks, marks)
        if passcut:                                                  # the same shapes of frame, cut at coding passes
            busy, btoffs, _ = ps.pass_stream("a", "P-random", marks)
            bloffs = btoffs[1:]
            flat_cuts = dict(qs=[pc.points(nbs[j]) if j % 7 == 0 else 0 for j in range(n)], lengths=[len(datas[j]) if j % 7 == 0 else 0 for j in range(n)], edits={})
            flat = ps.compose_cut(t2ref, ps.pass_tables("a"), flat_cuts, marks, marks)[0]
            planes = sr.base_stream("a", "L1-random", marks)[0]
        cut_n = btoffs[0] + 14 + (bloffs[0] - btoffs[0] - 14) // 2            # inside layer 0 of tile 0
        cut = bytearray(busy)
        cut[6:10] = cut_n.to_bytes(4, "big")                                  # (Psot says so: the chain starts, and runs out of bytes)
        cut = bytes(cut)
        noise = rng.integers(0, 256, len(busy)).astype(np.uint8).tobytes()
        # (name, bytes, the length the reader is told, tile_offs).  "cut": tile-part 0 ends inside its first layer while every byte behind it is
        # still in the buffer -- the segments the busy frame's entries point at lie inside the stream, so an entry that survived would count
        steps = [("busy", busy, len(busy), None), ("cut", cut, len(cut), None), ("flat", flat, len(flat), None), ("busy", busy, len(busy), None),
                 ("cut", cut, len(cut), btoffs), ("busy", busy, len(busy), btoffs), ("cut", cut, cut_n, None), ("noise", noise, len(noise), None),
                 ("busy", busy, len(busy), None)]
        if passcut:
            steps[1:1] = [("planes", planes, len(planes), None), ("busy", busy, len(busy), None)]
        for step, (name, stream, length, offs) in enumerate(steps):
            tag = (reader, marks, step, name)
            intact = name in ("busy", "flat", "planes")
            passes = passcut and name != "planes"
            verdicts = sr.read_tiles(t2ref, stream[:length], offs, tiles, k, marks, marks)
            assert sr.frame_ok(verdicts) == intact, tag
            cs = _in_buffer(torch, plan, stream)
            d_toffs = _dev(torch, plan, offs, np.int64) if offs is not None else None
            st, (ho, hl, hnb, hfl), src, guards, dev = _read_guarded(torch, plan, k, layered, cs, length, d_toffs, marks, len(stream) + 64, passes=passes)
            assert st == (_lib.OK if intact else _lib.ERR_INVALID_ARG) and guards, tag
            (_invariants_pass if passes else _invariants)(ho, hl, hnb, hfl, len(stream) + 64 if layered else length, tag)
            tab = (sr.block_tables_pass if passes else sr.block_tables)(stream[:length], verdicts)
            assert len(tab) == (n if intact else (n - sum(len(pk) for pk in tiles[0]) if offs is not None else 0)), tag
            _check_tables(tab, src if layered else np.frombuffer(stream, np.uint8), ho, hl, hnb, hfl, tag)
            if name == "cut":                                        # no block the chains did not reach carries the busy frame's entry
                assert not verdicts[0]["ok"] and 0 < verdicts[0]["done"] < len(tiles[0]) and "run out" in verdicts[0]["why"]
                reached = {j for pk in tiles[0][:verdicts[0]["done"]] for j in pk}
                unreached = [j for j in range(n) if j not in reached and j not in tab]
                assert len(unreached) >= 3 and any(busy_tab[j][0] for j in unreached), tag
                for j in unreached:
                    assert (int(hl[j]), int(hnb[j]), int(hfl[j])) == (0, 0, 0), (tag, j)
            elif name == "busy":
                busy_tab = tab


# ---- 5. a dense buffer that is too small ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("marks", MARKS, ids=MARK_IDS)
def test_dense_capacity(env, marks):
    import t2ref
    from j2kgfx import _lib
    torch, orc, ctx, get_plan = env
    plan = get_plan("a")
    _, tiles, datas, nbs, Rs, _ = sr.tables("a")
    stream, toffs, loffs, kept = sr.base_stream("a", "L32-mod5", marks)
    k, n = 32, len(nbs)
    tab = sr.block_tables(stream, sr.read_tiles(t2ref, stream, toffs, tiles, k, marks, marks))
    lens = [len(tab[j][0]) for j in range(n)]
    need = sum(lens)
    starts = np.concatenate([[0], np.cumsum(lens)])
    cs = _in_buffer(torch, plan, stream)
    for cap in (need, need - 1, need // 2, 0):
        whole = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=plan.device)
        dense, o, l, nb, fl = plan.decode_tile_parts(cs, len(stream), sop=marks, eph=marks, layers=k, dense=whole[GUARD:], dense_cap=cap)
        assert _status(plan) == (_lib.OK if cap == need else _lib.ERR_CAPACITY), cap
        ho, hl, hnb, hfl = _host_tables(plan, o, l, nb, fl)
        _invariants(ho, hl, hnb, hfl, cap, cap)
        kept_blocks = {j for j in range(n) if int(starts[j]) + lens[j] <= cap}          # the running sum in block order stays within the capacity
        assert cap == need or any(lens[j] for j in range(n) if j not in kept_blocks)
        hw = whole.cpu().numpy()
        assert (hw[:GUARD] == 0xA5).all() and (hw[GUARD + cap:] == 0xA5).all(), cap      # nothing before the buffer, nothing at or past cap
        for j in range(n):
            if j in kept_blocks:
                assert (int(hl[j]), int(hfl[j]), int(hnb[j])) == (lens[j], tab[j][1], tab[j][2]), (cap, j)
                assert bytes(hw[GUARD + int(ho[j]):GUARD + int(ho[j]) + lens[j]]) == tab[j][0], (cap, j)
            else:
                assert (int(hl[j]), int(hfl[j]), int(hnb[j]), int(ho[j])) == (0, 0, 0, 0), (cap, j)
    with pytest.raises(_lib.J2KError):
        plan.decode_tile_parts(cs, len(stream), layers=k, dense=whole[GUARD:], dense_cap=int(whole.numel()))
