"""GPU: rate control on batch plans (FramePlan(frame_rows=..., rate_per_frame=True)) against tests/frame_rate_cases.py -- the existing definitions
applied to every frame's job range -- and the oracle; the "as alone" identity with single-frame plans comes on top.

Plans: Mallat MQ, closed loop, 5-3 unless said otherwise.  Geometries (frame_rate_cases.GEOMETRIES): "thin" 3 frames of 130 x 70 RGB8, 4
resolutions, 64 x 64 blocks, untiled; "tiled" 2 frames of 260 x 44, tiles 128 x 32 (a partial last tile row in every frame); "strided" 2 frames of
200 x 150 x 3, 3 resolutions, 8 x 8 blocks: more than 1024 blocks per frame and a count that is no multiple of 64, so a thread owns several blocks
and frame 1 starts inside a wavefront's worth of indices -- allocation only, on quality_cases.random_tables (the allocation takes any tables).

Frames (closed_loop_ref.pixel_frame; they differ so that the frames' lambdas differ): 0 noise at 1/16 of the range, 1 flat -- ONE colour, so its few
bytes fit every budget that cuts its neighbours --, 2 noise at 1/2 of the range.

Budgets.  The flat frame is the smallest, so "50 % / 10 % of the smallest frame's body bytes" are next to nothing for the noisy frames; the same
fractions of the smallest NOISY frame are tested beside them: those cut the noisy frames in the middle of their tables while frame 1 stays whole.
The rate tables of the coded frames come from encode_blocks(planes=True / pass_cuts=True) on the batch plan (block coding and distortion run one
job per block and are held to the oracle in tests/test_gpu_rate_encode.py and tests/test_gpu_pass_cuts.py; the SigProp masks of the pass model
are the device's too).  Every comparison is bit for bit."""
import functools

import numpy as np
import pytest

import closed_loop_ref as ref
import coarse_cases as cc
import frame_rate_cases as fr
import layer_cases as lc
import mallat_cases as mc
import pass_cases as pc
import quality_cases as qc
import rate_cases as rc

pytestmark = pytest.mark.gpu
INF = fr.INF
PREC = 8


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    from j2kgfx import Context
    ctx = Context(0)
    yield torch, orc, ctx
    ctx.close()


def _u(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}.get(a.dtype, a.dtype))


def _plan(ctx, name, batch=True, lossless=True, quality=0, **kw):
    from j2kgfx.codec import FramePlan
    W, rows, F, Cn, nres, cb, tile = fr.GEOMETRIES[name]
    kw.setdefault("rate_per_frame", batch)
    return FramePlan(W, rows * F if batch else rows, Cn, precision=PREC, lossless=lossless, quality=quality, num_resolutions=nres, cb=(cb, cb), tile=tile, coder=0, ctx=ctx,
                     mallat=True, frame_rows=rows if batch else 0, dequantize=not lossless, **kw)


def _one_colour(orc, fmt, W, H, Cn):
    vals = np.stack([np.full((H, W), v, np.int32) for v in (200, 50, 10, 90)[:Cn]])
    pix = orc.create_image([vals[c] for c in range(Cn)], PREC)
    planes = np.stack(orc.extract_image_data(pix, fmt, W, H))
    assert np.array_equal(planes, vals)
    return pix, planes


@functools.lru_cache(None)
def _frames(name, lossless=True, quality=0):
    """(fmt, [pix of every frame], batch pix [F * rows, stride], the oracle's forward coefficient tiles of the batch) -- once, shared, never written"""
    import oracle as orc
    W, rows, F, Cn, nres, cb, tile = fr.GEOMETRIES[name]
    fmt = mc.PIX_FORMAT[(Cn, PREC)]
    pixs, planes = [], []
    for f in range(F):
        seed, noise = fr.FRAME_NOISE[f]
        if noise == 0.0:
            p, pl = _one_colour(orc, fmt, W, rows, Cn)
        else:
            p, _, _, pl = ref.pixel_frame(fmt, W, rows, 300 + seed, orc, noise=int(((1 << PREC) - 1) * noise))
        pixs.append(p); planes.append(pl)
    batch = np.ascontiguousarray(np.concatenate(pixs, axis=0))
    tiles = mc.forward_frame(orc, np.concatenate(planes, axis=1), tile, PREC, nres, lossless, quality, frame_rows=rows)
    return fmt, pixs, batch, tiles


def _block_res(plan):
    out, r, last = [], 0, None
    for b in plan.blocks():
        key = (int(b["plane"]), int(b["band"]))
        if last is not None and key != last:
            if key[0] != last[0]:
                r = 0
            elif key[1] < last[1] or last[1] == 0:
                r += 1
        out.append(r)
        last = key
    return out


def _packets(plan):
    bl, res, Cn = plan.blocks(), _block_res(plan), plan.ncomp
    tiles = [[] for _ in range(int(plan.info.tiles))]
    j = 0
    while j < len(bl):
        k = j
        while k < len(bl) and int(bl[k]["plane"]) == int(bl[j]["plane"]) and res[k] == res[j]:
            k += 1
        tiles[int(bl[j]["plane"]) // Cn].append(list(range(j, k)))
        j = k
    return tiles


def _weights(plan):
    w, res, Cn = plan.rate_weights(), _block_res(plan), plan.ncomp
    return [float(w[int(b["plane"]) % Cn, res[j], int(b["band"])]) for j, b in enumerate(plan.blocks())]


def _ranges(plan, F):
    Cn = plan.ncomp
    return fr.frame_ranges([int(b["plane"]) // Cn for b in plan.blocks()], int(plan.info.tiles) // F, F)


_TABLES = {}


def _tables(torch, ctx, name):
    """the batch's tables from the stage calls, fetched ONCE per geometry; everything the tests expect is the Python definition run on them"""
    if name in _TABLES:
        return _TABLES[name]
    from j2kgfx import entropy
    W, rows, F, Cn, nres, cb, tile = fr.GEOMETRIES[name]
    fmt, pixs, batch, tiles = _frames(name)
    plan = _plan(ctx, name)
    try:
        assert plan.rate_frames == F
        coeff = plan.forward_pixels(fmt, torch.from_numpy(batch).to(plan.device))
        slots, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True)
        _, lens2, nbs2, prate, pdist, spm = plan.encode_blocks(coeff, pass_cuts=True)
        ctx.sync()
        n = int(plan.info.blocks)
        bl = plan.blocks()
        nb = nbs.cpu().numpy()[:n].astype(np.int64)
        ln = _u(lens)[:n].astype(np.int64)
        assert np.array_equal(nb, nbs2.cpu().numpy()[:n]) and np.array_equal(ln, _u(lens2)[:n])
        hs, pos, datas, wins, vs, sps = slots.cpu().numpy(), 0, [], [], [], []
        spw = _u(spm)[:n]
        for j, b in enumerate(bl):
            datas.append(hs[pos:pos + int(ln[j])].copy())
            pos += (entropy.block_bound(0, int(b["w"]), int(b["h"])) + 15) & ~15
            t, c = int(b["plane"]) // Cn, int(b["plane"]) % Cn
            ys, xs = slice(int(b["y0"]), int(b["y0"]) + int(b["h"])), slice(int(b["x0"]), int(b["x0"]) + int(b["w"]))
            wins.append((t, c, ys, xs))
            v = tiles[t][c, ys, xs]
            assert pc.numbps_of(v) == int(nb[j]), j                      # the batch's blocks are the oracle's coefficients
            vs.append(v)
            sps.append(((spw[j][:v.shape[0], None] >> np.arange(v.shape[1], dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool))     # (the device's SigProp masks)
        out = dict(R=_u(rate)[:n].astype(np.int64), D=_u(dist)[:n], PR=_u(prate)[:n].astype(np.int64), PD=_u(pdist)[:n], nb=nb, lens=ln, ws=_weights(plan), datas=datas,
                   wins=wins, vs=vs, sps=sps, packets=_packets(plan), ranges=_ranges(plan, F), n=n, rate=rate, dist=dist, prate=prate, pdist=pdist, nbs=nbs,
                   pts=[pc.points(x) for x in nb])
        out["body"] = [int(ln[a:a + c].sum()) for a, c in out["ranges"]]
        _TABLES[name] = out
        return out
    finally:
        plan.close()


def _budgets(body):
    """scalars: infinity, 50 %, 10 %, 0 of the smallest frame; 50 % and 10 % of the smallest noisy frame.  The vector [0, infinity, 50 % of the last
    frame]; two frames: [50 % of frame 0, infinity] -- frame 1 returns early while its neighbour searches"""
    small, noisy = min(body), min(b for f, b in enumerate(body) if fr.FRAME_NOISE[f][1] > 0)
    scalars = [INF, small // 2, small // 10, 0, noisy // 2, noisy // 10]
    vector = [0, INF, body[2] // 2] if len(body) == 3 else [body[0] // 2, INF]
    return scalars, vector


def _bits(x):
    return [qc.float_bits(v) for v in np.asarray(x, dtype=np.float64).reshape(-1)]


# ---- 1. allocation against the definition -------------------------------------------------------------------------------------------------------
def _check_allocation(torch, plan, F, n, ranges, tabs, dev, body, passes):
    """tabs = (Rs, Ds, point counts, ws) on the host, dev = (rate, dist, numbps) on the device"""
    Rs, Ds, pts, ws = tabs
    rate, dist, nbs = dev
    scalars, vector = _budgets(body)
    for b in scalars + [vector]:
        per = isinstance(b, list)
        kept, chosen = plan.rate_allocate(rate, dist, nbs, **(dict(frame_bytes=b) if per else dict(max_body_bytes=b)), pass_cuts=passes)
        plan.ctx.sync()
        wk, wc = fr.allocate_frames(Rs, Ds, pts, ws, ranges, b)
        assert tuple(chosen.shape) == (F,) and chosen.cpu().numpy().tolist() == wc, b
        assert kept.cpu().numpy()[:n].tolist() == wk, b
        assert all(c <= (b[f] if per else b) for f, c in enumerate(wc))
    noisy = min(x for f, x in enumerate(body) if fr.FRAME_NOISE[f][1] > 0)
    wk, _ = fr.allocate_frames(Rs, Ds, pts, ws, ranges, noisy // 2)
    cut = [any(0 < wk[j] < pts[j] for j in range(a, a + c)) for a, c in ranges]
    assert cut[0] and cut[-1], "vacuous: a noisy frame is not cut inside its tables"
    if not passes:
        ladder = [noisy // 10, noisy // 2, INF]
        kept, chosen = plan.rate_allocate_layers(rate, dist, nbs, ladder)
        plan.ctx.sync()
        wk, wc = fr.allocate_layers_frames(Rs, Ds, pts, ws, ranges, ladder)
        assert tuple(chosen.shape) == (3, F) and chosen.cpu().numpy().tolist() == wc and kept.cpu().numpy().tolist() == wk
    start = [qc.wg_sum_f64([qc.term(ws[j], Ds[j][0]) for j in range(a, a + c)]) for a, c in ranges]
    top = max(start)
    one, falling, tvec = top / 50.0, [top / 8.0, top / 200.0, 0.0], [s / (3.0 + 5 * f) for f, s in enumerate(start)]
    for T in ([one], falling, tvec):
        per = T is tvec
        if passes and len(T) > 1 and not per:
            continue                                                     # (pass cuts take one target)
        kept, chosen, achieved = plan.rate_allocate_quality(rate, dist, nbs, **(dict(frame_targets=T) if per else dict(targets=T)), pass_cuts=passes)
        plan.ctx.sync()
        wk, wc, wa = fr.allocate_quality_layers_frames(Rs, Ds, pts, ws, ranges, T, per_frame=per, passes=passes)
        L = 1 if per else len(T)
        assert tuple(chosen.shape) == (L, F) == tuple(achieved.shape)
        assert kept.cpu().numpy().tolist() == wk and chosen.cpu().numpy().tolist() == wc, T
        assert _bits(achieved.cpu().numpy()) == _bits(wa), T
        assert all(wa[l][f] <= (T[f] if per else T[l]) for l in range(L) for f in range(F))
    assert len({tuple(wk[0][a:a + min(c, 40)]) for a, c in ranges}) > 1


@pytest.mark.parametrize("passes", [False, True], ids=["planes", "passes"])
def test_allocation_of_coded_frames(env, passes):
    torch, orc, ctx = env
    T = _tables(torch, ctx, "thin")
    F = 3
    plan = _plan(ctx, "thin")
    try:
        tabs = (T["PR"], T["PD"], T["pts"], T["ws"]) if passes else (T["R"], T["D"], [int(x) for x in T["nb"]], T["ws"])
        dev = (T["prate"], T["pdist"], T["nbs"]) if passes else (T["rate"], T["dist"], T["nbs"])
        _check_allocation(torch, plan, F, T["n"], T["ranges"], tabs, dev, T["body"], passes)
    finally:
        plan.close()


@pytest.mark.parametrize("passes", [False, True], ids=["planes", "passes"])
def test_allocation_many_blocks_per_thread(env, passes):
    """ "strided": random tables on a plan of more than 1024 blocks per frame"""
    torch, orc, ctx = env
    F = 2
    plan = _plan(ctx, "strided")
    try:
        n = int(plan.info.blocks)
        ranges = _ranges(plan, F)
        assert all(c > 1024 and c % 64 for _, c in ranges) and ranges[1][0] % 64, ranges
        _, _, nbs, _ = qc.random_tables(11, n)
        ws = _weights(plan)
        rng = np.random.default_rng(12)
        st = 96 if passes else 32
        R, D = np.zeros((n, st), np.uint32), np.zeros((n, st), np.uint64)
        pts = [pc.points(nb) if passes else int(nb) for nb in nbs]
        for j, q in enumerate(pts):                                      # rising R, falling D, D = 0 at the last point
            if q:
                # frame 1 costs about three times frame 0 per block, so one lambda does not serve both
                R[j, 1:q + 1] = np.cumsum(rng.integers(0, 40 if j < ranges[1][0] else 120, q))
                R[j, q:] = R[j, q]
                D[j, :q] = np.sort(rng.integers(1, 1 << 24, q).astype(np.uint64))[::-1]
        body = [int(sum(int(R[j, pts[j]]) for j in range(a, a + c))) for a, c in ranges]
        dev = (torch.from_numpy(R.view(np.int32)).to(plan.device), torch.from_numpy(D.view(np.int64)).to(plan.device),
               torch.from_numpy(np.asarray(nbs, np.uint8)).to(plan.device))
        _check_allocation(torch, plan, F, n, ranges, (R.astype(np.int64), D, pts, ws), dev, body, passes)
    finally:
        plan.close()


# ---- 2. streams ---------------------------------------------------------------------------------------------------------------------------------
def _single_streams(torch, ctx, name, calls):
    """frame f alone on a single-frame plan: calls[key] = keyword arguments per frame -> {key: [(bytes, tile_offs) per frame]} (sop / eph inside)"""
    W, rows, F, Cn, nres, cb, tile = fr.GEOMETRIES[name]
    fmt, pixs, _, _ = _frames(name)
    plan = _plan(ctx, name, batch=False)
    out = {k: [] for k in calls}
    try:
        for f in range(F):
            d = torch.from_numpy(pixs[f]).to(plan.device)
            for k, kws in calls.items():
                res = plan.encode_frame_pixels(fmt, d, **kws[f])
                plan.frame_status()
                out[k].append((res[0].cpu().numpy()[:int(res[1][-1].item())].copy(), res[1].cpu().numpy().copy()))
    finally:
        plan.close()
    return out


def _as_alone(h_cs, h_toffs, singles, tpf):
    """every frame's tile-parts, from byte 14 on (the SOT holds the tile's number in the batch), equal the single-frame plan's"""
    for f, (scs, stoffs) in enumerate(singles):
        for t in range(tpf):
            a, b = int(h_toffs[f * tpf + t]), int(h_toffs[f * tpf + t + 1])
            sa, sb = int(stoffs[t]), int(stoffs[t + 1])
            assert bytes(h_cs[a + 14:b]) == bytes(scs[sa + 14:sb]), (f, t)
            assert bytes(h_cs[a + 6:a + 10]) == bytes(scs[sa + 6:sa + 10]), (f, t)       # Psot


@pytest.mark.parametrize("marks", [False, True], ids=["bare", "sop_eph"])
@pytest.mark.parametrize("name", ["thin", "tiled"])
def test_streams(env, name, marks):
    import t2ref
    torch, orc, ctx = env
    W, rows, F, Cn, nres, cb, tile = fr.GEOMETRIES[name]
    fmt, pixs, batch, _ = _frames(name)
    T = _tables(torch, ctx, name)
    ranges, n, body = T["ranges"], T["n"], T["body"]
    nbl = [int(x) for x in T["nb"]]
    scalars, vector = _budgets(body)
    noisy = scalars[4] * 2
    budget, ladder, db = scalars[4], [noisy // 10, noisy // 2, INF], 30.0
    mk = dict(sop=marks, eph=marks)
    plan = _plan(ctx, name)
    tpf = int(plan.info.tiles) // F
    try:
        d_pix = torch.from_numpy(batch).to(plan.device)
        Tq = plan.psnr_distortion(db)
        assert Tq == fr.psnr_distortion(W, rows, Cn, PREC, True, 0, db)
        got = {}
        for key, kw in (("scalar", dict(max_body_bytes=budget)), ("vector", dict(frame_bytes=vector)), ("psnr", dict(min_psnr=db)), ("layers", dict(layer_bytes=ladder)),
                        ("pass", dict(max_body_bytes=budget, pass_cuts=True)), ("pass_vector", dict(frame_bytes=vector, pass_cuts=True))):
            res = plan.encode_frame_pixels(fmt, d_pix, **mk, **kw)
            plan.frame_status()
            length = int(res[1][-1].item())
            got[key] = (res[0].cpu().numpy()[:length].copy(), res[1].cpu().numpy().copy()) + tuple(x.cpu().numpy().copy() for x in res[2:])
        planes_tabs = (T["R"], T["D"], nbl, T["ws"])
        # the kept-prefix streams of the plane cuts
        for key, b in (("scalar", budget), ("vector", vector)):
            ps, _ = fr.allocate_frames(*planes_tabs, ranges, b)
            want = lc.compose_kept(t2ref, T["packets"], T["datas"], nbl, T["R"], ps, marks, marks)
            assert bytes(got[key][0]) == want and int(got[key][1][-1]) == len(want), key
        ps, _, ach = fr.allocate_quality_frames(*planes_tabs, ranges, Tq)
        assert bytes(got["psnr"][0]) == lc.compose_kept(t2ref, T["packets"], T["datas"], nbl, T["R"], ps, marks, marks)
        assert got["psnr"][2].shape == (F,) and _bits(got["psnr"][2]) == _bits(ach)
        kept, _ = fr.allocate_layers_frames(*planes_tabs, ranges, ladder)
        want, wto, wlo = lc.compose(t2ref, T["packets"], T["datas"], nbl, T["R"], kept, marks, marks)
        assert bytes(got["layers"][0]) == want and got["layers"][1].tolist() == wto and got["layers"][2].tolist() == wlo
        for key, b in (("pass", budget), ("pass_vector", vector)):
            qs, _ = fr.allocate_frames(T["PR"], T["PD"], T["pts"], T["ws"], ranges, b)
            assert bytes(got[key][0]) == pc.compose_kept_passes(t2ref, T["packets"], T["datas"], nbl, T["PR"], qs, marks, marks), key
        # every frame as it would be alone under its own budget
        calls = dict(scalar=[dict(max_body_bytes=budget, **mk)] * F, vector=[dict(max_body_bytes=vector[f], **mk) for f in range(F)],
                     psnr=[dict(min_psnr=db, **mk)] * F, layers=[dict(layer_bytes=ladder, **mk)] * F,
                     **{"pass": [dict(max_body_bytes=budget, pass_cuts=True, **mk)] * F})
        for key, singles in _single_streams(torch, ctx, name, calls).items():
            _as_alone(got[key][0], got[key][1], singles, tpf)
    finally:
        plan.close()


# ---- 3. pixels ----------------------------------------------------------------------------------------------------------------------------------
def _expected(orc, name, T, qs, reduce, skip, lossless=True, quality=0, tiles=None):
    """the oracle's inverse of the coefficients every block's pass cut qs[j] (and the uniform floor) leaves"""
    W, rows, F, Cn, nres, cb, tile = fr.GEOMETRIES[name]
    tiles = tiles if tiles is not None else _frames(name)[3]
    cut = [t.copy() for t in tiles]
    for j, (t, c, ys, xs) in enumerate(T["wins"]):
        nb = int(T["nb"][j])
        q = pc.q_of(nb, max(3 * skip, pc.pfloor_of(nb, int(qs[j]))))
        cut[t][c, ys, xs] = pc.coarse_pass(T["vs"][j], nb, q, T["sps"][j])
    kw = {} if lossless else dict(lossless=False, quality=quality, dequantize=True)
    return mc.pixels(orc, mc.inverse_frame(orc, cut, W, rows * F, tile, PREC, nres, reduce=reduce, frame_rows=rows, **kw), PREC)


@pytest.mark.parametrize("name", ["thin", "tiled"])
def test_pixels(env, name):
    from j2kgfx import codestream
    torch, orc, ctx = env
    W, rows, F, Cn, nres, cb, tile = fr.GEOMETRIES[name]
    fmt, pixs, batch, _ = _frames(name)
    T = _tables(torch, ctx, name)
    ranges, body = T["ranges"], T["body"]
    nbl = [int(x) for x in T["nb"]]
    scalars, vector = _budgets(body)
    noisy = scalars[4] * 2
    ladder = [noisy // 10, noisy // 2, INF]
    planes_tabs = (T["R"], T["D"], nbl, T["ws"])
    plan = _plan(ctx, name)
    try:
        d_pix = torch.from_numpy(batch).to(plan.device)
        assert 1 in mc.admissible(W, rows * F, tile, nres, rows)

        def check(cs, length, toffs, qs, what, **kw):
            for r in (0, 1):
                for k in (0, 3):
                    exp = _expected(orc, name, T, qs, r, k)
                    back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
                    plan.decode_frame_pixels(cs, length, back, tile_offs=toffs if k else None, reduce=r, skip_planes=k, **kw)
                    plan.frame_status()
                    assert np.array_equal(back.cpu().numpy(), exp), (what, r, k)

        cs, toffs = plan.encode_frame_pixels(fmt, d_pix, frame_bytes=vector)
        plan.frame_status()
        ps, _ = fr.allocate_frames(*planes_tabs, ranges, vector)
        check(cs, int(toffs[-1].item()), toffs, [rc.passes_of(p) for p in ps], "truncated", truncated=True)
        a, c = ranges[1]
        assert ps[a:a + c] == nbl[a:a + c] and np.array_equal(_expected(orc, name, T, [rc.passes_of(p) for p in ps], 0, 0)[rows:2 * rows], pixs[1])   # the flat frame: whole
        cs, toffs = plan.encode_frame_pixels(fmt, d_pix, max_body_bytes=scalars[4], pass_cuts=True)
        plan.frame_status()
        qs, _ = fr.allocate_frames(T["PR"], T["PD"], T["pts"], T["ws"], ranges, scalars[4])
        assert any(pc.split(q)[1] for q in qs if q), "vacuous: no block cut inside a plane"
        check(cs, int(toffs[-1].item()), toffs, qs, "pass_cuts", pass_cuts=True)
        cs, toffs, loffs = plan.encode_frame_pixels(fmt, d_pix, layer_bytes=ladder)
        plan.frame_status()
        length = int(toffs[-1].item())
        kept, _ = fr.allocate_layers_frames(*planes_tabs, ranges, ladder)
        h_cs, h_toffs, h_loffs = cs.cpu().numpy()[:length], toffs.cpu().numpy(), loffs.cpu().numpy()
        for k in (1, 2, 3):
            Q = [lc.normalise(T["R"][j], [kept[l][j] for l in range(k)])[-1] for j in range(T["n"])]
            qk = [rc.passes_of(p) for p in Q]
            check(cs, length, toffs, qk, "layers %d" % k, layers=k)
            cut, ctoffs = codestream.keep_layers(h_cs, h_toffs, h_loffs, k)
            d_cut = torch.from_numpy(np.frombuffer(cut, np.uint8).copy()).to(plan.device)
            exp = _expected(orc, name, T, qk, 0, 0)
            back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(d_cut, len(cut), back, layers=k)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), ("keep_layers", k)
        assert np.array_equal(_expected(orc, name, T, [rc.passes_of(p) for p in nbl], 0, 0), batch)      # every layer: the input exactly
    finally:
        plan.close()


def test_pixels_lossy_batch_of_two(env):
    """mallat_cases.LOSSY[0] as a batch of 2 (9-7, the dequantiser on): one budget per frame, the truncated decode against the oracle"""
    from j2kgfx import entropy
    from j2kgfx.codec import FramePlan
    torch, orc, ctx = env
    W, H, Cn, prec, tile, nres, q = mc.LOSSY[0][:7]
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    pixs, planes = [], []
    for f, noise in enumerate((15, 100)):
        p, _, _, pl = ref.pixel_frame(fmt, W, H, 500 + f, orc, noise=noise)
        pixs.append(p); planes.append(pl)
    batch = np.ascontiguousarray(np.concatenate(pixs, axis=0))
    tiles = mc.forward_frame(orc, np.concatenate(planes, axis=1), tile, prec, nres, False, q, frame_rows=H)
    plan = FramePlan(W, 2 * H, Cn, precision=prec, lossless=False, quality=q, num_resolutions=nres, cb=(64, 64), tile=tile, ctx=ctx, mallat=True, frame_rows=H,
                     dequantize=True, rate_per_frame=True)
    try:
        d_pix = torch.from_numpy(batch).to(plan.device)
        coeff = plan.forward_pixels(fmt, d_pix)
        _, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True)
        ctx.sync()
        n = int(plan.info.blocks)
        R, D, nb, ln = _u(rate)[:n].astype(np.int64), _u(dist)[:n], [int(x) for x in nbs.cpu().numpy()[:n]], _u(lens)[:n].astype(np.int64)
        ranges = _ranges(plan, 2)
        body = [int(ln[a:a + c].sum()) for a, c in ranges]
        vec = [body[0] // 3, body[1] // 5]
        ps, chosen = fr.allocate_frames(R, D, nb, _weights(plan), ranges, vec)
        cs, toffs = plan.encode_frame_pixels(fmt, d_pix, frame_bytes=vec)
        plan.frame_status()
        cut = [t.copy() for t in tiles]
        for j, b in enumerate(plan.blocks()):
            t, c = int(b["plane"]) // Cn, int(b["plane"]) % Cn
            ys, xs = slice(int(b["y0"]), int(b["y0"]) + int(b["h"])), slice(int(b["x0"]), int(b["x0"]) + int(b["w"]))
            cut[t][c, ys, xs] = cc.coarse(tiles[t][c, ys, xs], nb[j] - ps[j])
        exp = mc.pixels(orc, mc.inverse_frame(orc, cut, W, 2 * H, tile, prec, nres, lossless=False, quality=q, dequantize=True, frame_rows=H), prec)
        back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, int(toffs[-1].item()), back, truncated=True)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp)
        assert any(0 < ps[j] < nb[j] for j in range(n))
    finally:
        plan.close()


# ---- 4. host forms ------------------------------------------------------------------------------------------------------------------------------
def test_host_forms(env):
    torch, orc, ctx = env
    name = "tiled"
    W, rows, F, Cn, nres, cb, tile = fr.GEOMETRIES[name]
    fmt, pixs, batch, _ = _frames(name)
    T = _tables(torch, ctx, name)
    scalars, vector = _budgets(T["body"])
    tv = [1.0e5, 3.0e6]
    plan = _plan(ctx, name)
    try:
        d_pix = torch.from_numpy(batch).to(plan.device)
        for kw, dec in ((dict(max_body_bytes=scalars[4]), dict(truncated=True)), (dict(frame_bytes=vector), dict(truncated=True)),
                        (dict(frame_distortion=tv), dict(truncated=True)), (dict(frame_distortion=tv, pass_cuts=True), dict(pass_cuts=True)),
                        (dict(min_psnr=32.0), dict(truncated=True)), (dict(layer_distortion=[5.0e6, 2.0e5]), dict(layers=2))):
            dev = plan.encode_frame_pixels(fmt, d_pix, sop=True, **kw)
            plan.frame_status()
            length = int(dev[1][-1].item())
            host = plan.encode_pixels_host(fmt, batch, sop=True, **kw)
            assert bytes(host["bytes"]) == bytes(dev[0].cpu().numpy()[:length]), kw
            assert host["tile_offs"].tolist() == dev[1].cpu().numpy().tolist()
            assert host["lens"].astype(np.int64).tolist() == T["lens"].tolist() and host["numbps"].tolist() == T["nb"].tolist()      # the UNCUT tables
            if "achieved" in host:
                want = (2, F) if "layer_distortion" in kw else (F,)
                assert host["achieved"].shape == want == tuple(dev[-1].shape), kw
                assert _bits(host["achieved"]) == _bits(dev[-1].cpu().numpy())
            if "layer_distortion" in kw:
                assert host["layer_offs"].tolist() == dev[2].cpu().numpy().tolist()
            back = torch.full(batch.shape, 0x5A, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(dev[0], length, back, sop=True, **dec)
            plan.frame_status()
            hb = plan.decode_pixels_host(host["bytes"], batch.shape, sop=True, **dec)
            assert np.array_equal(hb, back.cpu().numpy()), kw
    finally:
        plan.close()


# ---- 5. the switch ------------------------------------------------------------------------------------------------------------------------------
def test_the_switch(env):
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    torch, orc, ctx = env
    name = "thin"
    W, rows, F, Cn, nres, cb, tile = fr.GEOMETRIES[name]
    fmt, pixs, batch, _ = _frames(name)
    plan = _plan(ctx, name, rate_per_frame=False)
    try:
        d_pix = torch.from_numpy(batch).to(plan.device)
        assert plan.rate_frames == 1

        def refused():
            with pytest.raises(J2KError) as e:
                plan.encode_frame_pixels(fmt, d_pix, max_body_bytes=1000)
            assert e.value.status == _lib.ERR_UNSUPPORTED and "a batch plan (frame_rows): not built" in str(e.value)
            with pytest.raises(J2KError) as e:
                plan.encode_frame_pixels(fmt, d_pix, frame_bytes=[1000])
            assert e.value.status == _lib.ERR_UNSUPPORTED
        refused()
        plan.set_rate_per_frame(True)
        assert plan.rate_frames == F
        cs, toffs = plan.encode_frame_pixels(fmt, d_pix, max_body_bytes=1000)
        plan.frame_status()
        plan.set_rate_per_frame(False)
        assert plan.rate_frames == 1
        refused()
        for bad in (2, -1):
            with pytest.raises(J2KError) as e:
                plan.set_rate_per_frame(bad)
            assert e.value.status == _lib.ERR_INVALID_ARG
    finally:
        plan.close()
    # one frame: the setting changes no byte and no table, chosen keeps its shape
    a, b = _plan(ctx, name, batch=False, rate_per_frame=False), _plan(ctx, name, batch=False, rate_per_frame=True)
    try:
        assert a.rate_frames == b.rate_frames == 1
        outs = []
        for p in (a, b):
            d = torch.from_numpy(pixs[0]).to(p.device)
            coeff = p.forward_pixels(fmt, d)
            _, lens, nbs, rate, dist = p.encode_blocks(coeff, planes=True)
            p.ctx.sync()
            total = int(_u(lens)[:int(p.info.blocks)].astype(np.int64).sum())
            k1, c1 = p.rate_allocate(rate, dist, nbs, total // 3)
            k2, c2 = p.rate_allocate(rate, dist, nbs, frame_bytes=[total // 3])
            k3, c3 = p.rate_allocate_layers(rate, dist, nbs, [total // 10, total // 3])
            k4, c4, a4 = p.rate_allocate_quality(rate, dist, nbs, [1.0e6, 1.0e4])
            p.ctx.sync()
            assert tuple(c1.shape) == (1,) == tuple(c2.shape) and tuple(c3.shape) == (2,) == tuple(c4.shape) == tuple(a4.shape)
            assert k1.cpu().numpy().tolist() == k2.cpu().numpy().tolist() and c1.item() == c2.item()
            row = [k1.cpu().numpy().tolist(), c1.item(), k3.cpu().numpy().tolist(), c3.cpu().numpy().tolist(), k4.cpu().numpy().tolist(), c4.cpu().numpy().tolist(), _bits(a4.cpu().numpy())]
            for kw in (dict(max_body_bytes=total // 3), dict(frame_bytes=[total // 3]), dict(min_psnr=33.0), dict(frame_psnr=[33.0]), dict(layer_bytes=[total // 10, total // 3]),
                       dict(max_body_bytes=total // 3, pass_cuts=True), dict(frame_bytes=[total // 3], pass_cuts=True)):
                res = p.encode_frame_pixels(fmt, d, **kw)
                p.frame_status()
                row.append(bytes(res[0].cpu().numpy()[:int(res[1][-1].item())]))
            assert row[7] == row[8] and row[9] == row[10] and row[12] == row[13]      # frame_bytes=[N] is max_body_bytes=N, byte for byte
            outs.append(row)
        assert outs[0] == outs[1]
    finally:
        a.close(); b.close()


# ---- 6. refusals: before any launch ---------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    from j2kgfx.codec import FramePlan
    torch, orc, ctx = env
    name = "thin"
    W, rows, F, Cn, nres, cb, tile = fr.GEOMETRIES[name]
    fmt, pixs, batch, _ = _frames(name)
    T = _tables(torch, ctx, name)
    plan = _plan(ctx, name)
    try:
        d_pix = torch.from_numpy(batch).to(plan.device)
        good, gto = plan.encode_frame_pixels(fmt, d_pix, max_body_bytes=T["body"][0] // 2)
        plan.frame_status()
        glen = int(gto[-1].item())
        out = torch.full((plan.frame_bound(),), 0x77, dtype=torch.uint8, device=plan.device)
        toffs = torch.full((int(plan.info.tiles) + 1,), 0x7777777777777777, dtype=torch.int64, device=plan.device)
        kept = torch.full((T["n"],), 0x77, dtype=torch.uint8, device=plan.device)
        chosen = torch.full((F,), 0x7777777777777777, dtype=torch.int64, device=plan.device)
        ach = torch.full((F,), 0x7777777777777777, dtype=torch.int64, device=plan.device).view(torch.float64)
        back = torch.full(batch.shape, 0x77, dtype=torch.uint8, device=plan.device)

        def untouched():
            ctx.sync()
            assert bool((out == 0x77).all()) and bool((toffs == 0x7777777777777777).all()) and bool((kept == 0x77).all())
            assert bool((chosen == 0x7777777777777777).all()) and bool((ach.view(torch.int64) == 0x7777777777777777).all()) and bool((back == 0x77).all())

        def enc(**kw):
            return plan.encode_frame_pixels(fmt, d_pix, out=out, tile_offs=toffs, **kw)

        def alloc(**kw):
            return plan.rate_allocate(T["rate"], T["dist"], T["nbs"], kept=kept, chosen=chosen, **kw)

        def allocq(**kw):
            return plan.rate_allocate_quality(T["rate"], T["dist"], T["nbs"], kept=kept, chosen=chosen, achieved=ach, **kw)

        # Python: a wrong length, a per-frame argument beside another cut, a tensor that is too small
        for call in (lambda: enc(frame_bytes=[1, 2]), lambda: enc(frame_bytes=[1, 2, 3, 4]), lambda: enc(frame_psnr=[30.0]), lambda: alloc(frame_bytes=[5] * 4),
                     lambda: allocq(frame_targets=[1.0]), lambda: enc(frame_bytes=[1, 2, 3], max_body_bytes=5), lambda: enc(frame_bytes=[1, 2, 3], min_psnr=30.0),
                     lambda: enc(frame_bytes=[1, 2, 3], layer_bytes=[5, 6]), lambda: enc(frame_bytes=[1, 2, 3], roi=(0, 0, 8, 8)),
                     lambda: enc(frame_bytes=[1, 2, 3], frame_psnr=[30.0] * 3), lambda: enc(frame_distortion=[1.0] * 3, layer_psnr=[30.0]),
                     lambda: plan.rate_allocate(T["rate"], T["dist"], T["nbs"], 100, kept=kept, chosen=chosen[:2]),
                     lambda: plan.rate_allocate_layers(T["rate"], T["dist"], T["nbs"], [1, 2], chosen=chosen)):
            with pytest.raises(ValueError):
                call()
            untouched()
        # C: a wrong nframes, a negative entry, a NaN / negative / infinite target, both arrays or none
        L, h = ctx.L, plan.h
        import ctypes as C
        i64 = lambda v: (C.c_int64 * len(v))(*v)
        f64 = lambda v: (C.c_double * len(v))(*v)
        p = plan._p
        pixargs = (h, int(fmt), p(d_pix), C.c_size_t(int(d_pix.shape[1])), 0, 0)
        tail = (p(out), C.c_size_t(int(out.numel())), p(toffs), p(ach))
        tabs = (h, p(T["rate"]), p(T["dist"]), p(T["nbs"]))
        nan, inf = float("nan"), float("inf")
        for st in (L.j2k_plan_rate_allocate_frames(*tabs, i64([1, 2]), 2, 0, p(kept), p(chosen)),
                   L.j2k_plan_rate_allocate_frames(*tabs, i64([1, 2, 3, 4]), 4, 0, p(kept), p(chosen)),
                   L.j2k_plan_rate_allocate_frames(*tabs, i64([1, -2, 3]), 3, 0, p(kept), p(chosen)),
                   L.j2k_plan_rate_allocate_frames(*tabs, i64([1, 2, -3]), 3, 1, p(kept), p(chosen)),
                   L.j2k_plan_rate_allocate_quality_frames(*tabs, f64([1.0, nan, 1.0]), 3, 0, p(kept), p(chosen), p(ach)),
                   L.j2k_plan_rate_allocate_quality_frames(*tabs, f64([1.0, 1.0, -1.0]), 3, 1, p(kept), p(chosen), p(ach)),
                   L.j2k_plan_rate_allocate_quality_frames(*tabs, f64([inf, 1.0, 1.0]), 3, 0, p(kept), p(chosen), p(ach)),
                   L.j2k_plan_rate_allocate_quality_frames(*tabs, f64([1.0, 1.0]), 2, 0, p(kept), p(chosen), p(ach)),
                   L.j2k_plan_encode_frame_pixels_rate_frames(*pixargs, i64([1, 2]), None, 2, 0, *tail),
                   L.j2k_plan_encode_frame_pixels_rate_frames(*pixargs, i64([1, 2, -1]), None, 3, 0, *tail),
                   L.j2k_plan_encode_frame_pixels_rate_frames(*pixargs, None, f64([1.0, nan, 2.0]), 3, 1, *tail),
                   L.j2k_plan_encode_frame_pixels_rate_frames(*pixargs, None, f64([1.0, -0.5, 2.0]), 3, 0, *tail),
                   L.j2k_plan_encode_frame_pixels_rate_frames(*pixargs, i64([1, 2, 3]), f64([1.0, 1.0, 2.0]), 3, 0, *tail),
                   L.j2k_plan_encode_frame_pixels_rate_frames(*pixargs, None, None, 3, 0, *tail)):
            assert st == _lib.ERR_INVALID_ARG
            untouched()
        # a falling and a rising vector are both fine: the entries belong to different frames
        for v in ([300, 200, 100], [100, 200, 300]):
            assert L.j2k_plan_rate_allocate_frames(*tabs, i64(v), 3, 0, p(torch.empty_like(kept)), p(torch.empty_like(chosen))) == _lib.OK
        # roi= with F > 1, area= on a batch
        for call in (lambda: enc(max_body_bytes=1000, roi=(0, 0, 32, 32)), lambda: enc(min_psnr=30.0, roi=(0, 0, 32, 32)),
                     lambda: plan.encode_blocks(plan.alloc_coeff(), planes=True, roi=(0, 0, 32, 32)), lambda: plan.roi_windows((0, 0, 32, 32))):
            with pytest.raises(J2KError) as e:
                call()
            assert e.value.status == _lib.ERR_UNSUPPORTED, str(e.value)
            untouched()
        ah, aw = 16, 16
        small = torch.full((ah, aw * 4), 0x77, dtype=torch.uint8, device=plan.device)
        for kw in (dict(truncated=True), dict(pass_cuts=True), dict(layers=1)):
            with pytest.raises(J2KError) as e:
                plan.decode_frame_pixels(good, glen, small, area=(0, 0, 16, 16), **kw)
            assert e.value.status == _lib.ERR_UNSUPPORTED
            ctx.sync()
            assert bool((small == 0x77).all())
        ctx.sync()
    finally:
        plan.close()
    # the setter on a shard of a batch; on a whole batch given as a shard it is accepted
    nt = 2 * 6
    rows2 = fr.GEOMETRIES["tiled"][1]
    kw = dict(precision=8, lossless=True, num_resolutions=4, cb=(64, 64), tile=(128, 32), ctx=ctx, mallat=True, frame_rows=rows2)
    shard = FramePlan(260, 2 * rows2, 3, tile_first=6, tile_count=6, **kw)
    whole = FramePlan(260, 2 * rows2, 3, tile_first=0, tile_count=nt, **kw)
    try:
        with pytest.raises(J2KError) as e:
            shard.set_rate_per_frame(True)
        assert e.value.status == _lib.ERR_UNSUPPORTED and shard.rate_frames == 1
        shard.set_rate_per_frame(False)
        whole.set_rate_per_frame(True)
        assert whole.rate_frames == 2
    finally:
        shard.close(); whole.close()


# ---- the vector forms carry many frames ---------------------------------------------------------------------------------------------------------
def test_many_frames_and_capture_replays_the_values(env):
    """F = 300 frames of 16 x 8 gray (more than one chunk of the by-value table): every frame under its own budget; a captured call replays the
    budgets it was captured with after the host array is gone"""
    from j2kgfx.codec import FramePlan
    torch, orc, ctx = env
    F, W, rows = 300, 16, 8
    plan = FramePlan(W, rows * F, 1, precision=8, lossless=True, num_resolutions=2, cb=(8, 8), ctx=ctx, mallat=True, frame_rows=rows, rate_per_frame=True)
    try:
        assert plan.rate_frames == F
        n = int(plan.info.blocks)
        ranges = _ranges(plan, F)
        Rs, Ds, nbs, _ = qc.random_tables(21, n, zero_weights=False)
        ws = _weights(plan)
        R, D = np.stack(Rs), np.stack(Ds)
        dev = (torch.from_numpy(R.view(np.int32)).to(plan.device), torch.from_numpy(D.view(np.int64)).to(plan.device), torch.from_numpy(np.asarray(nbs, np.uint8)).to(plan.device))
        body = [sum(int(Rs[j][nbs[j]]) for j in range(a, a + c)) for a, c in ranges]
        vec = [(body[f] * (f % 7)) // 6 for f in range(F)]
        kept, chosen = plan.rate_allocate(*dev, frame_bytes=vec)
        ctx.sync()
        wk, wc = fr.allocate_frames(Rs, Ds, [int(x) for x in nbs], ws, ranges, vec)
        assert chosen.cpu().numpy().tolist() == wc and kept.cpu().numpy()[:n].tolist() == wk
        tv = [float(1 + 1000 * (f % 5)) for f in range(F)]
        kept, chosen, ach = plan.rate_allocate_quality(*dev, frame_targets=tv)
        ctx.sync()
        wk, wc, wa = fr.allocate_quality_frames(Rs, Ds, [int(x) for x in nbs], ws, ranges, tv)
        assert kept.cpu().numpy()[0].tolist() == wk and chosen.cpu().numpy()[0].tolist() == wc and _bits(ach.cpu().numpy()) == _bits(wa)
        # captured with `other`, replayed after calls with `vec` and with the Python list long gone
        other = [(body[f] * ((f + 3) % 7)) // 6 for f in range(F)]
        ok, oc = fr.allocate_frames(Rs, Ds, [int(x) for x in nbs], ws, ranges, other)
        assert oc != wc
        kept = torch.zeros(n, dtype=torch.uint8, device=plan.device)
        chosen = torch.zeros(F, dtype=torch.int64, device=plan.device)
        with ctx.capture() as g:
            plan.rate_allocate(*dev, frame_bytes=list(other), kept=kept, chosen=chosen)
        del other
        for _ in range(2):
            plan.rate_allocate(*dev, frame_bytes=vec, kept=kept, chosen=chosen)      # the plan's value table now holds `vec`
            ctx.sync()
            kept.zero_(); chosen.zero_()
            torch.cuda.synchronize()
            g.launch()
            ctx.sync()
            assert chosen.cpu().numpy().tolist() == oc and kept.cpu().numpy().tolist() == ok
    finally:
        plan.close()
