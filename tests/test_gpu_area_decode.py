"""GPU: the region decode (area=(x0, y0, x1, y1) of decode_frame_pixels / decode_pixels_host; j2k_plan_area_shape, j2k_plan_area_blocks,
j2k_plan_decode_frame_pixels_area, j2k_decode_pixels_host_area) against tests/area_cases.py.

The need set must equal area_cases.frame_need exactly.  The pixels must equal, bit for bit, the yardstick's FULL decode of the same call without
`area`, cropped: mallat_cases forward -> coarse(v, max(skip_planes, the block's floor)) per block -> mallat_cases inverse, the floors by
rate_cases.allocate / layer_cases.allocate_layers on the frame's tables, as tests/test_gpu_rate_frames.py and tests/test_gpu_layers.py compose
it (test_gpu_layers.Frame holds a frame's tables; the blocks' weights are recomputed from the oracle's block list, see _frame_of).  No expectation
is a device result.

Geometries, windows and reduces are area_cases.GEOMETRIES / windows / REDUCES; the (window, reduce) pairs whose reduced rectangle is empty are in
the refusal test."""
import ctypes as C

import numpy as np
import pytest

import area_cases as ac
import closed_loop_ref as ref
import coarse_cases as cc
import layer_cases as lc
import mallat_cases as mc
import rate_cases as rc
import test_gpu_layers as lyr

pytestmark = pytest.mark.gpu
INF = 1 << 62
SENTINEL = 0x5A
GIDS = [ac.geometry_id(g) for g in ac.GEOMETRIES]
VARIANTS = ("plain", "skip3", "truncated50", "layers2of3")


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    from j2kgfx import Context
    ctx = Context(0)
    yield torch, orc, ctx
    ctx.close()


def _spec(g):
    case, cb, wavelet, q = g
    return (case, wavelet == "53", q, cb)


_FRAMES, _STREAMS = {}, {}


def _frame_of(torch, plan, gi):
    if gi not in _FRAMES:
        import oracle as orc
        g = ac.GEOMETRIES[gi]
        F = _FRAMES[gi] = lyr.Frame(torch, plan, _spec(g))
        # Every block's weight from the ORACLE's block list.  Frame infers a block's resolution from the order of the bands
        # (test_gpu_rate_frames._block_res), which is off where a resolution of a narrow edge tile has no HL / HH band: 108 of the 747
        # blocks of the 200 x 150 geometry.  The plan's jobs are the oracle's, tile by tile (checked here).
        Cn, bl = g[0][2], plan.blocks()
        want = [(t * Cn + int(b["comp"]), int(b["band"]), int(b["x0"]), int(b["y0"]), int(b["w"]), int(b["h"]), int(b["res"]))
                for t, (_, tb) in enumerate(ac.tile_blocks(orc, g)) for b in tb]
        assert [q[:6] for q in want] == [tuple(int(b[k]) for k in ("plane", "band", "x0", "y0", "w", "h")) for b in bl]
        w = plan.rate_weights()
        F.ws = [float(w[q[0] % Cn, q[6], q[1]]) for q in want]
    return _FRAMES[gi]


@pytest.fixture()
def shared(env, request):
    """(geometry index, plan, test_gpu_layers.Frame): the Frame -- the picture, the oracle's coefficient tiles, the device's rate tables -- is
    made once per geometry and kept; the plan is the test's own"""
    torch, orc, ctx = env
    gi = request.param
    plan = lyr._plan(ctx, _spec(ac.GEOMETRIES[gi]))
    try:
        yield gi, plan, _frame_of(torch, plan, gi)
    finally:
        plan.close()


def _budgets(F):
    return [F.U // 10, F.U // 2, INF]                    # test_gpu_layers.BUDGETS[2]


def _streams(gi, plan, F, marks):
    """host copies of the three streams of a geometry, made once: {name: (bytes uint8, tile_offs int64)}"""
    key = (gi, marks)
    if key not in _STREAMS:
        out = {}
        for name, kw in (("plain", {}), ("cut", dict(max_body_bytes=F.U // 2)), ("layered", dict(layer_bytes=_budgets(F)))):
            res = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, **kw)
            plan.frame_status()
            cs, toffs = res[0], res[1]
            out[name] = (cs[:int(toffs[-1].item())].cpu().numpy().copy(), toffs.cpu().numpy().copy())
        _STREAMS[key] = out
    return _STREAMS[key]


def _variant(F, variant):
    """(stream name, decode keywords, planes kept per block, skip_planes) of a variant"""
    if variant == "plain":
        return "plain", {}, F.nbs, 0
    if variant == "skip3":
        return "plain", dict(skip_planes=3), F.nbs, 3
    if variant == "truncated50":
        ps, _ = rc.allocate(F.R, F.D, F.nbs, F.ws, F.U // 2)
        assert any(0 < p < nb for p, nb in zip(ps, F.nbs)), "vacuous: no block cut inside"
        return "cut", dict(truncated=True), ps, 0
    if "layers3" not in F.alloc:
        budgets = _budgets(F)
        kept, _ = lc.allocate_layers(F.R, F.D, F.nbs, F.ws, budgets)
        F.alloc["layers3"] = list(zip(*[lc.normalise(F.R[j], [kept[l][j] for l in range(3)]) for j in range(F.n)]))
    assert any(q < nb for q, nb in zip(F.alloc["layers3"][1], F.nbs)), "vacuous: two layers hold everything"
    return "layered", dict(layers=2), F.alloc["layers3"][1], 0


def _dev(torch, plan, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(plan.device)


def _decode_area(torch, plan, d_cs, total, d_toffs, marks, area, r, bpp, **kw):
    """decode into a sentinel-filled buffer of area_shape with 8 bytes of row padding -> (pixels, padding)"""
    h, w = plan.area_shape(area, r)
    back = torch.full((h, w * bpp + 8), SENTINEL, dtype=torch.uint8, device=plan.device)
    plan.decode_frame_pixels(d_cs, total, back, tile_offs=d_toffs, sop=marks, eph=marks, reduce=r, area=area, **kw)
    plan.frame_status()
    out = back.cpu().numpy()
    return out[:, :w * bpp], out[:, w * bpp:]


# ---- the need set ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", range(len(ac.GEOMETRIES)), ids=GIDS, indirect=True)
def test_area_blocks(env, shared):
    torch, orc, ctx = env
    gi, plan, F = shared
    (W, H, Cn, prec, tile, nres), cb, wavelet, q = ac.GEOMETRIES[gi]
    blocks = plan.blocks()
    for area, r in ac.window_cases(W, H):
        want = ac.frame_need(blocks, Cn, W, H, tile, nres, r, area, wavelet)
        got = plan.area_blocks(area, r)
        ctx.sync()
        assert np.array_equal(got.cpu().numpy().astype(bool), want), (area, r)
        x0, y0, x1, y1 = ac.output_rect(area, r)
        assert plan.area_shape(area, r) == (y1 - y0, x1 - x0)
        if (gi, area, r) in ac.COUNTS:
            assert (int(want.sum()), len(blocks)) == ac.COUNTS[(gi, area, r)]
        if area == (0, 0, W, H) and r == 0:
            assert want.all()


# ---- the pixels -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("marks", [False, True], ids=["bare", "sop_eph"])
@pytest.mark.parametrize("shared", range(len(ac.GEOMETRIES)), ids=GIDS, indirect=True)
def test_pixels_are_the_crop_of_the_full_decode(env, shared, marks, variant):
    torch, orc, ctx = env
    gi, plan, F = shared
    (W, H, Cn, prec, tile, nres) = ac.GEOMETRIES[gi][0]
    bpp = ac.bytes_per_pixel(Cn, prec)
    name, kw, kept, skip = _variant(F, variant)
    h_cs, h_toffs = _streams(gi, plan, F, marks)[name]
    d_cs, d_toffs = _dev(torch, plan, h_cs), _dev(torch, plan, h_toffs)
    for i, (area, r) in enumerate(ac.window_cases(W, H)):
        full = F.expected(orc, _spec(ac.GEOMETRIES[gi]), kept, skip, r)
        got, pad = _decode_area(torch, plan, d_cs, int(h_cs.size), d_toffs if i % 2 else None, marks, area, r, bpp, **kw)
        assert np.array_equal(got, ac.crop(full, area, r, bpp)), (area, r)
        assert (pad == SENTINEL).all(), (area, r)
    if variant == "plain" and ac.GEOMETRIES[gi][2] == "53" and prec == 8:     # (the lossless loop hands the picture back)
        assert np.array_equal(F.expected(orc, _spec(ac.GEOMETRIES[gi]), kept, 0, 0), F.pix)


def test_blocks_outside_the_need_set_take_no_part(env):
    """every byte of the bodies of the blocks that are not needed overwritten (0x00 ... 0x7F: no marker appears): the same pixels"""
    torch, orc, ctx = env
    gi = 0
    g = ac.GEOMETRIES[gi]
    (W, H, Cn, prec, tile, nres), cb, wavelet, q = g
    bpp = ac.bytes_per_pixel(Cn, prec)
    plan = lyr._plan(ctx, _spec(g))
    try:
        F = _frame_of(torch, plan, gi)
        rng = np.random.default_rng(5)
        for marks in (False, True):
            h_cs, h_toffs = _streams(gi, plan, F, marks)["plain"]
            d_cs = _dev(torch, plan, h_cs)
            offs, lens, _nb = plan.decode_tile_parts(d_cs, int(h_cs.size), sop=marks, eph=marks)
            plan.frame_status()
            offs, lens = offs.cpu().numpy()[:F.n], lens.cpu().numpy().view(np.uint32)[:F.n]
            for area, r in (((37, 11, 90, 40), 0), ((0, 0, 1, 1), 1), ((W // 2 - 9, H // 2 - 7, W // 2 + 8, H // 2 + 6), 2)):
                need = ac.frame_need(plan.blocks(), Cn, W, H, tile, nres, r, area, wavelet)
                bad = h_cs.copy()
                changed = 0
                for j in np.nonzero(~need)[0]:
                    a, n = int(offs[j]), int(lens[j])
                    bad[a:a + n] = rng.integers(0, 0x80, n).astype(np.uint8)
                    changed += n
                assert changed * 2 > int(lens.sum()) and not np.array_equal(bad, h_cs)      # most of the body bytes are gone
                got, pad = _decode_area(torch, plan, _dev(torch, plan, bad), int(bad.size), None, marks, area, r, bpp)
                assert np.array_equal(got, ac.crop(F.expected(orc, _spec(g), F.nbs, 0, r), area, r, bpp)), (marks, area, r)
    finally:
        plan.close()


@pytest.mark.parametrize("shared", [1, 3], ids=[GIDS[1], GIDS[3]], indirect=True)
def test_whole_frame_window_is_the_call_without_area(env, shared):
    torch, orc, ctx = env
    gi, plan, F = shared
    (W, H, Cn, prec, tile, nres) = ac.GEOMETRIES[gi][0]
    bpp = ac.bytes_per_pixel(Cn, prec)
    for variant in VARIANTS:
        name, kw, _kept, _skip = _variant(F, variant)
        h_cs, h_toffs = _streams(gi, plan, F, True)[name]
        d_cs = _dev(torch, plan, h_cs)
        for r in ac.REDUCES:
            Hr, Wr = plan.reduced_shape(r)
            assert plan.area_shape((0, 0, W, H), r) == (Hr, Wr)
            x = torch.full((Hr, Wr * bpp + 8), SENTINEL, dtype=torch.uint8, device=plan.device)
            y = x.clone()
            plan.decode_frame_pixels(d_cs, int(h_cs.size), x, sop=True, eph=True, reduce=r, **kw)
            plan.decode_frame_pixels(d_cs, int(h_cs.size), y, sop=True, eph=True, reduce=r, area=(0, 0, W, H), **kw)
            plan.frame_status()
            assert torch.equal(x, y) and not bool((x[:, :Wr * bpp] == SENTINEL).all()), (variant, r)


@pytest.mark.parametrize("shared", [0, 2], ids=[GIDS[0], GIDS[2]], indirect=True)
def test_host_one_call_form(env, shared):
    torch, orc, ctx = env
    gi, plan, F = shared
    (W, H, Cn, prec, tile, nres) = ac.GEOMETRIES[gi][0]
    bpp = ac.bytes_per_pixel(Cn, prec)
    area = (W // 2 - 9, H // 2 - 7, W // 2 + 8, H // 2 + 6)
    for variant, r in (("plain", 0), ("skip3", 1), ("truncated50", 2), ("layers2of3", 1)):
        name, kw, kept, skip = _variant(F, variant)
        h_cs, h_toffs = _streams(gi, plan, F, True)[name]
        dev, _ = _decode_area(torch, plan, _dev(torch, plan, h_cs), int(h_cs.size), None, True, area, r, bpp, **kw)
        h, w = plan.area_shape(area, r)
        host = plan.decode_pixels_host(h_cs, (h, w * bpp), sop=True, eph=True, reduce=r, area=area, **kw)
        assert np.array_equal(host, dev), (variant, r)
        assert np.array_equal(host, ac.crop(F.expected(orc, _spec(ac.GEOMETRIES[gi]), kept, skip, r), area, r, bpp)), (variant, r)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    torch, orc, ctx = env
    from j2kgfx import J2KError, _lib
    from j2kgfx.codec import FramePlan

    def status(fn):
        try:
            fn()
        except J2KError as e:
            assert str(e)
            return e.status
        return _lib.OK
    gi = 1
    g = ac.GEOMETRIES[gi]
    (W, H, Cn, prec, tile, nres), cb, wavelet, q = g
    L = mc.levels_of(nres)

    def mk(**kw):
        kw.setdefault("mallat", True)
        return FramePlan(W, kw.pop("height", H), Cn, precision=prec, lossless=True, num_resolutions=nres, cb=(cb, cb), tile=tile, coder=kw.pop("coder", 0), ctx=ctx, **kw)
    plan = mk()
    others = dict(prefix=mk(mallat=False, closed_loop=True), ht=mk(coder=1), batch=mk(height=2 * H, frame_rows=H), shard=mk(tile_first=1, tile_count=2))
    try:
        F = _frame_of(torch, plan, gi)
        h_cs, h_toffs = _streams(gi, plan, F, False)["plain"]
        d_cs, total = _dev(torch, plan, h_cs), int(h_cs.size)
        area = (37, 11, 90, 40)
        ah, aw = plan.area_shape(area, 0)
        sentinel = torch.full((ah, aw * 4), SENTINEL, dtype=torch.uint8, device=plan.device)
        h_sentinel = np.full((ah, aw * 4), SENTINEL, np.uint8)

        def every_call(p, a, r, **kw):
            """the status of each of the four entries; all must agree"""
            st = {status(lambda: p.area_shape(a, r)), status(lambda: p.area_blocks(a, r)),
                  status(lambda: p.decode_frame_pixels(d_cs, total, sentinel, reduce=r, area=a, **kw)),
                  status(lambda: p.decode_pixels_host(h_cs, h_sentinel.shape, reduce=r, area=a, pix=h_sentinel, **kw))}
            assert len(st) == 1, st
            return st.pop()
        # plans
        for name, p in others.items():
            assert every_call(p, area, 0) == _lib.ERR_UNSUPPORTED, name
        # rectangles: inverted, empty, outside the frame, empty after reduce
        for a in ((90, 11, 37, 40), (37, 40, 90, 11), (37, 11, 37, 40), (37, 11, 90, 11), (-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, W + 1, 4), (0, 0, 4, H + 1), (W, 0, W + 1, 4)):
            assert every_call(plan, a, 0) == _lib.ERR_INVALID_ARG, a
        for a, r in ac.empty_cases(W, H):
            assert every_call(plan, a, r) == _lib.ERR_INVALID_ARG, (a, r)
        # a pix buffer that is not area_shape: a row too many, a row too few, a stride shorter than a row
        for shape in ((ah + 1, aw * 4), (ah - 1, aw * 4), (ah, aw * 4 - 4)):
            buf = torch.full(shape, SENTINEL, dtype=torch.uint8, device=plan.device)
            assert status(lambda: plan.decode_frame_pixels(d_cs, total, buf, area=area)) == _lib.ERR_INVALID_ARG, shape
            ctx.sync()
            assert bool((buf == SENTINEL).all())
            if shape[0] != ah:
                assert status(lambda: plan.decode_pixels_host(h_cs, shape, area=area)) == _lib.ERR_INVALID_ARG, shape
        r = ctx.L.j2k_plan_decode_frame_pixels_area(plan.h, plan._p(d_cs), C.c_size_t(total), None, 0, 0, 0, 0, 0, 0, C.byref(_lib.Rect(*area)), plan._p(sentinel),
                                                    C.c_size_t(aw * 4 - 4))
        assert r == _lib.ERR_INVALID_ARG
        # what the call without `area` refuses: reduce outside 0 ... L, skip_planes and layers out of range
        for bad in (-1, L + 1):
            assert every_call(plan, area, bad) == _lib.ERR_INVALID_ARG, bad
        for kw in (dict(skip_planes=-1), dict(skip_planes=32), dict(layers=33), dict(layers=-1)):
            assert status(lambda: plan.decode_frame_pixels(d_cs, total, sentinel, area=area, **kw)) == _lib.ERR_INVALID_ARG, kw
            assert status(lambda: plan.decode_pixels_host(h_cs, h_sentinel.shape, area=area, pix=h_sentinel, **kw)) == _lib.ERR_INVALID_ARG, kw
        ctx.sync()
        assert bool((sentinel == SENTINEL).all()) and (h_sentinel == SENTINEL).all()

        # a stream the decoder refuses leaves the caller's buffer alone, on the device and on the host
        def cut_short():
            plan.decode_frame_pixels(d_cs, total // 2, sentinel, area=area)
            plan.frame_status()
        assert status(cut_short) == _lib.ERR_INVALID_ARG
        assert bool((sentinel == SENTINEL).all())
        assert status(lambda: plan.decode_pixels_host(h_cs[:total // 2], h_sentinel.shape, area=area, pix=h_sentinel)) == _lib.ERR_INVALID_ARG
        assert (h_sentinel == SENTINEL).all()
        # ... and the same call on the whole stream writes it
        plan.decode_frame_pixels(d_cs, total, sentinel, area=area)
        plan.frame_status()
        assert np.array_equal(sentinel.cpu().numpy(), ac.crop(F.expected(orc, _spec(g), F.nbs, 0, 0), area, 0, 4))
    finally:
        plan.close()
        for p in others.values():
            p.close()


# ---- graph capture --------------------------------------------------------------------------------------------------------------------------
def test_graph(env):
    """one area call (reduce = 1, skip_planes = 2) captured after a warm call, replayed on a second stream of the same geometry: the rectangle is
    an argument of the captured launches, the streams are what the buffers hold"""
    torch, orc, _ = env
    from j2kgfx import Context
    g = ac.GEOMETRIES[1]
    (W, H, Cn, prec, tile, nres), cb, wavelet, q = g
    fmt, bpp = mc.PIX_FORMAT[(Cn, prec)], ac.bytes_per_pixel(Cn, prec)
    area, r, k = (W // 2 - 9, H // 2 - 7, W // 2 + 8, H // 2 + 6), 1, 2
    ctx = Context(0)
    plan = lyr._plan(ctx, _spec(g))
    try:
        streams, exps = [], []
        for seed in (81, 82):
            pix, _, _, planes = ref.pixel_frame(fmt, W, H, seed, orc, noise=(1 << prec) // 16)
            tiles = mc.forward_frame(orc, planes, tile, prec, nres, True, 0)
            cs, toffs = plan.encode_frame_pixels(fmt, _dev(torch, plan, pix), sop=True, eph=True)
            plan.frame_status()
            streams.append((cs.clone(), toffs.clone()))
            full = mc.pixels(orc, mc.inverse_frame(orc, cc.coarse_tiles(tiles, k), W, H, tile, prec, nres, reduce=r), prec)
            exps.append(ac.crop(full, area, r, bpp))
        assert not np.array_equal(exps[0], exps[1])
        cs, toffs = streams[0][0].clone(), streams[0][1].clone()
        back = torch.zeros(exps[0].shape, dtype=torch.uint8, device=plan.device)
        kw = dict(tile_offs=toffs, sop=True, eph=True, reduce=r, skip_planes=k, area=area)
        plan.decode_frame_pixels(cs, int(cs.numel()), back, **kw)      # warm: makes the tables of reduce 1 and of the region decode
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exps[0])
        with ctx.capture() as gr:
            plan.decode_frame_pixels(cs, int(cs.numel()), back, **kw)
        for i in (1, 0, 1):
            cs.copy_(streams[i][0])
            toffs.copy_(streams[i][1])
            back.zero_()
            torch.cuda.synchronize()
            gr.launch()
            ctx.sync()
            assert np.array_equal(back.cpu().numpy(), exps[i]), i
        gr.close()
    finally:
        plan.close()
