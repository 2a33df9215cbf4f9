"""GPU: quality layers end to end against tests/layer_cases.py -- rate_allocate_layers, encode_frame_pixels(layer_bytes=...), decode_frame_pixels
(layers=k), the stage calls, codestream.keep_layers, the host one-call forms, the refusals and the pinned streams.

Plans: Mallat MQ plans; coarse_cases.FRAME_CASES[0] (untiled, 4 resolutions) and [1] (128 x 32 tiles: several tiles, edge tiles, one chain per
tile), mallat_cases.LOSSY[0] as 9-7 with the dequantiser, all with 64 x 64 blocks, and a 200 x 150 gray frame with 3 resolutions and 16 x 16
blocks whose finest packet holds 105 blocks (more than the packet kernels' lane chunk of 64).  Budgets (U = the uncut body bytes): [50 %];
[0, 2^62] (an empty first layer: every first inclusion above layer 0, behind a presence-bit-0 packet); [10 %, 50 %, 2^62]; [5 %, 5 %, 20 %, U,
2^62] (a repeated budget and an exact U: empty middle and last layers).  The tables R, D of a frame come from encode_blocks(planes=True) (held to
the oracle in tests/test_gpu_rate_encode.py); everything after them is the yardstick's, and every comparison is bit for bit."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import coarse_cases as cc
import layer_cases as lc
import mallat_cases as mc
import rate_cases as rc
import test_gpu_rate_frames as rf

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF = 1 << 62
# (case, lossless, quality, cb)
PLANS = [(cc.FRAME_CASES[0], True, 0, 64), (cc.FRAME_CASES[1], True, 0, 64), (mc.LOSSY[0][:6], False, mc.LOSSY[0][6], 64), ((200, 150, 1, 8, (0, 0), 3), True, 0, 16)]
PLAN_IDS = ["130x70x3", "260x44x3-tiled", "130x70x3-97q%d" % mc.LOSSY[0][6], "200x150x1-cb16"]
BUDGETS = [lambda U: [U // 2], lambda U: [0, INF], lambda U: [U // 10, U // 2, INF], lambda U: [U // 20, U // 20, U // 5, U, INF]]
BUDGET_IDS = ["L1", "L2-empty-first", "L3", "L5-repeats"]


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    from j2kgfx import Context
    ctx = Context(0)
    yield torch, orc, ctx
    ctx.close()


def _plan(ctx, spec, **kw):
    from j2kgfx.codec import FramePlan
    (W, H, Cn, prec, tile, nres), lossless, q, cb = spec
    return FramePlan(W, H, Cn, precision=prec, lossless=lossless, quality=q, num_resolutions=nres, cb=(cb, cb), tile=tile, coder=0, ctx=ctx, mallat=True,
                     dequantize=not lossless, **kw)


def _slot_offsets(plan):
    from j2kgfx import entropy
    offs, pos = [], 0
    for b in plan.blocks():
        offs.append(pos)
        pos += (entropy.block_bound(0, int(b["w"]), int(b["h"])) + 15) & ~15
    return offs


class Frame:
    """everything a plan's checks share, made once per plan spec: the frame, the oracle's coefficient tiles, the device's tables, the packets"""

    def __init__(self, torch, plan, spec):
        case, lossless, q, cb = spec
        W, H, Cn, prec, tile, nres = case
        self.fmt = mc.PIX_FORMAT[(Cn, prec)]
        self.pix, self.ctiles = rf._frame(case, lossless, q)
        self.d_pix = torch.from_numpy(self.pix).to(plan.device)
        coeff = plan.forward_pixels(self.fmt, self.d_pix)
        slots, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True)
        plan.ctx.sync()
        self.dev = (slots, lens, nbs, rate, dist)
        n = self.n = int(plan.info.blocks)
        self.R = rate.cpu().numpy().view(np.uint32)[:n].astype(np.int64)          # [blocks, 32]
        self.D = dist.cpu().numpy().view(np.uint64)[:n]
        self.nbs = [int(x) for x in nbs.cpu().numpy()[:n]]
        self.lens = [int(x) for x in lens.cpu().numpy().view(np.uint32)[:n]]
        h_slots, so = slots.cpu().numpy(), _slot_offsets(plan)
        self.datas = [bytes(h_slots[so[j]:so[j] + self.lens[j]]) for j in range(n)]
        w, res, bl = plan.rate_weights(), rf._block_res(plan), plan.blocks()
        self.ws = [float(w[int(b["plane"]) % Cn, res[j], int(b["band"])]) for j, b in enumerate(bl)]
        self.wins = rf._windows(plan, self.ctiles, Cn)
        self.U = sum(self.lens)
        self.tiles = [[] for _ in range(int(plan.info.tiles))]
        for j, b in enumerate(bl):
            t = int(b["plane"]) // Cn
            if j == 0 or (int(bl[j - 1]["plane"]), res[j - 1]) != (int(b["plane"]), res[j]):
                self.tiles[t].append([])
            self.tiles[t][-1].append(j)
        self.alloc = {}
        self.pixel_cache = {}

    def cuts(self, bi):
        """(budgets, kept [L][n], chosen [L], Q [L][n]) of budget family bi by the yardstick"""
        if bi not in self.alloc:
            budgets = BUDGETS[bi](self.U)
            kept, chosen = lc.allocate_layers(self.R, self.D, self.nbs, self.ws, budgets)
            Q = list(zip(*[lc.normalise(self.R[j], [kept[l][j] for l in range(len(kept))]) for j in range(self.n)]))
            self.alloc[bi] = (budgets, kept, chosen, Q)
        return self.alloc[bi]

    def expected(self, orc, spec, Qk, skip, reduce):
        case, lossless, q, cb = spec
        floors = tuple(max(skip, nb - qk) for nb, qk in zip(self.nbs, Qk))
        key = (floors, reduce)
        if key not in self.pixel_cache:
            self.pixel_cache[key] = rf._expected_pixels(orc, case, lossless, q, self.ctiles, self.wins, floors, reduce)
        return self.pixel_cache[key]


_FRAMES = {}


@pytest.fixture()
def shared(env, request):
    """(plan, Frame) of the test's plan spec; the Frame is made once and kept, the plan is the test's own"""
    torch, orc, ctx = env
    pi = request.param
    plan = _plan(ctx, PLANS[pi])
    try:
        if pi not in _FRAMES:
            _FRAMES[pi] = Frame(torch, plan, PLANS[pi])
        yield pi, plan, _FRAMES[pi]
    finally:
        plan.close()


def _dev_i64(torch, plan, a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(plan.device)


# ---- 1. the allocation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", range(len(PLANS)), ids=PLAN_IDS, indirect=True)
def test_rate_allocate_layers(env, shared):
    torch, orc, ctx = env
    pi, plan, F = shared
    slots, lens, nbs, rate, dist = plan.encode_blocks(plan.forward_pixels(F.fmt, F.d_pix), planes=True)
    for bi in range(len(BUDGETS)):
        budgets, kept, chosen, Q = F.cuts(bi)
        d_kept, d_chosen = plan.rate_allocate_layers(rate, dist, nbs, budgets)
        plan.ctx.sync()
        assert d_kept.cpu().numpy().tolist() == kept, BUDGET_IDS[bi]
        assert d_chosen.cpu().numpy().tolist() == chosen, BUDGET_IDS[bi]
        if len(budgets) == 1:
            k1, c1 = plan.rate_allocate(rate, dist, nbs, budgets[0])
            plan.ctx.sync()
            assert torch.equal(k1[:F.n], d_kept[0]) and int(c1.item()) == int(d_chosen[0].item())
    # the layers are not vacuous: the ordinary case cuts inside blocks in its first two layers and ends uncut
    budgets, kept, chosen, Q = F.cuts(2)
    assert any(0 < kept[0][j] < F.nbs[j] for j in range(F.n)) and kept[2] == F.nbs and chosen[0] < chosen[1] < chosen[2] == F.U


# ---- 2. the frame encode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bi", range(len(BUDGETS)), ids=BUDGET_IDS)
@pytest.mark.parametrize("shared", range(len(PLANS)), ids=PLAN_IDS, indirect=True)
def test_encode_frame_pixels_layers(env, shared, bi):
    import t2ref
    torch, orc, ctx = env
    pi, plan, F = shared
    budgets, kept, chosen, Q = F.cuts(bi)
    L = len(budgets)
    for marks in (False, True):
        want, wtoffs, wloffs = lc.compose(t2ref, F.tiles, F.datas, F.nbs, F.R, kept, marks, marks)
        cs, toffs, loffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, layer_bytes=budgets)
        plan.frame_status()
        assert toffs.cpu().numpy().tolist() == wtoffs and loffs.cpu().numpy().tolist() == wloffs, marks
        assert bytes(cs.cpu().numpy()[:wtoffs[-1]]) == want, marks
        if L == 1:
            one, otoffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, max_body_bytes=budgets[0])
            plan.frame_status()
            assert otoffs.cpu().numpy().tolist() == wtoffs and bytes(one.cpu().numpy()[:wtoffs[-1]]) == want
    if bi == 1:                                                      # the empty first layer: presence-bit-0 packets only
        assert not any(Q[0]) and all(int(wloffs[t * L]) - int(wtoffs[t]) == 14 + 9 * len(F.tiles[t]) for t in range(len(F.tiles)))
    if bi == 3:                                                      # a repeated budget and an exact U: layers that add nothing
        assert Q[1] == Q[0] and Q[4] == Q[3] == tuple(q for q in Q[3])


# ---- 3. + 4. the frame decode, keep_layers, the stage decode --------------------------------------------------------------------------------------
@pytest.mark.parametrize("bi", range(len(BUDGETS)), ids=BUDGET_IDS)
@pytest.mark.parametrize("shared", range(len(PLANS)), ids=PLAN_IDS, indirect=True)
def test_decode_layers(env, shared, bi):
    from j2kgfx import codestream
    torch, orc, ctx = env
    pi, plan, F = shared
    spec = PLANS[pi]
    (W, H, Cn, prec, tile, nres), lossless = spec[0], spec[1]
    budgets, kept, chosen, Q = F.cuts(bi)
    L = len(budgets)
    marks = bi % 2 == 1
    cs, toffs, loffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, layer_bytes=budgets)
    plan.frame_status()
    length = int(toffs[-1].item())
    h_cs, h_toffs, h_loffs = cs.cpu().numpy()[:length], toffs.cpu().numpy(), loffs.cpu().numpy()
    for k in range(1, L + 1):
        for r in (0, 1):
            assert r in mc.admissible(W, H, tile, nres)
            for skip in (0, 3):
                exp = F.expected(orc, spec, Q[k - 1], skip, r)
                back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
                plan.decode_frame_pixels(cs, length, back, tile_offs=toffs if skip else None, sop=marks, eph=marks, reduce=r, skip_planes=skip, layers=k)
                plan.frame_status()
                assert np.array_equal(back.cpu().numpy(), exp), (k, r, skip)
        if k == L and lossless and budgets[-1] == INF:
            assert np.array_equal(F.expected(orc, spec, Q[k - 1], 0, 0), F.pix)        # every layer: the input pixels exactly
        # 4. the stream cut to k layers on the host, decoded with layers = k ...
        cut, ctoffs = codestream.keep_layers(h_cs, h_toffs, h_loffs, k)
        d_cut = torch.from_numpy(np.frombuffer(cut, np.uint8).copy()).to(plan.device)
        exp = F.expected(orc, spec, Q[k - 1], 0, 0)
        back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(d_cut, len(cut), back, tile_offs=_dev_i64(torch, plan, ctoffs) if k % 2 else None, sop=marks, eph=marks, layers=k)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp), ("keep", k)
        # ... and the stage call on it: the gathered bytes data[:R[Q_k]], the yardstick's floors
        dense, o2, l2, n2, f2 = plan.decode_tile_parts(d_cut, len(cut), sop=marks, eph=marks, layers=k)
        plan.frame_status()
        h_dense, o2, l2, n2, f2 = dense.cpu().numpy(), o2.cpu().numpy(), l2.cpu().numpy().view(np.uint32), n2.cpu().numpy(), f2.cpu().numpy()
        for j in range(F.n):
            q, nb = Q[k - 1][j], F.nbs[j]
            want = F.datas[j][:int(F.R[j][q])] if q else b""
            assert int(l2[j]) == len(want) and bytes(h_dense[int(o2[j]):int(o2[j]) + len(want)]) == want, (k, j)
            assert (int(f2[j]), int(n2[j])) == ((nb - q, nb) if q else (0, 0)), (k, j)
        if k == 1:                                                   # decode_blocks + place_blocks on the gathered tables = the coarsened coefficients
            placed = plan.place_blocks(plan.decode_blocks(dense, _dev_i64(torch, plan, o2), _dev_u32(torch, plan, l2), torch.from_numpy(n2).to(plan.device),
                                                          floors=torch.from_numpy(f2).to(plan.device)))
            plan.frame_status()
            hp = placed.cpu().numpy()
            cutc = [t.copy() for t in F.ctiles]
            for (t, c, ys, xs), nb, q in zip(F.wins, F.nbs, Q[0]):
                cutc[t][c, ys, xs] = cc.coarse(F.ctiles[t][c, ys, xs], nb - q)
            for t_, c_, _x0, _y0, w_, h_, off in (tuple(int(v) for v in row) for row in plan.planes()):
                assert np.array_equal(hp[off:off + w_ * h_].reshape(h_, w_), cutc[t_][c_]), (t_, c_)


def _dev_u32(torch, plan, a):
    return torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32).copy()).to(plan.device)


# ---- 5. the host one-call forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [0, 1], ids=PLAN_IDS[:2], indirect=True)
def test_host_one_call_forms(env, shared):
    torch, orc, ctx = env
    pi, plan, F = shared
    spec = PLANS[pi]
    budgets, kept, chosen, Q = F.cuts(2)
    got = plan.encode_pixels_host(F.fmt, F.pix, sop=True, eph=True, layer_bytes=budgets)
    cs, toffs, loffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=True, eph=True, layer_bytes=budgets)
    plan.frame_status()
    assert bytes(got["bytes"]) == bytes(cs.cpu().numpy()[:int(toffs[-1].item())])
    assert got["tile_offs"].tolist() == toffs.cpu().numpy().tolist() and got["layer_offs"].tolist() == loffs.cpu().numpy().tolist()
    assert got["lens"].tolist() == F.lens and got["numbps"].tolist() == F.nbs
    for k, r, skip in ((1, 0, 0), (2, 1, 3), (3, 0, 0)):
        exp = F.expected(orc, spec, Q[k - 1], skip, r)
        host = plan.decode_pixels_host(got["bytes"], exp.shape, sop=True, eph=True, reduce=r, skip_planes=skip, layers=k)
        assert np.array_equal(host, exp), (k, r, skip)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why,kw", [
    ("ht", dict(coder=1)),
    ("batch", dict(frame_rows=35)),
    ("no_closed_loop", dict(mallat=False)),
])
def test_plan_refusals(env, why, kw):
    torch, orc, ctx = env
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    from j2kgfx.codec import FramePlan
    kw = dict(kw)
    plan = FramePlan(130, 70, 3, precision=8, lossless=True, num_resolutions=4, cb=(64, 64), coder=kw.pop("coder", 0), ctx=ctx, mallat=kw.pop("mallat", True), **kw)
    try:
        pix = torch.zeros((70, 130 * 4), dtype=torch.uint8, device=plan.device)
        out = torch.full((1 << 16,), 0x77, dtype=torch.uint8, device=plan.device)
        back = torch.full((70, 130 * 4), 0x5A, dtype=torch.uint8, device=plan.device)
        with pytest.raises(J2KError) as e:
            plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, layer_bytes=[1000, 2000])
        assert e.value.status == _lib.ERR_UNSUPPORTED
        with pytest.raises(J2KError) as e:
            plan.decode_frame_pixels(out, 1 << 16, back, layers=1)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        ctx.sync()
        assert bool((out == 0x77).all()) and bool((back == 0x5A).all())   # refused before any launch
    finally:
        plan.close()


@pytest.mark.parametrize("shared", [0], ids=PLAN_IDS[:1], indirect=True)
def test_argument_refusals(env, shared):
    torch, orc, ctx = env
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    pi, plan, F = shared
    out = torch.full((1 << 17,), 0x77, dtype=torch.uint8, device=plan.device)
    slots, lens, nbs, rate, dist = F.dev
    for bad in ([], [100, 50], [-1, 10], [10, -1], list(range(33))):
        with pytest.raises(J2KError) as e:
            plan.encode_frame_pixels(F.fmt, F.d_pix, out=out, layer_bytes=bad)
        assert e.value.status == _lib.ERR_INVALID_ARG, bad
        with pytest.raises(J2KError) as e:
            plan.rate_allocate_layers(rate, dist, nbs, bad)
        assert e.value.status == _lib.ERR_INVALID_ARG, bad
        with pytest.raises(J2KError) as e:
            plan.encode_pixels_host(F.fmt, F.pix, layer_bytes=bad)
        assert e.value.status == _lib.ERR_INVALID_ARG, bad
    with pytest.raises(J2KError) as e:
        plan.encode_frame_pixels(F.fmt, F.d_pix, out=out, layer_bytes=[10, 20], max_body_bytes=20)
    assert e.value.status == _lib.ERR_INVALID_ARG
    back = torch.full(F.pix.shape, 0x5A, dtype=torch.uint8, device=plan.device)
    for bad in (0, 33, -1):
        with pytest.raises(J2KError) as e:
            plan.decode_frame_pixels(out, 1 << 17, back, layers=bad)
        assert e.value.status == _lib.ERR_INVALID_ARG
    ctx.sync()
    assert bool((out == 0x77).all()) and bool((back == 0x5A).all())


@pytest.mark.parametrize("shared", [0, 1], ids=PLAN_IDS[:2], indirect=True)
def test_more_layers_than_the_stream_holds(env, shared):
    """layers = L + 1 on the whole stream, and layers = 2 on the stream cut to one layer (a buffer of exactly its bytes): the packet decoder's own
    error through frame_status, the caller's pixels untouched"""
    from j2kgfx import _lib, codestream
    from j2kgfx._lib import J2KError
    torch, orc, ctx = env
    pi, plan, F = shared
    budgets, kept, chosen, Q = F.cuts(2)
    for marks in (False, True):
        cs, toffs, loffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, layer_bytes=budgets)
        plan.frame_status()
        length = int(toffs[-1].item())
        cut, ctoffs = codestream.keep_layers(cs.cpu().numpy()[:length], toffs.cpu().numpy(), loffs.cpu().numpy(), 1)
        d_cut = torch.from_numpy(np.frombuffer(cut, np.uint8).copy()).to(plan.device)
        for buf, n, to, k in ((cs[:length].clone(), length, toffs, len(budgets) + 1), (d_cut, len(cut), None, 2), (d_cut, len(cut), _dev_i64(torch, plan, ctoffs), 2)):
            back = torch.full(F.pix.shape, 0x5A, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(buf, n, back, tile_offs=to, sop=marks, eph=marks, layers=k)
            with pytest.raises(J2KError) as e:
                plan.frame_status()
            assert e.value.status == _lib.ERR_INVALID_ARG
            assert bool((back == 0x5A).all())


# ---- the pinned streams ---------------------------------------------------------------------------------------------------------------------------
GOLDEN = json.load(open(os.path.join(HERE, "golden", lc.GOLDEN_FILE)))


@functools.lru_cache(None)
def _golden(name):
    import oracle as orc
    import t2ref
    return lc.golden_stream(next(c for c in lc.GOLDEN_CASES if c["name"] == name), orc, t2ref)


@pytest.mark.parametrize("case", lc.GOLDEN_CASES, ids=[c["name"] for c in lc.GOLDEN_CASES])
def test_product_writes_the_pinned_streams(env, case):
    """the stage call on the yardstick's own tables (codewords by the oracle, R by shortest_rates, cuts by allocate_layers): exactly the pinned bytes;
    and the frame decode of every prefix of them"""
    torch, orc, ctx = env
    pix, (_, tiles, datas, nbs, Rs, Ds, ws, ctiles), kept, (stream, wtoffs, wloffs) = _golden(case["name"])
    spec = (case["case"], True, 0, case["cb"])
    plan = _plan(ctx, spec)
    try:
        n, L = len(datas), len(kept)
        assert n == int(plan.info.blocks)
        rate = np.zeros((n, 32), np.uint32)
        for j in range(n):
            rate[j, :nbs[j] + 1] = Rs[j]
            rate[j, nbs[j] + 1:] = Rs[j][nbs[j]]
        offs = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64)
        d_stream = torch.from_numpy(np.frombuffer(b"".join(datas) + bytes(64), np.uint8).copy()).to(plan.device)
        cs, toffs, loffs = plan.encode_tile_parts(d_stream, _dev_i64(torch, plan, offs), _dev_u32(torch, plan, [len(d) for d in datas]),
                                                  torch.from_numpy(np.asarray(nbs, np.uint8)).to(plan.device), sop=case["marks"], eph=case["marks"],
                                                  kept=torch.from_numpy(np.asarray(kept, np.uint8)).to(plan.device), rate=_dev_u32(torch, plan, rate.reshape(-1)), layers=L)
        plan.frame_status()
        g = GOLDEN[case["name"]]
        total = int(toffs[-1].item())
        assert total == g["bytes"] and loffs.cpu().numpy().tolist() == g["layer_offs"] and toffs.cpu().numpy().tolist() == wtoffs
        assert hashlib.sha256(cs[:total].cpu().numpy().tobytes()).hexdigest() == g["sha256"]
        # every prefix decodes to the oracle's coarsened frame
        W, H, Cn, prec, tile, nres = case["case"]
        wins = rf._windows(plan, ctiles, Cn)
        for k in range(1, L + 1):
            floors = [nb - lc.normalise(Rs[j], [kept[l][j] for l in range(L)])[k - 1] for j, nb in enumerate(nbs)]
            exp = rf._expected_pixels(orc, case["case"], True, 0, ctiles, wins, floors, 0)
            back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, sop=case["marks"], eph=case["marks"], layers=k)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), k
        assert np.array_equal(exp, pix)
    finally:
        plan.close()
