"""GPU: pass-level rate control against tests/pass_cases.py, bit for bit.

  blocks      pass_cases.SHAPES x CONTENTS, each as the single block of a closed-loop plan, through the two-kernel and the one-kernel encoder form:
              spmask is the model's; R and D keep the definition's invariants, D is the model's, R[3 p - 2] / D[3 p - 2] are the tables of
              encode_blocks(planes=True); every (block, q) has the prefix property with the UNCHANGED oracle decoder at the per-sample floors of
              coarse_pass; decode_blocks(pfloors = 3 nb - 2 - q) is coarse_pass(v, nb, q, sp); pfloors = 3 k is decode_blocks(floors = k);
              skip_planes and pfloors combine as max(3 skip, pfloor)  (many blocks a launch with pfloors of their own, and codewords that are
              no prefix of a known block: tests/test_gpu_pass_streams.py)
  allocation  on a frame's 96-entry tables the device equals rate_cases.allocate / quality_cases.allocate_quality run on them (zero weights too)
  frames      130 x 70 x 3, 8 bit, 5-3 Mallat, cb 16 and 64, with and without tiles, SOP / EPH on and off: the stream is the t2ref composition, the
              pass reader's pixels are the oracle's inverse of the coarse_pass coefficients (also with reduce, skip_planes and an area), the
              truncated=True reader gives the whole-plane reading, a budget that cuts nothing gives the plain call's bytes, the host forms give the
              device forms' bytes and pixels, every refusal leaves a poisoned buffer alone
"""
import functools

import numpy as np
import pytest

import area_cases as ac
import closed_loop_ref as ref
import coarse_cases as cc
import mallat_cases as mc
import pass_cases as pc
import quality_cases as qc
import rate_cases as rc

pytestmark = pytest.mark.gpu

FORMS = {"split": dict(t1_split=1), "one_kernel": dict(t1_split=0)}


def _ctx_with(**opts):
    from j2kgfx import Context
    ctx = Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def _u(t):
    return t.cpu().numpy().view({4: np.uint32, 8: np.uint64, 1: np.uint8}[t.element_size()])


@functools.lru_cache(None)
def _model(w, h, content):
    """(v, oracle bytes, nb, sp, D, [coarse_pass at every q]) of one block -- computed once, shared by the tests, never written"""
    import oracle as orc
    v = pc.block(w, h, content)
    data, nb = orc.t1_encode(v, w, h, 0)                              # the single block of a one-resolution plan is its LL band
    nb = int(nb)
    assert nb == pc.numbps_of(v)
    sp = pc.sp_mask(v, nb)
    cuts = [pc.coarse_pass(v, nb, q, sp) for q in range(pc.points(nb) + 1)]
    for a in [v, sp] + cuts:
        a.setflags(write=False)
    return v, np.asarray(data, np.uint8), nb, sp, pc.distortion_passes(v, nb, sp), cuts


def _one_block_plan(ctx, w, h):
    from j2kgfx.codec import FramePlan
    plan = FramePlan(w, h, 1, precision=16, lossless=True, num_resolutions=1, cb=(64, 64), coder=0, ctx=ctx, closed_loop=True)
    assert int(plan.info.blocks) == 1
    return plan


# ---- blocks: the encoder's tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", pc.CONTENTS)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_block_tables(form, content):
    import torch
    import oracle as orc
    ctx = _ctx_with(**FORMS[form])
    inside = 0
    try:
        for (w, h) in pc.SHAPES:
            v, data, nb, sp, Dm, cuts = _model(w, h, content)
            plan = _one_block_plan(ctx, w, h)
            try:
                coeff = torch.from_numpy(mc.flat_coeff(plan.planes(), [v[None]], int(plan.info.coeff_elems))).to(plan.device)
                slots, lens, numbps, rate, dist, spm = plan.encode_blocks(coeff, pass_cuts=True)
                s32, l32, n32, rate32, dist32 = plan.encode_blocks(coeff, planes=True)
                ctx.sync()
                n = int(_u(lens)[0])
                assert n == len(data) == int(_u(l32)[0]) and int(numbps.cpu().numpy()[0]) == nb
                assert bytes(slots.cpu().numpy()[:n]) == bytes(data)
                # 1. the SigProp masks
                assert np.array_equal(_u(spm)[0], pc.sp_words(sp)), (w, h)
                # 2. the tables
                R, D = _u(rate)[0], _u(dist)[0]
                pc.check_tables(R, D, nb, n)
                last = pc.points(nb)
                assert [int(x) for x in D[:last + 1]] == Dm, (w, h)
                R32, D32 = _u(rate32)[0], _u(dist32)[0]
                for p in range(1, nb + 1):
                    assert int(R[3 * p - 2]) == int(R32[p]) and int(D[3 * p - 2]) == int(D32[p]), (w, h, p)
                assert int(D[0]) == int(D32[0])
                # 3. the prefix property on the unchanged oracle, at every q
                for q in range(last + 1):
                    assert pc.prefix_ok_pass(orc, data, int(R[q]), nb, 0, v, q, sp), (w, h, q, int(R[q]))
                    if q >= 1 and pc.split(q)[1] and not np.array_equal(cuts[q], cuts[q - 1]):
                        inside += 1
            finally:
                plan.close()
    finally:
        ctx.close()
    if content in ("noise", "gradient", "sparse"):
        assert inside > 0, "vacuous: no pass inside a plane changed anything"


def test_block_tables_small_symbol_workspace():
    """a frame whose left half has coefficients of 21 bits and whose right half of 6, with a symbol workspace of 1 MiB (17 planes per block) and 8
    blocks per wavefront of the lanes kernel: the context kernel hands the deep blocks on and the one-kernel passes form fills THEIR tables and masks,
    the lanes kernel the others' -- several lanes of a wavefront consuming coinciding marks at different symbols"""
    import torch
    import oracle as orc
    from j2kgfx.codec import FramePlan
    W, H, Cn, prec, tile, nres = cc.FRAME_CASES[2]
    rng = np.random.default_rng(41)
    t = rng.integers(-(1 << 6) + 1, 1 << 6, (1, H, W)).astype(np.int32)
    t[:, :, : W // 2] = rng.integers(-(1 << 21) + 1, 1 << 21, (1, H, W // 2))
    t[:, 40:, W // 2:] = 0
    t[:, 50, W - 3] = 9                                              # a nearly empty block among them
    ctx = _ctx_with(t1_lanes=8, t1_sym_mb=1)
    try:
        plan = FramePlan(W, H, Cn, precision=prec, lossless=True, num_resolutions=nres, cb=(64, 64), tile=tile, coder=0, ctx=ctx, mallat=True)
        coeff = torch.from_numpy(mc.flat_coeff(plan.planes(), [t], int(plan.info.coeff_elems))).to(plan.device)
        slots, lens, numbps, rate, dist, spm = plan.encode_blocks(coeff, pass_cuts=True)
        s32, l32, n32, rate32, dist32 = plan.encode_blocks(coeff, planes=True)
        ctx.sync()
        n = int(plan.info.blocks)
        nbs, ln = numbps.cpu().numpy()[:n], _u(lens)[:n]
        assert (nbs > 17).any() and ((nbs > 0) & (nbs <= 17)).any()
        assert torch.equal(lens[:n], l32[:n])
        R, D, R32, D32, SP, hs = _u(rate), _u(dist), _u(rate32), _u(dist32), _u(spm), slots.cpu().numpy()
        from j2kgfx import entropy
        pos, checked = 0, set()
        for j, b in enumerate(plan.blocks()):
            w, h, band, nb = int(b["w"]), int(b["h"]), int(b["band"]), int(nbs[j])
            v = np.ascontiguousarray(t[int(b["plane"]) % Cn][int(b["y0"]):int(b["y0"]) + h, int(b["x0"]):int(b["x0"]) + w])
            data = hs[pos:pos + int(ln[j])]
            pos += (entropy.block_bound(0, w, h) + 15) & ~15
            sp = pc.sp_mask(v, nb)
            assert np.array_equal(SP[j], pc.sp_words(sp)), j
            pc.check_tables(R[j], D[j], nb, int(ln[j]))
            assert [int(x) for x in D[j][:pc.points(nb) + 1]] == pc.distortion_passes(v, nb, sp), j
            for p in range(1, nb + 1):
                assert int(R[j][3 * p - 2]) == int(R32[j][p]) and int(D[j][3 * p - 2]) == int(D32[j][p]), (j, p)
            kind = nb > 17
            if nb and kind not in checked:                           # every q of one block of either kind on the oracle's decoder
                checked.add(kind)
                for q in range(pc.points(nb) + 1):
                    assert pc.prefix_ok_pass(orc, data, int(R[j][q]), nb, band, v, q, sp), (j, q)
        assert checked == {False, True}
        plan.close()
    finally:
        ctx.close()


# ---- blocks: the decoder ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", pc.CONTENTS)
def test_block_decode(content):
    import torch
    ctx = _ctx_with()
    try:
        for (w, h) in pc.SHAPES:
            v, data, nb, sp, Dm, cuts = _model(w, h, content)
            plan = _one_block_plan(ctx, w, h)
            try:
                dev = plan.device
                stream = torch.zeros(max(len(data), 1) + 64, dtype=torch.uint8, device=dev)
                stream[:len(data)] = torch.from_numpy(data.copy()).to(dev)
                offs = torch.zeros(2, dtype=torch.int64, device=dev)
                lens = torch.tensor([len(data)], dtype=torch.int32, device=dev)
                nbt = torch.tensor([nb], dtype=torch.uint8, device=dev)
                last = pc.points(nb)

                def dec(**kw):
                    out = plan.decode_blocks(stream, offs, lens, nbt, **{k: (torch.tensor([x], dtype=torch.uint8, device=dev) if k != "skip_planes" else x)
                                                                        for k, x in kw.items()})
                    ctx.sync()
                    return out.cpu().numpy()[:w * h].reshape(h, w).copy()

                # 4. every cut
                for q in range(last + 1):
                    assert np.array_equal(dec(pfloors=last - q), cuts[q]), (w, h, q)
                # (more passes left out than the block has: nothing)
                assert not dec(pfloors=last + 1).any() and not dec(pfloors=93).any()
                # 5. whole planes: the floors call, bit for bit
                for k in sorted({0, 1, 2, nb // 2, max(nb - 1, 0), nb, min(nb + 1, 31), 31}):
                    assert np.array_equal(dec(pfloors=3 * k), dec(floors=k)), (w, h, k)
                    assert np.array_equal(dec(pfloors=3 * k), cc.coarse(v, k)), (w, h, k)
                # 6. skip_planes and pfloors: max(3 skip, pfloor)
                for skip, f in ((1, 0), (1, 2), (1, 4), (2, 5), (2, 7), (0, 1), (3, 8), (nb, 1)):
                    if skip > 31:
                        continue
                    assert np.array_equal(dec(skip_planes=skip, pfloors=f), cuts[pc.q_of(nb, max(3 * skip, f))]), (w, h, skip, f)
            finally:
                plan.close()
    finally:
        ctx.close()


# ---- frames -----------------------------------------------------------------------------------------------------------------------------------
CASE = (130, 70, 3, 8)                                               # W, H, components, precision; 4 resolutions
NRES = 4
# (tiles of 80 x 48: the edge tiles are 50 x 22, every band of every resolution has samples -- _block_res below counts on that)
GEOMS = {"cb64": (64, (0, 0)), "cb16": (16, (0, 0)), "cb16_tiles": (16, (80, 48)), "cb64_tiles": (64, (80, 48))}
BUDGETS = ("0", "1", "10", "35", "80", "total-1", "total", "total+1")


def _budget(name, total):
    return {"0": 0, "1": 1, "10": total // 10, "35": total * 35 // 100, "80": total * 8 // 10, "total-1": total - 1, "total": total, "total+1": total + 1}[name]


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    from j2kgfx import Context
    ctx = Context(0)
    yield torch, orc, ctx
    ctx.close()


def _plan(ctx, geom, **kw):
    from j2kgfx.codec import FramePlan
    W, H, Cn, prec = CASE
    cb, tile = GEOMS[geom]
    kw.setdefault("mallat", True)
    return FramePlan(W, H, Cn, precision=prec, lossless=True, num_resolutions=NRES, cb=(kw.pop("cb", cb), kw.pop("cb2", cb)), tile=tile, coder=kw.pop("coder", 0), ctx=ctx, **kw)


@functools.lru_cache(None)
def _frame(tile):
    """(pix, the oracle's forward coefficient tiles) -- once per tiling, shared"""
    import oracle as orc
    W, H, Cn, prec = CASE
    pix, _, _, planes = ref.pixel_frame(mc.PIX_FORMAT[(Cn, prec)], W, H, 77, orc, noise=24)
    return pix, mc.forward_frame(orc, planes, tile, prec, NRES)


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
    """per tile its packets (lists of block numbers): a new packet where the component or the resolution changes"""
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


_TABLES = {}


def _tables(torch, ctx, geom):
    """the frame's tables, fetched ONCE per geometry: everything the frame tests expect is the Python definition run on them"""
    if geom in _TABLES:
        return _TABLES[geom]
    from j2kgfx import entropy
    W, H, Cn, prec = CASE
    pix, tiles = _frame(GEOMS[geom][1])
    plan = _plan(ctx, geom)
    try:
        coeff = plan.forward_pixels(mc.PIX_FORMAT[(Cn, prec)], torch.from_numpy(pix).to(plan.device))
        slots, lens, nbs, rate, dist, spm = plan.encode_blocks(coeff, pass_cuts=True)
        ctx.sync()
        n = int(plan.info.blocks)
        w = plan.rate_weights()
        res = _block_res(plan)
        bl = plan.blocks()
        ws = [float(w[int(b["plane"]) % Cn, res[j], int(b["band"])]) for j, b in enumerate(bl)]
        R, D = _u(rate)[:n].astype(np.int64), _u(dist)[:n]
        nb = nbs.cpu().numpy()[:n].astype(np.int64)
        ln = _u(lens)[:n].astype(np.int64)
        hs, pos, datas, wins, sps, vs = slots.cpu().numpy(), 0, [], [], [], []
        spw = _u(spm)[:n]
        for j, b in enumerate(bl):
            datas.append(hs[pos:pos + int(ln[j])].copy())
            pos += (entropy.block_bound(0, int(b["w"]), int(b["h"])) + 15) & ~15
            t, c = int(b["plane"]) // Cn, int(b["plane"]) % Cn
            ys, xs = slice(int(b["y0"]), int(b["y0"]) + int(b["h"])), slice(int(b["x0"]), int(b["x0"]) + int(b["w"]))
            wins.append((t, c, ys, xs))
            v = tiles[t][c, ys, xs]
            sp = pc.sp_mask(v, int(nb[j]))
            assert np.array_equal(spw[j], pc.sp_words(sp)), j          # (the frame's masks are the model's too)
            assert [int(x) for x in D[j][:pc.points(nb[j]) + 1]] == pc.distortion_passes(v, int(nb[j]), sp), j
            pc.check_tables(R[j], D[j], int(nb[j]), int(ln[j]))
            vs.append(v); sps.append(sp)
        out = dict(R=R, D=D, nb=nb, lens=ln, pts=[pc.points(x) for x in nb], ws=ws, datas=datas, wins=wins, sps=sps, vs=vs, packets=_packets(plan),
                   total=int(ln.sum()), rate=rate, dist=dist, nbs=nbs, n=n)
        # kept off the device tensors' plan: they are plain buffers of this context
        _TABLES[geom] = out
        return out
    finally:
        plan.close()


def _expected(orc, T, tile, qs, reduce=0, skip=0, whole_planes=False):
    """the oracle's inverse transform of the coefficients every block's cut leaves"""
    W, H, Cn, prec = CASE
    _, tiles = _frame(tile)
    cut = [t.copy() for t in tiles]
    for j, (t, c, ys, xs) in enumerate(T["wins"]):
        nb, q = int(T["nb"][j]), int(qs[j])
        if whole_planes:                                             # the older reader: p whole planes, s ignored
            q = rc.passes_of(pc.split(q)[0]) if q >= 1 else 0
        q = pc.q_of(nb, max(3 * skip, pc.pfloor_of(nb, q)))
        cut[t][c, ys, xs] = pc.coarse_pass(T["vs"][j], nb, q, T["sps"][j])
    return mc.pixels(orc, mc.inverse_frame(orc, cut, W, H, tile, prec, NRES, reduce=reduce), prec)


# ---- allocation --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["cb16", "cb64_tiles"])
def test_allocation(env, geom):
    torch, orc, ctx = env
    T = _tables(torch, ctx, geom)
    plan = _plan(ctx, geom)
    try:
        n, total = T["n"], T["total"]
        for zero in (False, True):
            ws = list(T["ws"])
            if zero:                                                 # the weights of one resolution's bands to zero
                w = plan.rate_weights()
                w[:, NRES - 1, :] = 0.0
                plan.set_rate_weights(w)
                res = _block_res(plan)
                ws = [0.0 if res[j] == NRES - 1 else ws[j] for j in range(n)]
            for name in BUDGETS:
                budget = _budget(name, total)
                kept, chosen = plan.rate_allocate(T["rate"], T["dist"], T["nbs"], budget, pass_cuts=True)
                ctx.sync()
                want, wbytes = rc.allocate(T["R"], T["D"], T["pts"], ws, budget)
                got = [int(x) for x in kept.cpu().numpy()[:n]]
                assert got == want and int(chosen.cpu().numpy()[0]) == wbytes <= budget, (name, zero)
                if name == "35" and not zero:
                    assert any(q >= 1 and pc.split(q)[1] for q in want), "vacuous: no block cut inside a plane"
                if name in ("total", "total+1"):
                    assert want == T["pts"]
            full = qc.weighted_distortion(T["D"], ws, [0] * n)
            for frac in (0.0, 1e-4, 0.01, 0.2, 1.0):
                target = full * frac
                kept, chosen, ach = plan.rate_allocate_quality(T["rate"], T["dist"], T["nbs"], [target], pass_cuts=True)
                ctx.sync()
                want, wbytes, wS = pc.allocate_quality(T["R"], T["D"], T["pts"], ws, target)
                assert [int(x) for x in kept.cpu().numpy()[0, :n]] == want, (frac, zero)
                assert int(chosen.cpu().numpy()[0]) == wbytes and qc.float_bits(float(ach.cpu().numpy()[0])) == qc.float_bits(wS) and wS <= target
        plan.set_rate_weights(None)
    finally:
        plan.close()


# ---- frames ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("marks", [False, True], ids=["bare", "sop_eph"])
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_frames(env, geom, marks):
    import t2ref
    torch, orc, ctx = env
    W, H, Cn, prec = CASE
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    cb, tile = GEOMS[geom]
    T = _tables(torch, ctx, geom)
    pix, _ = _frame(tile)
    plan = _plan(ctx, geom)
    try:
        d_pix = torch.from_numpy(pix).to(plan.device)
        n, total = T["n"], T["total"]
        plain, ptoffs = plan.encode_frame_pixels(fmt, d_pix, sop=marks, eph=marks)
        plan.frame_status()
        plain_bytes = bytes(plain.cpu().numpy()[:int(ptoffs[-1].item())])
        for name in ("35", "10", "total", "total+1", "0"):
            budget = _budget(name, total)
            qs, chosen = rc.allocate(T["R"], T["D"], T["pts"], T["ws"], budget)
            cs, toffs = plan.encode_frame_pixels(fmt, d_pix, sop=marks, eph=marks, max_body_bytes=budget, pass_cuts=True)
            plan.frame_status()
            length = int(toffs[-1].item())
            got = bytes(cs.cpu().numpy()[:length])
            assert got == pc.compose_kept_passes(t2ref, T["packets"], T["datas"], T["nb"], T["R"], qs, marks, marks), name
            if name in ("total", "total+1"):
                assert got == plain_bytes, name                      # a budget that cuts nothing
                continue
            if name == "35":
                assert any(q >= 1 and pc.split(q)[1] for q in qs), "vacuous: no block cut inside a plane"
            # the reader's tables
            o2, l2, n2, pf = plan.decode_tile_parts(cs, length, tile_offs=toffs, sop=marks, eph=marks, pfloors=True)
            plan.frame_status()
            l2, n2, pf = _u(l2)[:n], n2.cpu().numpy()[:n], pf.cpu().numpy()[:n]
            for j in range(n):
                ln = int(T["R"][j][qs[j]]) if qs[j] else 0
                assert int(l2[j]) == ln, (name, j)
                assert (int(pf[j]), int(n2[j])) == ((pc.pfloor_of(T["nb"][j], qs[j]), int(T["nb"][j])) if ln else (0, 0)), (name, j)
            assert int(l2.astype(np.int64).sum()) == chosen <= budget
            combos = ((0, 0, None),) if name != "35" else ((0, 0, None), (1, 0, None), (0, 2, None), (1, 2, None), (0, 0, (37, 9, 101, 58)), (1, 2, (37, 9, 101, 58)))
            for r, k, area in combos:
                assert r in mc.admissible(W, H, tile, NRES)
                exp = _expected(orc, T, tile, qs, reduce=r, skip=k)
                if area is not None:
                    exp = ac.crop(exp, area, r, 4)
                back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
                plan.decode_frame_pixels(cs, length, back, tile_offs=toffs if k else None, sop=marks, eph=marks, reduce=r, skip_planes=k, area=area, pass_cuts=True)
                plan.frame_status()
                assert np.array_equal(back.cpu().numpy(), exp), (name, r, k, area)
            # the older reader on the same stream: p whole planes per block, s ignored
            exp = _expected(orc, T, tile, qs, whole_planes=True)
            back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, length, back, sop=marks, eph=marks, truncated=True)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), name
    finally:
        plan.close()


def test_quality_target_frame(env):
    """one distortion target in the place of the budget: the stream of quality_cases.allocate_quality's cuts, achieved bit for bit"""
    import t2ref
    torch, orc, ctx = env
    W, H, Cn, prec = CASE
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    geom = "cb16"
    T = _tables(torch, ctx, geom)
    pix, _ = _frame(GEOMS[geom][1])
    plan = _plan(ctx, geom)
    try:
        target = plan.psnr_distortion(38.0)
        qs, wbytes, wS = pc.allocate_quality(T["R"], T["D"], T["pts"], T["ws"], target)
        assert any(q >= 1 and pc.split(q)[1] for q in qs) and any(q < p for q, p in zip(qs, T["pts"]))
        cs, toffs, ach = plan.encode_frame_pixels(fmt, torch.from_numpy(pix).to(plan.device), sop=True, eph=True, min_psnr=38.0, pass_cuts=True)
        plan.frame_status()
        got = bytes(cs.cpu().numpy()[:int(toffs[-1].item())])
        assert got == pc.compose_kept_passes(t2ref, T["packets"], T["datas"], T["nb"], T["R"], qs, True, True)
        assert qc.float_bits(float(ach.cpu().numpy()[0])) == qc.float_bits(wS) and wS <= target
        host = plan.encode_pixels_host(fmt, pix, sop=True, eph=True, max_distortion=target, pass_cuts=True)
        assert bytes(host["bytes"]) == got and qc.float_bits(float(host["achieved"][0])) == qc.float_bits(wS)
    finally:
        plan.close()


def test_stage_calls(env):
    """encode_stream's outputs -> rate_allocate(pass_cuts) -> encode_tile_parts(kept, rate, pass_cuts) give the frame call's bytes; kept = 3 nb - 2
    gives encode_tile_parts' bytes; decode_tile_parts(pfloors) + decode_blocks(pfloors) + place_blocks give the coarse_pass coefficients"""
    torch, orc, ctx = env
    W, H, Cn, prec = CASE
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    geom = "cb16_tiles"
    T = _tables(torch, ctx, geom)
    pix, tiles = _frame(GEOMS[geom][1])
    plan = _plan(ctx, geom)
    try:
        d_pix = torch.from_numpy(pix).to(plan.device)
        coeff = plan.forward_pixels(fmt, d_pix)
        slots, lens, nbs, rate, dist, spm = plan.encode_blocks(coeff, pass_cuts=True)
        offs, stream = plan.compact(slots, lens)
        n, budget = T["n"], T["total"] * 35 // 100
        kept, chosen = plan.rate_allocate(rate, dist, nbs, budget, pass_cuts=True)
        cs, toffs = plan.encode_tile_parts(stream, offs, lens, nbs, sop=True, eph=False, kept=kept, rate=rate, pass_cuts=True)
        plan.frame_status()
        cs2, toffs2 = plan.encode_frame_pixels(fmt, d_pix, sop=True, eph=False, max_body_bytes=budget, pass_cuts=True)
        plan.frame_status()
        length = int(toffs[-1].item())
        assert length == int(toffs2[-1].item()) and torch.equal(cs[:length], cs2[:length])
        allq = torch.tensor(T["pts"], dtype=torch.uint8, device=plan.device)
        full, ftoffs = plan.encode_tile_parts(stream, offs, lens, nbs, sop=True, eph=False, kept=allq, rate=rate, pass_cuts=True)
        ref_cs, rtoffs = plan.encode_tile_parts(stream, offs, lens, nbs, sop=True, eph=False)
        plan.frame_status()
        flen = int(rtoffs[-1].item())
        assert int(ftoffs[-1].item()) == flen and torch.equal(full[:flen], ref_cs[:flen])
        o2, l2, n2, pf = plan.decode_tile_parts(cs, length, sop=True, eph=False, pfloors=True)
        placed = plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2, pfloors=pf))
        plan.frame_status()
        qs = [int(x) for x in kept.cpu().numpy()[:n]]
        assert qs == rc.allocate(T["R"], T["D"], T["pts"], T["ws"], budget)[0]
        cut = [t.copy() for t in tiles]
        for j, (t, c, ys, xs) in enumerate(T["wins"]):
            cut[t][c, ys, xs] = pc.coarse_pass(T["vs"][j], int(T["nb"][j]), qs[j], T["sps"][j])
        hp = placed.cpu().numpy()
        for t_, c_, _x0, _y0, w_, h_, off in (tuple(int(v) for v in r) for r in plan.planes()):
            assert np.array_equal(hp[off:off + w_ * h_].reshape(h_, w_), cut[t_][c_]), (t_, c_)
    finally:
        plan.close()


def test_host_forms(env):
    torch, orc, ctx = env
    W, H, Cn, prec = CASE
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    geom = "cb64_tiles"
    T = _tables(torch, ctx, geom)
    tile = GEOMS[geom][1]
    pix, _ = _frame(tile)
    plan = _plan(ctx, geom)
    try:
        budget = T["total"] * 35 // 100
        qs, _ = rc.allocate(T["R"], T["D"], T["pts"], T["ws"], budget)
        got = plan.encode_pixels_host(fmt, pix, sop=True, eph=True, max_body_bytes=budget, pass_cuts=True)
        cs, toffs = plan.encode_frame_pixels(fmt, torch.from_numpy(pix).to(plan.device), sop=True, eph=True, max_body_bytes=budget, pass_cuts=True)
        plan.frame_status()
        assert bytes(got["bytes"]) == bytes(cs.cpu().numpy()[:int(toffs[-1].item())])
        assert np.array_equal(got["lens"].astype(np.int64), T["lens"]) and np.array_equal(got["numbps"].astype(np.int64), T["nb"])
        area = (37, 9, 101, 58)
        for r, k, a in ((0, 0, None), (1, 2, None), (1, 0, area)):
            exp = _expected(orc, T, tile, qs, reduce=r, skip=k)
            if a is not None:
                exp = ac.crop(exp, a, r, 4)
            host = plan.decode_pixels_host(got["bytes"], exp.shape, sop=True, eph=True, reduce=r, skip_planes=k, area=a, pass_cuts=True)
            assert np.array_equal(host, exp), (r, k, a)
    finally:
        plan.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why,kw", [
    ("ht", dict(coder=1)),
    ("batch", dict(frame_rows=35)),
    ("blocks_128", dict(cb=128, cb2=128)),
    ("no_closed_loop", dict(mallat=False)),
    ("raw_magref", dict()),
])
def test_refusals_unsupported(env, why, kw):
    torch, orc, ctx = env
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    plan = _plan(ctx, "cb64", **dict(kw))
    try:
        if why == "raw_magref":
            ctx.check(ctx.L.j2k_plan_set_raw_magref(plan.h, 1))
        dev = plan.device
        n = max(int(plan.info.blocks), 1)
        pix = torch.zeros((70, 130 * 4), dtype=torch.uint8, device=dev)
        out = torch.full((1 << 16,), 0x77, dtype=torch.uint8, device=dev)
        back = torch.full((70, 130 * 4), 0x77, dtype=torch.uint8, device=dev)
        kept = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)
        rate = torch.zeros((n, 96), dtype=torch.int32, device=dev)
        dist = torch.zeros((n, 96), dtype=torch.int64, device=dev)
        nbs = torch.zeros(n, dtype=torch.uint8, device=dev)
        dec = torch.full((int(plan.info.decoded_elems) + 16,), 0x77, dtype=torch.int32, device=dev)
        offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        lens = torch.zeros(n, dtype=torch.int32, device=dev)
        calls = [
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, max_body_bytes=1000, pass_cuts=True),
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, max_distortion=5.0, pass_cuts=True),
            lambda: plan.decode_frame_pixels(out, 4096, back, pass_cuts=True),
            lambda: plan.rate_allocate(rate, dist, nbs, 10, kept=kept, pass_cuts=True),
            lambda: plan.rate_allocate_quality(rate, dist, nbs, [1.0], kept=kept, pass_cuts=True),
            lambda: plan.decode_blocks(out, offs, lens, nbs, decoded=dec, pfloors=kept),
            lambda: plan.decode_tile_parts(out, 4096, pfloors=kept),
            lambda: plan.encode_pixels_host(_lib.PIX_RGBA8, np.zeros((70, 130 * 4), np.uint8), max_body_bytes=1000, pass_cuts=True),
        ]
        if why not in ("no_closed_loop",):                            # (the stage encode of a plan without the closed loop has no coefficient layout to speak of)
            coeff = torch.zeros(int(plan.info.coeff_elems) + 16, dtype=torch.int32, device=dev)
            calls.append(lambda: plan.encode_blocks(coeff, slots=out if int(plan.info.bytes_cap) <= out.numel() else None, pass_cuts=True))
        for call in calls:
            with pytest.raises(J2KError) as e:
                call()
            assert e.value.status == _lib.ERR_UNSUPPORTED, why
        ctx.sync()
        for buf in (out, back, kept, dec):
            assert bool((buf == 0x77).all()), why                    # refused before any launch
    finally:
        plan.close()


def test_refusals_invalid_and_python(env):
    torch, orc, ctx = env
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    plan = _plan(ctx, "cb64")
    try:
        dev = plan.device
        n = int(plan.info.blocks)
        pix = torch.zeros((70, 130 * 4), dtype=torch.uint8, device=dev)
        hpix = np.zeros((70, 130 * 4), np.uint8)
        out = torch.full((1 << 16,), 0x77, dtype=torch.uint8, device=dev)
        kept = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)
        rate = torch.zeros((n, 96), dtype=torch.int32, device=dev)
        dist = torch.zeros((n, 96), dtype=torch.int64, device=dev)
        nbs = torch.zeros(n, dtype=torch.uint8, device=dev)
        for call in (
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, max_body_bytes=-1, pass_cuts=True),
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, max_distortion=-1.0, pass_cuts=True),
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, max_distortion=float("inf"), pass_cuts=True),
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, max_distortion=float("nan"), pass_cuts=True),
            lambda: plan.encode_pixels_host(_lib.PIX_RGBA8, hpix, max_body_bytes=-5, pass_cuts=True),
            lambda: plan.encode_pixels_host(_lib.PIX_RGBA8, hpix, max_distortion=float("nan"), pass_cuts=True),
            lambda: plan.rate_allocate(rate, dist, nbs, -1, kept=kept, pass_cuts=True),
            lambda: plan.rate_allocate_quality(rate, dist, nbs, [-0.5], kept=kept, pass_cuts=True),
            lambda: plan.rate_allocate_quality(rate, dist, nbs, [float("inf")], kept=kept, pass_cuts=True),
        ):
            with pytest.raises(J2KError) as e:
                call()
            assert e.value.status == _lib.ERR_INVALID_ARG
        for call in (
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, layer_bytes=[100, 200], pass_cuts=True),
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, layer_psnr=[30.0, 40.0], pass_cuts=True),
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, layer_distortion=[9.0, 4.0], pass_cuts=True),
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, max_body_bytes=100, roi=(0, 0, 8, 8), pass_cuts=True),
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, pass_cuts=True),
            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, max_body_bytes=100, min_psnr=30.0, pass_cuts=True),
            lambda: plan.encode_pixels_host(_lib.PIX_RGBA8, hpix, layer_bytes=[100], pass_cuts=True),
            lambda: plan.decode_frame_pixels(out, 4096, pix, layers=1, pass_cuts=True),
            lambda: plan.decode_pixels_host(b"\0" * 64, (70, 130 * 4), layers=1, pass_cuts=True),
            lambda: plan.encode_tile_parts(out, nbs, nbs, nbs, kept=kept, rate=rate, layers=2, pass_cuts=True),
            lambda: plan.rate_allocate_quality(rate, dist, nbs, [9.0, 4.0], pass_cuts=True),
            lambda: plan.encode_blocks(out, roi=(0, 0, 8, 8), pass_cuts=True),
        ):
            with pytest.raises(ValueError):
                call()
        ctx.sync()
        assert bool((out == 0x77).all()) and bool((kept == 0x77).all())
    finally:
        plan.close()


def test_capture_needs_one_call_before(env):
    """the frame calls' workspaces are made at their first call: a capture that meets them first is refused, as with the _rate calls"""
    torch, orc, ctx0 = env
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    ctx = _ctx_with()
    plan = _plan(ctx, "cb64")
    try:
        pix = torch.zeros((70, 130 * 4), dtype=torch.uint8, device=plan.device)
        out = torch.full((int(plan.frame_bound()),), 0x77, dtype=torch.uint8, device=plan.device)
        toffs = torch.zeros(int(plan.info.tiles) + 1, dtype=torch.int64, device=plan.device)
        torch.cuda.synchronize()
        with pytest.raises(J2KError) as e:
            with ctx.capture():
                plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, tile_offs=toffs, max_body_bytes=1000, pass_cuts=True)
        assert e.value.status == _lib.ERR_INVALID_ARG
        cs, _ = plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, tile_offs=toffs, max_body_bytes=1000, pass_cuts=True)      # usable afterwards
        plan.frame_status()
        ctx.sync()
        assert bool((out == 0x77).all())
    finally:
        plan.close()
        ctx.close()
