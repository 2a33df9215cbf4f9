"""GPU: the quality-scalable MQ decode (skip_planes = k: every block decoder stops after bit plane k, non-zero magnitudes take the midpoint of
what was left) against tests/coarse_cases.py.  Every expectation is the ORACLE's full decode (or, for frames, the oracle's forward
coefficients, which a lossless MQ loop hands back exactly) put through coarse(); no expectation is a device result.  Bit for bit.

Which test reaches which kernel:
  t1_decode64_kernel / t1_decode_kernel<LDSW> (t1_decode_block_wave)      test_one_launch_kernels (t1_dec_general 0 / 1)
  t1_dec_sig_lanes_kernel<true> (PERSIST), <false> + t1_dec_plane_kernel + t1_dec_magref_lanes_kernel<true>, t1_dec_step_kernel +
  t1_dec_magref_lanes_kernel<false>, t1_dec_assemble_kernel                  test_plane_stepped_forms (t1_dec_lanes 2 / 1 / 0), test_plan_path
  t1_decode_big_kernel<4,258> / <2,130>, the general kernel on 260 x 4     test_big_blocks
  the four C entries, both axes, refusals, batch / shard / graph            test_frames ... test_graph"""
import ctypes as C
import functools

import numpy as np
import pytest

import closed_loop_ref as ref
import coarse_cases as cc
import mallat_cases as mc

pytestmark = pytest.mark.gpu
CB = 64


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    from j2kgfx import Context
    ctx = Context(0)
    yield torch, orc, ctx
    ctx.close()


@functools.lru_cache(None)
def _family(name):
    """(blocks, the oracle's full decode of each): computed once, shared, never written"""
    import oracle as orc
    blocks = cc.FAMILIES[name][0](orc)
    full = [cc.full_decode(orc, b) for b in blocks]
    for f in full:
        f.setflags(write=False)
    return blocks, full


def _decode(blocks, ctx, k):
    from j2kgfx import entropy
    from j2kgfx.entropy import BLOCK_DTYPE
    bl = np.zeros(len(blocks), dtype=BLOCK_DTYPE)
    offs, pos = [], 0
    for i, b in enumerate(blocks):
        bl[i] = (0, b["band"], 0, 0, b["w"], b["h"])
        offs.append(pos)
        pos += b["data"].size
    stream = np.concatenate([b["data"] for b in blocks]) if pos else np.zeros(0, np.uint8)
    return entropy.decode_blocks(0, stream, np.array(offs, np.uint64), np.array([b["data"].size for b in blocks], np.uint32),
                                 np.array([b["nb"] for b in blocks], np.uint8), bl, ctx=ctx, skip_planes=k)


def _check(blocks, full, ctx, k, idx=None):
    idx = range(len(blocks)) if idx is None else idx
    got = _decode([blocks[i] for i in idx], ctx, k)
    for g, i in zip(got, idx):
        assert np.array_equal(g, cc.coarse(full[i], k)), (k, i, blocks[i]["w"], blocks[i]["h"], blocks[i]["nb"])


def _own_floors(name, blocks, full, ctx, offsets):
    """every block at the floors numBPS + offset of its own: one call per distinct numBPS"""
    for nb, idx in sorted(cc.by_numbps(blocks).items()):
        for o in offsets:
            if 0 <= nb + o <= 31:
                _check(blocks, full, ctx, nb + o, idx)


def _ctx_with(**opts):
    from j2kgfx import Context
    ctx = Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("k", cc.ONE_LAUNCH_KS + ("numBPS-1", "numBPS"))
def test_one_launch_kernels(k, general):
    blocks, full = _family("one_launch")
    ctx = _ctx_with(t1_dec_split=0, t1_dec_general=general)
    try:
        if isinstance(k, int):
            _check(blocks, full, ctx, k)
        else:
            _own_floors("one_launch", blocks, full, ctx, (-1,) if k == "numBPS-1" else (0,))
    finally:
        ctx.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [2, 1, 0])
@pytest.mark.parametrize("k", cc.STEPPED_KS)
def test_plane_stepped_forms(k, lanes):
    """one call: 100 small blocks on the plane-stepped form, three deep blocks on t1_decode64_kernel, one 128 x 128 block on the big kernel --
    each kernel applies the floor to its own blocks and leaves the others' output alone"""
    blocks, full = _family("stepped")
    ctx = _ctx_with(t1_dec_split=1, t1_dec_lanes=lanes)
    try:
        _check(blocks, full, ctx, k)
    finally:
        ctx.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", [("J2K_T1_BIG_DEC_CLASSES", "0"), ("J2K_T1_BIG_DEC_CLASSES", "1"), ("J2K_T1_BIG_DEC", "0")], ids=lambda p: "%s=%s" % p)
@pytest.mark.parametrize("k", cc.BIG_KS + ("numBPS-1",))
def test_big_blocks(env, monkeypatch, k, knob):
    torch, orc, ctx = env
    monkeypatch.setenv(*knob)
    blocks, full = _family("big")
    if isinstance(k, int):
        _check(blocks, full, ctx, k)
    else:
        _own_floors("big", blocks, full, ctx, (-1,))


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("case", cc.PLAN_CASES, ids=lambda c: "%dx%d" % c[:2])
def test_plan_path(env, case, split):
    """plan.decode_blocks(skip_planes=k): block by block against the oracle's decode of the same bytes, coarsened"""
    torch, orc, _ = env
    from j2kgfx.codec import FramePlan
    W, H, tile, cb, prec = case
    ctx = _ctx_with(t1_dec_split=split)
    plan = FramePlan(W, H, 3, ctx=ctx, precision=prec, lossless=True, num_resolutions=4, cb=cb, tile=tile, coder=0)
    try:
        coeff = plan.forward(torch.from_numpy(cc.plan_frame(W, H, prec)).to(plan.device))
        stream, offs, lens, nb = plan.encode_stream(coeff)
        ctx.sync()
        h_stream, h_offs, h_lens, h_nb = stream.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy(), nb.cpu().numpy()
        bl, doff = plan.blocks(), plan.decoded_offsets()
        full = [orc.t1_decode(h_stream[int(h_offs[j]):int(h_offs[j]) + int(h_lens[j])], int(h_nb[j]), int(b["band"]), int(b["w"]), int(b["h"]))
                for j, b in enumerate(bl)]
        assert int(h_nb[:len(bl)].max()) > 8
        assert (h_nb[:len(bl)] == 0).any() or cb != (32, 32)       # the flat area: blocks without planes (64 x 16 blocks all reach past it)
        for k in cc.PLAN_KS:
            dec = torch.full((int(plan.info.decoded_elems),), -7, dtype=torch.int32, device=plan.device)
            plan.decode_blocks(stream, offs, lens, nb, decoded=dec, skip_planes=k)
            ctx.sync()
            h = dec.cpu().numpy()
            for j, b in enumerate(bl):
                n = int(b["w"]) * int(b["h"])
                assert np.array_equal(h[int(doff[j]):int(doff[j]) + n], cc.coarse(full[j], k).reshape(-1)), (k, j)
    finally:
        plan.close()
        ctx.close()


# ---- 5 - 9, frames ----------------------------------------------------------------------------------------------------------------------
def _plan(ctx, W, H, Cn, prec, tile, nres, **kw):
    from j2kgfx.codec import FramePlan
    kw.setdefault("mallat", True)
    return FramePlan(W, H, Cn, precision=prec, lossless=kw.pop("lossless", True), quality=kw.pop("quality", 0), num_resolutions=nres, cb=(CB, CB), tile=tile,
                     coder=kw.pop("coder", 0), ctx=ctx, **kw)


def _dev(torch, plan, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(plan.device)


@functools.lru_cache(None)
def _frame(case, seed, lossless=True, quality=0):
    """(pix, planes, forward coefficient tiles by the oracle) of a frame case"""
    import oracle as orc
    W, H, Cn, prec, tile, nres = case[:6]
    pix, Cn2, prec2, planes = ref.pixel_frame(mc.PIX_FORMAT[(Cn, prec)], W, H, seed, orc, noise=(1 << prec) // 16)
    assert (Cn2, prec2) == (Cn, prec)
    return pix, planes, mc.forward_frame(orc, planes, tile, prec, nres, lossless, quality)


def _expect(orc, case, tiles, r, k, **kw):
    W, H, Cn, prec, tile, nres = case[:6]
    return mc.pixels(orc, mc.inverse_frame(orc, cc.coarse_tiles(tiles, k), W, H, tile, prec, nres, reduce=r, **kw), prec)


def _encode(torch, plan, case, pix, marks):
    W, H, Cn, prec = case[:4]
    cs, toffs = plan.encode_frame_pixels(mc.PIX_FORMAT[(Cn, prec)], _dev(torch, plan, pix), sop=marks, eph=marks)
    plan.frame_status()
    return cs, toffs, int(toffs[-1].item())


@pytest.mark.parametrize("marks", [False, True], ids=["bare", "sop_eph"])
@pytest.mark.parametrize("case", cc.FRAME_CASES, ids=mc.case_id)
def test_frames(env, case, marks):
    torch, orc, ctx = env
    W, H, Cn, prec, tile, nres = case
    pix, planes, tiles = _frame(case, 81)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres)
    try:
        cs, toffs, total = _encode(torch, plan, case, pix, marks)
        for r in cc.FRAME_REDUCES:
            assert r in mc.admissible(W, H, tile, nres)
            for k in cc.FRAME_KS:
                exp = _expect(orc, case, tiles, r, k)
                back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
                plan.decode_frame_pixels(cs, total, back, tile_offs=toffs if k == 3 else None, sop=marks, eph=marks, reduce=r, skip_planes=k)
                plan.frame_status()
                assert np.array_equal(back.cpu().numpy(), exp), (r, k)
                if k == 12 and prec == 8:              # every coefficient of an 8-bit frame is below 2^12: the flat mid-gray frame
                    px = exp.reshape(exp.shape[0], -1, 4)
                    assert (px[..., :3] == 128).all() and (px[..., 3] == 255).all()
                if k == 0 and r == 0 and prec == 8:
                    assert np.array_equal(exp, pix)
    finally:
        plan.close()


def test_frame_prefix_layout(env):
    """a closed_loop=True plan (the reference's prefix layout) at reduce = 0: the oracle's own multi-level inverse of the coarsened planes"""
    torch, orc, ctx = env
    case = cc.FRAME_CASES[1]
    W, H, Cn, prec, tile, nres = case
    pix, planes, _ = _frame(case, 81)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres, mallat=False, closed_loop=True)
    try:
        cs, toffs, total = _encode(torch, plan, case, pix, True)
        for k in (1, 3):
            frm = np.zeros((Cn, H, W), np.int32)
            for x0, y0, w, h in mc.tiles_of(W, H, tile):
                sub = [np.ascontiguousarray(planes[c, y0:y0 + h, x0:x0 + w]).astype(np.int32) for c in range(Cn)]
                coeff = orc.preprocess(sub, w, h, prec, True, nres, 0)
                rec = [orc.reconstruct53(cc.coarse(np.asarray(coeff[c]).reshape(h, w), k), w, h, nres - 1) for c in range(Cn)]
                px = orc.postprocess(rec, prec, True)
                for c in range(Cn):
                    frm[c, y0:y0 + h, x0:x0 + w] = np.asarray(px[c]).reshape(h, w)
            exp = mc.pixels(orc, frm, prec)
            back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, sop=True, eph=True, skip_planes=k)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), k
    finally:
        plan.close()


def test_frame_lossy_dequantize(env):
    """mallat_cases.LOSSY[0] with the dequantiser on at k = 2: the quantised coefficients coarsened, then the oracle's dequantising inverse"""
    torch, orc, ctx = env
    case = mc.LOSSY[0]
    W, H, Cn, prec, tile, nres, q = case
    pix, planes, tiles = _frame(case, 83, False, q)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres, lossless=False, quality=q, dequantize=True)
    try:
        cs, toffs, total = _encode(torch, plan, case, pix, True)
        for r in (0, 1):
            exp = _expect(orc, case, tiles, r, 2, lossless=False, quality=q, dequantize=True)
            back = torch.zeros(exp.shape, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=True, eph=True, reduce=r, skip_planes=2)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), r
    finally:
        plan.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,r,k,marks", [(cc.FRAME_CASES[0], 1, 3, False), (cc.FRAME_CASES[1], 2, 1, True), (cc.FRAME_CASES[2], 0, 3, True)],
                         ids=["130x70-r1-k3", "260x44-r2-k1", "gray16-r0-k3"])
def test_host_one_call_form(env, case, r, k, marks):
    torch, orc, ctx = env
    W, H, Cn, prec, tile, nres = case
    pix, planes, tiles = _frame(case, 81)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres)
    try:
        cs, toffs, total = _encode(torch, plan, case, pix, marks)
        exp = _expect(orc, case, tiles, r, k)
        back = torch.zeros(exp.shape, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, total, back, sop=marks, eph=marks, reduce=r, skip_planes=k)
        plan.frame_status()
        host = plan.decode_pixels_host(cs[:total].cpu().numpy(), exp.shape, sop=marks, eph=marks, reduce=r, skip_planes=k)
        assert np.array_equal(host, back.cpu().numpy()) and np.array_equal(host, exp)
    finally:
        plan.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------
def test_skip_planes_zero_is_the_old_call(env):
    """each of the four new entries with skip_planes = 0 (asked for by name: the keyword's default takes the old entry) against the entry it extends"""
    torch, orc, ctx = env
    from j2kgfx import entropy
    from j2kgfx.entropy import BLOCK_DTYPE
    L = ctx.L
    # j2k_decode_blocks_coarse
    blocks, full = _family("one_launch")
    sub = blocks[:14]
    old = _decode(sub, ctx, 0)
    bl = np.zeros(len(sub), dtype=BLOCK_DTYPE)
    for i, b in enumerate(sub):
        bl[i] = (0, b["band"], 0, 0, b["w"], b["h"])
    lens = np.array([b["data"].size for b in sub], np.uint32)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
    stream = np.concatenate([b["data"] for b in sub])
    nb = np.array([b["nb"] for b in sub], np.uint8)
    sizes = np.array([b["w"] * b["h"] for b in sub], np.int64)
    coff = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64)
    out = np.full(int(sizes.sum()), -7, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
    ctx.check(L.j2k_decode_blocks_coarse(ctx.h, 0, P(stream), P(offs), P(lens), P(nb), P(bl), C.c_size_t(len(sub)), 0, P(out), P(coff)))
    assert np.array_equal(out, np.concatenate([o.reshape(-1) for o in old]))
    # the plan entries
    case = cc.FRAME_CASES[1]
    W, H, Cn, prec, tile, nres = case
    pix, planes, tiles = _frame(case, 81)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres)
    try:
        cs, toffs, total = _encode(torch, plan, case, pix, True)
        o2, l2, n2 = plan.decode_tile_parts(cs, total, sop=True, eph=True)
        plan.frame_status()
        a = torch.full((int(plan.info.decoded_elems),), -7, dtype=torch.int32, device=plan.device)
        b = a.clone()
        plan.decode_blocks(cs, o2, l2, n2, decoded=a)
        ctx.check(L.j2k_plan_decode_blocks_coarse(plan.h, plan._p(cs), plan._p(o2), plan._p(l2), plan._p(n2), 0, plan._p(b)))
        ctx.sync()
        assert torch.equal(a, b)
        for r in (0, 1):
            Hr, Wr = plan.reduced_shape(r)
            x = torch.full((Hr, Wr * 4 + 8), 0x5A, dtype=torch.uint8, device=plan.device)
            y = x.clone()
            plan.decode_frame_pixels(cs, total, x, sop=True, eph=True, reduce=r)
            ctx.check(L.j2k_plan_decode_frame_pixels_coarse(plan.h, plan._p(cs), C.c_size_t(total), None, 1, 1, r, 0, plan._p(y), C.c_size_t(int(y.shape[1]))))
            plan.frame_status()
            assert torch.equal(x, y) and not bool((x[:, :Wr * 4] == 0x5A).all())
            h_cs = cs[:total].cpu().numpy()
            hx = plan.decode_pixels_host(h_cs, (Hr, Wr * 4 + 8), sop=True, eph=True, reduce=r)
            hy = np.zeros((Hr, Wr * 4 + 8), np.uint8)
            ctx.check(L.j2k_decode_pixels_host_coarse(plan.h, P(h_cs), C.c_size_t(h_cs.size), 1, 1, r, 0, P(hy), C.c_size_t(Wr * 4 + 8)))
            assert np.array_equal(hx, hy)
    finally:
        plan.close()


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    torch, orc, ctx = env
    from j2kgfx import J2KError, _lib

    def status(fn):
        try:
            fn()
        except J2KError as e:
            assert str(e)
            return e.status
        return _lib.OK
    case = cc.FRAME_CASES[1]
    W, H, Cn, prec, tile, nres = case
    pix, planes, tiles = _frame(case, 81)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres)
    ht = _plan(ctx, W, H, Cn, prec, tile, nres, coder=1)
    plain = _plan(ctx, W, H, Cn, prec, tile, nres, mallat=False, closed_loop=True)
    try:
        cs, toffs, total = _encode(torch, plan, case, pix, False)
        hcs, htoffs, htotal = _encode(torch, ht, case, pix, False)
        h_cs = cs[:total].cpu().numpy()
        sentinel = torch.full((H, W * 4), 0x5A, dtype=torch.uint8, device=plan.device)
        blocks, full = _family("one_launch")
        for bad in (-1, 32):
            assert status(lambda: plan.decode_frame_pixels(cs, total, sentinel, skip_planes=bad)) == _lib.ERR_INVALID_ARG
            assert status(lambda: plan.decode_frame_pixels(cs, total, sentinel, reduce=1, skip_planes=bad)) == _lib.ERR_INVALID_ARG
            assert status(lambda: plan.decode_pixels_host(h_cs, (H, W * 4), skip_planes=bad)) == _lib.ERR_INVALID_ARG
            assert status(lambda: _decode(blocks[:2], ctx, bad)) == _lib.ERR_INVALID_ARG
            o2, l2, n2 = plan.decode_tile_parts(cs, total)
            assert status(lambda: plan.decode_blocks(cs, o2, l2, n2, skip_planes=bad)) == _lib.ERR_INVALID_ARG
        # the HT coder has no planes to stop between
        assert status(lambda: ht.decode_frame_pixels(hcs, htotal, sentinel, skip_planes=1)) == _lib.ERR_UNSUPPORTED
        assert status(lambda: ht.decode_frame_pixels(hcs, htotal, sentinel, reduce=1, skip_planes=1)) == _lib.ERR_UNSUPPORTED
        assert status(lambda: ht.decode_pixels_host(hcs[:htotal].cpu().numpy(), (H, W * 4), skip_planes=1)) == _lib.ERR_UNSUPPORTED
        o3, l3, n3 = ht.decode_tile_parts(hcs, htotal)
        assert status(lambda: ht.decode_blocks(hcs, o3, l3, n3, skip_planes=1)) == _lib.ERR_UNSUPPORTED
        assert status(lambda: _decode_ht_one(ctx, 1)) == _lib.ERR_UNSUPPORTED
        # reduce on a plan that is not a Mallat plan: refused as before, whatever the floor
        assert status(lambda: plain.decode_frame_pixels(cs, total, sentinel, reduce=1, skip_planes=2)) == _lib.ERR_UNSUPPORTED
        assert status(lambda: plain.decode_pixels_host(h_cs, (H, W * 4), reduce=1, skip_planes=2)) == _lib.ERR_UNSUPPORTED
        assert status(lambda: plan.decode_frame_pixels(cs, total, sentinel, reduce=-1, skip_planes=2)) == _lib.ERR_INVALID_ARG
        assert status(lambda: plan.decode_frame_pixels(cs, total, sentinel, reduce=mc.levels_of(nres) + 1, skip_planes=2)) == _lib.ERR_INVALID_ARG
        plan.ctx.sync()
        assert bool((sentinel == 0x5A).all())
        # a stream the decoder refuses leaves d_pix untouched at a floor too
        def truncated():
            plan.decode_frame_pixels(cs, total // 2, sentinel, skip_planes=2)
            plan.frame_status()
        assert status(truncated) == _lib.ERR_INVALID_ARG
        assert bool((sentinel == 0x5A).all())
        # HT with k = 0: the old result
        x, y = torch.zeros_like(sentinel), torch.zeros_like(sentinel)
        ht.decode_frame_pixels(hcs, htotal, x)
        ctx.check(ctx.L.j2k_plan_decode_frame_pixels_coarse(ht.h, ht._p(hcs), C.c_size_t(htotal), None, 0, 0, 0, 0, ht._p(y), C.c_size_t(W * 4)))
        ht.frame_status()
        assert torch.equal(x, y) and bool(x.any())
    finally:
        plan.close()
        ht.close()
        plain.close()


def _decode_ht_one(ctx, k):
    from j2kgfx import entropy
    from j2kgfx.entropy import BLOCK_DTYPE
    bl = np.zeros(1, dtype=BLOCK_DTYPE)
    bl[0] = (0, 0, 0, 0, 8, 8)
    return entropy.decode_blocks(1, np.zeros(4, np.uint8), np.zeros(1, np.uint64), np.array([4], np.uint32), np.array([3], np.uint8), bl, ctx=ctx, skip_planes=k)


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------------
def test_batch(env):
    """two frames of 260 x 44, frame_rows = 44"""
    torch, orc, ctx = env
    case = cc.FRAME_CASES[1]
    W, H, Cn, prec, tile, nres = case
    frames = [_frame(case, 81 + b) for b in range(2)]
    pix = np.concatenate([f[0] for f in frames])
    plan = _plan(ctx, W, 2 * H, Cn, prec, tile, nres, frame_rows=H)
    try:
        cs, toffs, total = _encode(torch, plan, case, pix, True)
        tiles = cc.coarse_tiles(frames[0][2] + frames[1][2], 3)
        for r in (0, 2):
            exp = mc.pixels(orc, mc.inverse_frame(orc, tiles, W, 2 * H, tile, prec, nres, reduce=r, frame_rows=H), prec)
            back = torch.zeros(exp.shape, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=True, eph=True, reduce=r, skip_planes=3)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), r
    finally:
        plan.close()


def test_shard(env):
    """tiles 1 and 2 of the 260 x 44 frame into a sentinel frame: only the shard's tiles are written"""
    torch, orc, ctx = env
    case = cc.FRAME_CASES[1]
    W, H, Cn, prec, tile, nres = case
    pix, planes, tiles = _frame(case, 81)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres, tile_first=1, tile_count=2)
    try:
        cs, toffs, total = _encode(torch, plan, case, pix, False)
        for r, k in ((1, 2), (0, 3)):
            full = _expect(orc, case, tiles, r, k)
            exp = np.full_like(full, 0x5A)
            for t, (x, y, w, h) in enumerate(mc.reduced_rects(W, H, tile, r)):
                if t in (1, 2):
                    exp[y:y + h, 4 * x:4 * (x + w)] = full[y:y + h, 4 * x:4 * (x + w)]
            back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, reduce=r, skip_planes=k)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), (r, k)
    finally:
        plan.close()


def test_graph(env):
    """decode_frame_pixels(reduce=1, skip_planes=2) captured after one warm call, replayed on a second stream of the same geometry"""
    torch, orc, _ = env
    from j2kgfx import Context
    case = cc.FRAME_CASES[1]
    W, H, Cn, prec, tile, nres = case
    ctx = Context(0)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres)
    try:
        streams, exps = [], []
        for seed in (81, 82):
            pix, planes, tiles = _frame(case, seed)
            cs, toffs, total = _encode(torch, plan, case, pix, True)
            streams.append((cs.clone(), toffs.clone()))
            exps.append(_expect(orc, case, tiles, 1, 2))
        assert not np.array_equal(exps[0], exps[1])
        cs, toffs = streams[0][0].clone(), streams[0][1].clone()
        back = torch.zeros(exps[0].shape, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, int(cs.numel()), back, tile_offs=toffs, sop=True, eph=True, reduce=1, skip_planes=2)      # warm: makes the tables of reduce 1
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exps[0])
        with ctx.capture() as g:
            plan.decode_frame_pixels(cs, int(cs.numel()), back, tile_offs=toffs, sop=True, eph=True, reduce=1, skip_planes=2)
        for i in (1, 0, 1):
            cs.copy_(streams[i][0])
            toffs.copy_(streams[i][1])
            back.zero_()
            torch.cuda.synchronize()
            g.launch()
            ctx.sync()
            assert np.array_equal(back.cpu().numpy(), exps[i]), i
        g.close()
    finally:
        plan.close()
        ctx.close()
