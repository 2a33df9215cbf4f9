"""GPU: Mallat plans (FramePlan(mallat=True), j2k_params.closed_loop = J2K_CLOSED_LOOP_MALLAT) and their reduced-resolution decode against the
expectation of tests/mallat_cases.py (checked on the CPU by tests/test_mallat_ref.py).  Every comparison is bit for bit (np.array_equal).

The shapes are the smallest at which the routing of the general kernels' Mallat instantiation can go wrong -- a strip is 63 lanes of 2 / 4 / 8
columns (lossless53_cases.STRIP_BASES), a band is band_prows (5-3) / band_prows_97 (9-7) pair-rows (lossless53_cases.defaults()); see
mallat_cases.LOSSLESS for what each case reaches.  Which test reaches which site of the product:

  dwt53_fwd_kernel<.., MAL> fwd_store_row / dwt53_inv_kernel<.., MAL> inv_load_row       test_lossless_forward_and_inverse, test_lossless_arbitrary_coefficients
    vector path (256 x 12, 520 x 10, the 64 x 64 tiles), scalar fallback (258 x 10, 130 x 70, 5 x 3), thin levels (5 x 3)
  dwt97_fwd_kernel<.., MAL> / dwt97_inv_kernel<.., DEQ, MAL>                               test_lossy
  plan_reduced: the final launch of level r, mallat_ll_kernel (r = L), the reduced pack   test_lossless_reduced, test_lossy, test_pixel_formats
  select_blocks_kernel, the block decoders on a subset, j2k_plan_decode_frame_pixels_reduced / j2k_decode_pixels_host_reduced
                                                                                           test_closed_loop, test_decode_skips_the_top_resolution, test_batch, test_shard, test_graph
  the refusals                                                                             test_refusals"""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import closed_loop_ref as ref
import lossless53_cases as ll
import lossy97_cases as lc
import mallat_cases as mc

pytestmark = pytest.mark.gpu
CB = 64
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    import t2ref
    from j2kgfx import Context
    ctx = Context(0)
    yield torch, orc, t2ref, ctx
    ctx.close()


def _plan(ctx, W, H, Cn, prec, tile, nres, lossless=True, quality=0, coder=0, **kw):
    from j2kgfx.codec import FramePlan
    return FramePlan(W, H, Cn, precision=prec, lossless=lossless, quality=quality, num_resolutions=nres, cb=(CB, CB), tile=tile, coder=coder, ctx=ctx,
                     mallat=True, **kw)


def _dev(torch, plan, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(plan.device)


def _bpp(Cn, prec):
    return (1 if Cn == 1 else 4) * (2 if prec > 8 else 1)


@functools.lru_cache(None)
def _lossless_expectation(case, family):
    import oracle as orc
    W, H, Cn, prec, tile, nres = case
    frm = mc.lossless_frame(case, family)
    return frm, mc.forward_frame(orc, frm, tile, prec, nres)


def _check_reduced(torch, orc, plan, d_coeff, tiles, W, H, Cn, prec, tile, nres, lossless=True, quality=0, dequantize=False, pix=True):
    """inverse(reduce=r) and inverse_pixels(reduce=r) for every admissible r against the expectation; r = 0 against the existing calls"""
    rs = mc.admissible(W, H, tile, nres)
    assert rs[0] == 0
    for r in rs:
        want = mc.inverse_frame(orc, tiles, W, H, tile, prec, nres, lossless, quality, dequantize, r)
        assert plan.reduced_shape(r) == want.shape[1:]
        frame = torch.full((Cn,) + want.shape[1:], -77, dtype=torch.int32, device=plan.device)
        if r == 0:      # (the keyword's default is the existing call: ask for the reduced entry point by name)
            plan.ctx.check(plan.ctx.L.j2k_plan_inverse_reduced(plan.h, plan._p(d_coeff), 0, plan._p(frame)))
            same = plan.inverse(d_coeff)
            plan.ctx.sync()
            assert torch.equal(frame, same)
        else:
            plan.inverse(d_coeff, frame, reduce=r)
            plan.ctx.sync()
        assert np.array_equal(frame.cpu().numpy(), want), r
        if not pix or (Cn, prec) not in mc.PIX_FORMAT:
            continue
        Hr, Wr = want.shape[1:]
        stride = Wr * _bpp(Cn, prec) + 8
        out = torch.full((Hr, stride), 0x5A, dtype=torch.uint8, device=plan.device)
        assert not plan.pixels_fused(mc.PIX_FORMAT[(Cn, prec)], out, inverse=True)          # a Mallat plan stages its pixels
        if r == 0:
            plan.ctx.check(plan.ctx.L.j2k_plan_inverse_pixels_reduced(plan.h, plan._p(d_coeff), 0, plan._p(out), C.c_size_t(int(out.shape[1]))))
            same = plan.inverse_pixels(d_coeff, torch.full_like(out, 0x5A))
            plan.ctx.sync()
            assert torch.equal(out, same)
        else:
            plan.inverse_pixels(d_coeff, out, reduce=r)
            plan.ctx.sync()
        want_pix = np.full((Hr, stride), 0x5A, np.uint8)
        want_pix[:, :stride - 8] = mc.pixels(orc, want, prec)
        assert np.array_equal(out.cpu().numpy(), want_pix), r


# ---- 1 - 3, lossless ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["noise", "impulse"])
@pytest.mark.parametrize("case", mc.LOSSLESS, ids=mc.case_id)
def test_lossless_forward_and_inverse(env, case, family):
    torch, orc, t2ref, ctx = env
    W, H, Cn, prec, tile, nres = case
    frm, tiles = _lossless_expectation(case, family)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres)
    try:
        want = mc.flat_coeff(plan.planes(), tiles, int(plan.info.coeff_elems))
        coeff = plan.forward(_dev(torch, plan, frm), plan.alloc_coeff().zero_())        # (zeroed: the planes' padding to four elements is nobody's)
        plan.ctx.sync()
        got = coeff.cpu().numpy()[:want.size]
        assert np.array_equal(got, want)
        if mc.levels_of(nres) >= 2:          # the contrast: not the prefix layout
            prefix = mc.flat_coeff(plan.planes(), mc.forward_frame(orc, frm, tile, prec, nres, prefix=True), want.size)
            assert not np.array_equal(got, prefix)
        back = plan.inverse(coeff)
        plan.ctx.sync()
        assert np.array_equal(back.cpu().numpy(), frm)
    finally:
        plan.close()


@pytest.mark.parametrize("case", mc.LOSSLESS, ids=mc.case_id)
def test_lossless_reduced(env, case):
    torch, orc, t2ref, ctx = env
    W, H, Cn, prec, tile, nres = case
    frm, tiles = _lossless_expectation(case, "noise")
    plan = _plan(ctx, W, H, Cn, prec, tile, nres)
    try:
        d_coeff = _dev(torch, plan, mc.flat_coeff(plan.planes(), tiles, max(int(plan.info.coeff_elems), 4)))
        _check_reduced(torch, orc, plan, d_coeff, tiles, W, H, Cn, prec, tile, nres)
    finally:
        plan.close()


@pytest.mark.parametrize("family", ["noise", "fullrange"])
@pytest.mark.parametrize("case", mc.LOSSLESS, ids=mc.case_id)
def test_lossless_arbitrary_coefficients(env, case, family):
    """coefficient sets no forward transform produced, int32 wrap-around included: the full inverse and every reduced one"""
    torch, orc, t2ref, ctx = env
    W, H, Cn, prec, tile, nres = case
    plan = _plan(ctx, W, H, Cn, prec, tile, nres)
    try:
        tiles = [np.stack([ll.coeff_plane(family, w, h, 5 * t + c) for c in range(Cn)]) for t, (x0, y0, w, h) in enumerate(mc.tiles_of(W, H, tile))]
        d_coeff = _dev(torch, plan, mc.flat_coeff(plan.planes(), tiles, max(int(plan.info.coeff_elems), 4)))
        _check_reduced(torch, orc, plan, d_coeff, tiles, W, H, Cn, prec, tile, nres, pix=family == "noise")
    finally:
        plan.close()


@pytest.mark.parametrize("Cn,prec,name", [(1, 8, "gray8"), (1, 16, "gray16"), (3, 8, "rgba8"), (3, 16, "rgba64"), (4, 8, "nrgba8")])
def test_pixel_formats(env, Cn, prec, name):
    """the reduced pack in every format decoder.createImage writes, on 130 x 70 (reduce 1 leaves 0 ... 2^p - 1: the clamp) and the tiled 260 x 44"""
    torch, orc, t2ref, ctx = env
    for W, H, tile, nres in ((130, 70, (0, 0), 4), (260, 44, (128, 32), 4)):
        frm = ref.frame_n(W, H, Cn, prec, 17 + Cn)
        if Cn == 3 and prec == 8:
            frm = ref.frame(W, H, 3, 16).astype(np.int32)
        tiles = mc.forward_frame(orc, frm, tile, prec, nres)
        plan = _plan(ctx, W, H, Cn, prec, tile, nres)
        try:
            d_coeff = _dev(torch, plan, mc.flat_coeff(plan.planes(), tiles, int(plan.info.coeff_elems)))
            _check_reduced(torch, orc, plan, d_coeff, tiles, W, H, Cn, prec, tile, nres)
        finally:
            plan.close()


# ---- 1 - 3, lossy ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dequantize", [False, True])
@pytest.mark.parametrize("case", mc.LOSSY, ids=mc.case_id)
def test_lossy(env, case, dequantize):
    torch, orc, t2ref, ctx = env
    W, H, Cn, prec, tile, nres, q = case
    frm = ref.frame_n(W, H, Cn, prec, 23)
    tiles = mc.forward_frame(orc, frm, tile, prec, nres, False, q)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres, lossless=False, quality=q, dequantize=dequantize)
    try:
        want = mc.flat_coeff(plan.planes(), tiles, int(plan.info.coeff_elems))
        coeff = plan.forward(_dev(torch, plan, frm), plan.alloc_coeff().zero_())
        plan.ctx.sync()
        got = coeff.cpu().numpy()[:want.size]
        assert np.array_equal(got, want)
        prefix = mc.flat_coeff(plan.planes(), mc.forward_frame(orc, frm, tile, prec, nres, False, q, prefix=True), want.size)
        assert not np.array_equal(got, prefix)
        _check_reduced(torch, orc, plan, coeff, tiles, W, H, Cn, prec, tile, nres, False, q, dequantize)
        # ... and coefficients no forward transform produced
        band = (lc.defaults()["band_prows_97"],)
        tiles2 = [np.stack([lc.coeff_plane("noise", w, h, 7 * t + c, band) for c in range(Cn)]) for t, (x0, y0, w, h) in enumerate(mc.tiles_of(W, H, tile))]
        d2 = _dev(torch, plan, mc.flat_coeff(plan.planes(), tiles2, int(plan.info.coeff_elems)))
        _check_reduced(torch, orc, plan, d2, tiles2, W, H, Cn, prec, tile, nres, False, q, dequantize, pix=False)
    finally:
        plan.close()


# ---- 4, the closed loop ----------------------------------------------------------------------------------------------------------------------
def _closed_loop_frame(orc, case, seed):
    from j2kgfx import _lib  # noqa: F401
    W, H, Cn, prec, tile, nres = case[:6]
    pix, Cn2, prec2, planes = ref.pixel_frame(mc.PIX_FORMAT[(Cn, prec)], W, H, seed, orc, noise=(1 << prec) // 16)
    assert (Cn2, prec2) == (Cn, prec)
    return pix, planes


def _decode_expectation(orc, want, W, H, Cn, prec, tile, nres, coder, r, **kw):
    tiles = mc.decoded_tiles(orc, want, Cn, nres, CB, coder)
    return mc.pixels(orc, mc.inverse_frame(orc, tiles, W, H, tile, prec, nres, reduce=r, **kw), prec)


@pytest.mark.parametrize("marks", [False, True], ids=["bare", "sop_eph"])
@pytest.mark.parametrize("coder", [0, 1], ids=["mq", "ht"])
@pytest.mark.parametrize("case", mc.LOSSLESS, ids=mc.case_id)
def test_closed_loop(env, case, coder, marks):
    torch, orc, t2ref, ctx = env
    W, H, Cn, prec, tile, nres = case
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    pix, planes = _closed_loop_frame(orc, case, 31 + coder)
    want = mc.oracle_frame(planes, W, H, tile[0], tile[1], nres, CB, coder, marks, marks, orc, t2ref, precision=prec)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres, coder=coder)
    try:
        d_pix = _dev(torch, plan, pix)
        cs, toffs = plan.encode_frame_pixels(fmt, d_pix, sop=marks, eph=marks)
        plan.frame_status()
        h_cs, h_toffs = cs.cpu().numpy(), toffs.cpu().numpy()
        for i, t in enumerate(sorted(want)):
            assert bytes(h_cs[int(h_toffs[i]):int(h_toffs[i + 1])]) == want[t]["part"], t
        total = int(h_toffs[-1])
        if coder == 0:
            assert np.array_equal(np.stack(mc.decoded_tiles(orc, want, Cn, nres, CB, 0)[0]), np.stack(want[0]["coeff"]))
        # the stage calls agree with the one-call forms
        coeff = plan.forward(_dev(torch, plan, planes.astype(np.int32)))
        stream, offs, lens, numbps = plan.encode_stream(coeff)
        cs2, toffs2 = plan.encode_tile_parts(stream, offs, lens, numbps, sop=marks, eph=marks)
        plan.frame_status()
        assert int(toffs2[-1].item()) == total and torch.equal(cs2[:total], cs[:total])
        o2, l2, n2 = plan.decode_tile_parts(cs2, total, tile_offs=None, sop=marks, eph=marks)
        staged = plan.inverse(plan.place_blocks(plan.decode_blocks(cs2, o2, l2, n2), torch.zeros_like(coeff)))
        plan.frame_status()
        stage_pix = mc.pixels(orc, staged.cpu().numpy(), prec)
        for r in mc.admissible(W, H, tile, nres):
            exp = _decode_expectation(orc, want, W, H, Cn, prec, tile, nres, coder, r)
            back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
            if r == 0:
                plan.ctx.check(plan.ctx.L.j2k_plan_decode_frame_pixels_reduced(plan.h, plan._p(cs), C.c_size_t(total), None, int(marks), int(marks), 0, plan._p(back),
                                                                               C.c_size_t(int(back.shape[1]))))
            else:
                plan.decode_frame_pixels(cs, total, back, tile_offs=None, sop=marks, eph=marks, reduce=r)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), r
            host = plan.decode_pixels_host(h_cs[:total], exp.shape, sop=marks, eph=marks, reduce=r)
            assert np.array_equal(host, exp), r
            if r == 0:
                assert np.array_equal(exp, stage_pix)
                same = torch.zeros_like(back)
                plan.decode_frame_pixels(cs, total, same, tile_offs=toffs, sop=marks, eph=marks)
                plan.frame_status()
                assert torch.equal(same, back)
                if coder == 0 and prec == 8:                 # the MQ loop is lossless (16 bit: createImage's own rescale wraps, decoder.go:434-451)
                    assert np.array_equal(exp, pix)
    finally:
        plan.close()


@pytest.mark.parametrize("case", mc.LOSSY, ids=mc.case_id)
def test_closed_loop_lossy(env, case):
    """the lossy cases with the dequantiser on: tile-parts by the oracle's composition, every reduced decode"""
    torch, orc, t2ref, ctx = env
    W, H, Cn, prec, tile, nres, q = case
    pix, planes = _closed_loop_frame(orc, case, 37)
    want = mc.oracle_frame(planes, W, H, tile[0], tile[1], nres, CB, 0, True, True, orc, t2ref, precision=prec, lossless=False, quality=q)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres, lossless=False, quality=q, dequantize=True)
    try:
        cs, toffs = plan.encode_frame_pixels(mc.PIX_FORMAT[(Cn, prec)], _dev(torch, plan, pix), sop=True, eph=True)
        plan.frame_status()
        total = int(toffs[-1].item())
        assert bytes(cs[:total].cpu().numpy()) == b"".join(want[t]["part"] for t in sorted(want))
        for r in mc.admissible(W, H, tile, nres):
            exp = _decode_expectation(orc, want, W, H, Cn, prec, tile, nres, 0, r, lossless=False, quality=q, dequantize=True)
            back = torch.zeros(exp.shape, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=True, eph=True, reduce=r)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), r
    finally:
        plan.close()


GOLDEN = json.load(open(os.path.join(HERE, "golden", mc.GOLDEN_FILE)))


@pytest.mark.parametrize("case", mc.GOLDEN_CASES, ids=[c["name"] for c in mc.GOLDEN_CASES])
def test_product_writes_the_pinned_tile_parts(env, case):
    torch, orc, t2ref, ctx = env
    from j2kgfx import _lib
    W, H = case["W"], case["H"]
    frm = ref.frame(W, H, case["seed"], noise=case["noise"])
    pix = np.full((H, W, 4), 255, np.uint8)
    pix[..., :3] = frm.transpose(1, 2, 0)
    plan = _plan(ctx, W, H, 3, 8, case["tile"], case["nres"], coder=case["coder"])
    try:
        cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA8, _dev(torch, plan, pix.reshape(H, W * 4)), sop=case["sop"], eph=case["eph"])
        plan.frame_status()
        total = int(toffs[-1].item())
        g = GOLDEN[case["name"]]
        assert total == g["bytes"] and hashlib.sha256(cs[:total].cpu().numpy().tobytes()).hexdigest() == g["sha256"]
    finally:
        plan.close()


# ---- 5, the decode skips what it may skip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", [0, 1], ids=["mq", "ht"])
def test_decode_skips_the_top_resolution(env, coder):
    """the plan owns its coefficient planes and decoded-block buffer, so: damage the body of one code-block of the top resolution in the
    stream.  reduce = 1 never decodes it -- same pixels, status J2K_OK; reduce = 0 does, and differs."""
    torch, orc, t2ref, ctx = env
    case = mc.LOSSLESS[0]
    W, H, Cn, prec, tile, nres = case
    pix, planes = _closed_loop_frame(orc, case, 41)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres, coder=coder)
    try:
        cs, toffs = plan.encode_frame_pixels(mc.PIX_FORMAT[(Cn, prec)], _dev(torch, plan, pix))
        plan.frame_status()
        total = int(toffs[-1].item())
        o2, l2, n2 = plan.decode_tile_parts(cs, total)
        plan.frame_status()
        offs, lens = o2.cpu().numpy(), l2.cpu().numpy()
        w1, h1 = mc.dims(W, H, 1)[1]
        top = [j for j, b in enumerate(plan.blocks()) if (b["x0"] >= w1 or b["y0"] >= h1) and lens[j] >= 64]
        assert top
        j = top[0]

        def decode(r):
            Hr, Wr = plan.reduced_shape(r)
            back = torch.zeros((Hr, Wr * 4), dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, reduce=r)
            plan.frame_status()                  # raises unless J2K_OK
            return back.cpu().numpy()
        full, half = decode(0), decode(1)
        # (the first bytes of the body: the MQ codeword's start / the HT block's MagSgn bytes)
        at = int(offs[j]) + 2
        cs[at:at + 24] = cs[at:at + 24] ^ 0x55
        plan.ctx.sync()
        assert np.array_equal(decode(1), half)
        assert not np.array_equal(decode(0), full)
    finally:
        plan.close()


# ---- 6, refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    torch, orc, t2ref, ctx = env
    from j2kgfx import J2KError, _lib
    from j2kgfx.codec import FramePlan
    W, H, Cn, prec, tile, nres = mc.LOSSLESS[1]
    L = mc.levels_of(nres)
    pix, planes = _closed_loop_frame(orc, mc.LOSSLESS[1], 43)

    def status(fn):
        try:
            fn()
        except J2KError as e:
            return e.status
        return _lib.OK
    plain = FramePlan(W, H, Cn, precision=prec, num_resolutions=nres, cb=(CB, CB), tile=tile, ctx=ctx, closed_loop=True)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres)
    try:
        cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA8, _dev(torch, plan, pix))
        plan.frame_status()
        total = int(toffs[-1].item())
        coeff = plan.alloc_coeff().zero_()
        sentinel = torch.full((H, W * 4), 0x5A, dtype=torch.uint8, device=plan.device)
        frame = torch.full((Cn, H, W), -77, dtype=torch.int32, device=plan.device)
        for r in (1, 0):
            ask = lambda p, r=r: p.ctx.check(p.ctx.L.j2k_plan_inverse_reduced(p.h, p._p(coeff), r, p._p(frame)))     # noqa: E731
            assert status(lambda: ask(plain)) == _lib.ERR_UNSUPPORTED
        assert status(lambda: plain.reduced_shape(1)) == _lib.ERR_UNSUPPORTED
        assert status(lambda: plain.inverse_pixels(coeff, sentinel, reduce=1)) == _lib.ERR_UNSUPPORTED
        assert status(lambda: plain.decode_frame_pixels(cs, total, sentinel, reduce=1)) == _lib.ERR_UNSUPPORTED
        assert status(lambda: plain.decode_pixels_host(cs[:total].cpu().numpy(), (H, W * 4), reduce=1)) == _lib.ERR_UNSUPPORTED
        for r in (L + 1, -1):
            assert status(lambda: plan.reduced_shape(r)) == _lib.ERR_INVALID_ARG, r
            assert status(lambda: plan.inverse(coeff, frame, reduce=r)) == _lib.ERR_INVALID_ARG, r
            assert status(lambda: plan.inverse_pixels(coeff, sentinel, reduce=r)) == _lib.ERR_INVALID_ARG, r
            assert status(lambda: plan.decode_frame_pixels(cs, total, sentinel, reduce=r)) == _lib.ERR_INVALID_ARG, r
            assert status(lambda: plan.decode_pixels_host(cs[:total].cpu().numpy(), (H, W * 4), reduce=r)) == _lib.ERR_INVALID_ARG, r
        plan.ctx.sync()
        assert bool((sentinel == 0x5A).all()) and bool((frame == -77).all())
        # a tile size that 2^reduce does not divide (128 x 32 tiles, seven resolutions: reduce 6 is in range, 32 is no multiple of 64); a batch
        # whose frame_rows it does not divide
        deep = _plan(ctx, W, H, Cn, prec, tile, 7)
        assert status(lambda: deep.inverse(deep.alloc_coeff().zero_(), reduce=5)) == _lib.OK
        assert status(lambda: deep.inverse(deep.alloc_coeff().zero_(), reduce=6)) == _lib.ERR_INVALID_ARG
        assert status(lambda: deep.decode_frame_pixels(cs, total, sentinel, reduce=6)) == _lib.ERR_INVALID_ARG
        deep.close()
        odd = _plan(ctx, 100, 60, 1, 8, (40, 24), 6)
        assert status(lambda: odd.inverse(odd.alloc_coeff().zero_(), reduce=3)) == _lib.OK
        assert status(lambda: odd.inverse(odd.alloc_coeff().zero_(), reduce=4)) == _lib.ERR_INVALID_ARG
        odd.close()
        batch = _plan(ctx, W, 2 * H, Cn, prec, tile, nres, frame_rows=H)
        assert status(lambda: batch.inverse(batch.alloc_coeff().zero_(), reduce=2)) == _lib.OK
        assert status(lambda: batch.inverse(batch.alloc_coeff().zero_(), reduce=3)) == _lib.ERR_INVALID_ARG
        batch.close()
        # a stream the decoder refuses leaves d_pix untouched, at every reduce
        def truncated(out, r):                        # (half the stream: the tile-parts run out)
            plan.decode_frame_pixels(cs, total // 2, out, reduce=r)
            plan.frame_status()
        for r in (0, 1, 3):
            Hr, Wr = plan.reduced_shape(r)
            out = torch.full((Hr, Wr * 4), 0x5A, dtype=torch.uint8, device=plan.device)
            assert status(lambda: truncated(out, r)) == _lib.ERR_INVALID_ARG, r
            assert bool((out == 0x5A).all()), r
            plan.decode_frame_pixels(cs, total, out, reduce=r)
            plan.frame_status()
            assert not bool((out == 0x5A).all()), r
    finally:
        plan.close()
        plain.close()


# ---- 7, a batch and a shard --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", [0, 1], ids=["mq", "ht"])
def test_batch(env, coder):
    """two frames of 260 x 44, frame_rows = 44 (44 = 4 * 11: reduce 2 is admissible), tiles 128 x 32"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import _lib
    W, H, Cn, prec, tile, nres = mc.LOSSLESS[1]
    frames = [_closed_loop_frame(orc, mc.LOSSLESS[1], 51 + b) for b in range(2)]
    pix = np.concatenate([f[0] for f in frames])
    want = ref.oracle_batch([f[1] for f in frames], W, H, tile[0], tile[1], nres, CB, coder, True, True, mc.MallatOracle(orc), t2ref)
    plan = _plan(ctx, W, 2 * H, Cn, prec, tile, nres, coder=coder, frame_rows=H)
    try:
        cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA8, _dev(torch, plan, pix), sop=True, eph=True)
        plan.frame_status()
        total = int(toffs[-1].item())
        assert bytes(cs[:total].cpu().numpy()) == b"".join(g["part"] for g in want)
        assert mc.admissible(W, 2 * H, tile, nres, frame_rows=H) == [0, 1, 2]
        tiles = mc.decoded_tiles(orc, dict(enumerate(want)), Cn, nres, CB, coder)
        for r in (1, 2):
            exp = mc.pixels(orc, mc.inverse_frame(orc, tiles, W, 2 * H, tile, prec, nres, reduce=r, frame_rows=H), prec)
            back = torch.zeros(exp.shape, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=True, eph=True, reduce=r)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), r
    finally:
        plan.close()


@pytest.mark.parametrize("coder", [0, 1], ids=["mq", "ht"])
def test_shard(env, coder):
    """tiles 1 and 2 of the 260 x 44 frame at reduce 1: only the shard's tiles are written"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import _lib
    W, H, Cn, prec, tile, nres = mc.LOSSLESS[1]
    pix, planes = _closed_loop_frame(orc, mc.LOSSLESS[1], 61)
    want = mc.oracle_frame(planes, W, H, tile[0], tile[1], nres, CB, coder, False, False, orc, t2ref, precision=prec)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres, coder=coder, tile_first=1, tile_count=2)
    try:
        cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA8, _dev(torch, plan, pix))
        plan.frame_status()
        total = int(toffs[-1].item())
        assert bytes(cs[:total].cpu().numpy()) == want[1]["part"] + want[2]["part"]
        tiles = mc.decoded_tiles(orc, want, Cn, nres, CB, coder)
        r = 1
        full = mc.pixels(orc, mc.inverse_frame(orc, tiles, W, H, tile, prec, nres, reduce=r), prec)
        exp = np.full_like(full, 0x5A)
        for t, (x, y, w, h) in enumerate(mc.reduced_rects(W, H, tile, r)):
            if t in (1, 2):
                exp[y:y + h, 4 * x:4 * (x + w)] = full[y:y + h, 4 * x:4 * (x + w)]
        back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, total, back, reduce=r)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp)
        frame = torch.full((Cn,) + plan.reduced_shape(r), -77, dtype=torch.int32, device=plan.device)
        placed = mc.flat_coeff(plan.planes() - np.array([1, 0, 0, 0, 0, 0, 0]), tiles[1:3], int(plan.info.coeff_elems))
        plan.inverse(_dev(torch, plan, placed), frame, reduce=r)
        plan.ctx.sync()
        assert np.array_equal(frame.cpu().numpy(), mc.inverse_frame(orc, tiles, W, H, tile, prec, nres, reduce=r, only=(1, 2), fill=-77))
    finally:
        plan.close()


# ---- 8, a graph ----------------------------------------------------------------------------------------------------------------------------------
def test_graph(env):
    """decode_frame_pixels(reduce=1) captured once, replayed on a second stream of the same geometry"""
    torch, orc, t2ref, _ = env
    from j2kgfx import Context, _lib
    W, H, Cn, prec, tile, nres = mc.LOSSLESS[1]
    ctx = Context(0)
    plan = _plan(ctx, W, H, Cn, prec, tile, nres)
    try:
        streams = []
        for seed in (71, 72):
            pix, planes = _closed_loop_frame(orc, mc.LOSSLESS[1], seed)
            cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA8, _dev(torch, plan, pix), sop=True, eph=True)
            plan.frame_status()
            streams.append((cs.clone(), toffs.clone()))
        cs, toffs = streams[0][0].clone(), streams[0][1].clone()
        Hr, Wr = plan.reduced_shape(1)
        back = torch.zeros((Hr, Wr * 4), dtype=torch.uint8, device=plan.device)
        direct = []
        for s_cs, s_toffs in streams:                      # the direct calls (the first also makes the tables of reduce 1)
            plan.decode_frame_pixels(s_cs, int(s_cs.numel()), back, tile_offs=s_toffs, sop=True, eph=True, reduce=1)
            plan.frame_status()
            direct.append(back.cpu().numpy().copy())
        assert not np.array_equal(direct[0], direct[1])
        with ctx.capture() as g:
            plan.decode_frame_pixels(cs, int(cs.numel()), back, tile_offs=toffs, sop=True, eph=True, reduce=1)
        for k in (0, 1, 0):
            cs.copy_(streams[k][0])
            toffs.copy_(streams[k][1])
            back.zero_()
            torch.cuda.synchronize()
            g.launch()
            ctx.sync()
            assert np.array_equal(back.cpu().numpy(), direct[k]), k
        g.close()
    finally:
        plan.close()
        ctx.close()
