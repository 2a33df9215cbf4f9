"""GPU: the specialised 5-3 forms of a Mallat plan -- packed-RGBA8 workgroup level 0, single-component planes in workgroup form at level 0 --
and the pixel fusion they bring, against the expectation of tests/mallat_cases.py on the cases of
tests/mallat_forms_cases.py (checked on the CPU by tests/test_mallat_forms_ref.py).  Every comparison is bit for bit.

Which test reaches which site of the product:
  dwt53_fwd_rgba8_wg_kernel<8, 1, 6, MAL> / dwt53_inv_rgba8_wg_kernel<4, 5, false, MAL>     cases 1, 2, 3, 8 of test_pixels, test_closed_loop
  dwt53_*_plane_wg_kernel<.., MAL>: SRC / DST 1 (case 5, MULTI), 2 (6), 3 (8), 4 (7 NC = 3, 9); 0 = level 0 of an int32 frame (test_planar_gray)    test_pixels
  pix_fusable's Mallat rule                                                                   test_pixels (the table), test_misaligned, test_options_off,
                                                                                              test_other_settings_stage_and_say_so
  the launch counts                                                                           test_dispatch_counts"""
import functools

import numpy as np
import pytest

import closed_loop_ref as ref
import lossless53_cases as ll
import mallat_cases as mc
import mallat_forms_cases as fc

pytestmark = pytest.mark.gpu
CB = 64
PIX_CASES = [i for i, c in enumerate(fc.CASES) if fc.pix_format(c) is not None]


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    import t2ref
    from j2kgfx import Context
    ctx = Context(0)
    yield torch, orc, t2ref, ctx
    ctx.close()


def _plan(ctx, case, coder=0, **kw):
    from j2kgfx.codec import FramePlan
    W, H, Cn, prec, tile, nres = case
    return FramePlan(W, H, Cn, precision=prec, lossless=True, num_resolutions=nres, cb=(CB, CB), tile=tile, coder=coder, ctx=ctx, mallat=True, **kw)


def _dev(torch, plan, a):
    return torch.from_numpy(np.array(a, order="C")).to(plan.device)            # (a copy: the shared expectations are read-only)


def _stride(case, W=None):
    """the row rounded up to 16 bytes plus 16 bytes of padding"""
    return ((W or case[0]) * fc.bpp(case) + 15) // 16 * 16 + 16


@functools.lru_cache(None)
def _expectation(i, family):
    """(frame, coefficient tiles) of case i: computed once, shared, never written"""
    import oracle as orc
    case = fc.CASES[i]
    frm = fc.frame(case, family)
    tiles = mc.forward_frame(orc, frm, case[4], case[3], case[5])
    frm.setflags(write=False)
    for t in tiles:
        t.setflags(write=False)
    return frm, tiles


def _padded(pix_rows, H, stride):
    out = np.full((H, stride), 0x5A, np.uint8)
    out[:, :pix_rows.shape[1]] = pix_rows
    return out


def _pixels_both_ways(torch, orc, plan, case, frm, tiles, stride, fused, offset=0):
    """forward_pixels + inverse_pixels on a [H, stride] buffer that starts `offset` bytes into its allocation; returns (coefficients, pixels)"""
    W, H, Cn, prec, tile, nres = case
    fmt = fc.pix_format(case)
    src = ll.pack_pixels(fmt, frm, stride, pad_byte=0x5A)
    if prec == 8:       # (the source IS createImage of the frame; at 16 bit createImage's own rescale wraps above 32768, decoder.go:434-451)
        assert np.array_equal(src[:, :W * fc.bpp(case)], mc.pixels(orc, np.asarray(frm), prec))

    def buf(a):
        flat = torch.full((H * stride + 16,), 0x5A, dtype=torch.uint8, device=plan.device)
        view = flat[offset:offset + H * stride].view(H, stride)
        view.copy_(torch.from_numpy(a).to(plan.device))
        return view
    d_src = buf(src)
    assert (plan.pixels_fused(fmt, d_src), plan.pixels_fused(fmt, d_src, inverse=True)) == (bool(fused[0]), bool(fused[1]))
    want = mc.flat_coeff(plan.planes(), tiles, int(plan.info.coeff_elems))
    coeff = plan.forward_pixels(fmt, d_src, plan.alloc_coeff().zero_())
    plan.ctx.sync()
    got = coeff.cpu().numpy()[:want.size]
    assert np.array_equal(got, want)
    out = buf(np.full((H, stride), 0x5A, np.uint8))
    plan.inverse_pixels(coeff, out)
    plan.ctx.sync()
    back = out.cpu().numpy()
    want_pix = _padded(mc.pixels(orc, mc.inverse_frame(orc, tiles, W, H, tile, prec, nres), prec), H, stride)
    assert np.array_equal(back, want_pix)                          # the padding is intact
    if prec == 8:
        assert np.array_equal(back, src)                           # ... and lossless: the source itself
    return got, back


# ---- 1, pixels in and out -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["noise", "impulse"])
@pytest.mark.parametrize("i", PIX_CASES, ids=[fc.case_id(fc.CASES[i]) for i in PIX_CASES])
def test_pixels(env, i, family):
    torch, orc, t2ref, ctx = env
    case = fc.CASES[i]
    frm, tiles = _expectation(i, family)
    plan = _plan(ctx, case)
    try:
        _pixels_both_ways(torch, orc, plan, case, frm, tiles, _stride(case), fc.FUSED[i])
    finally:
        plan.close()


def test_planar_frame(env):
    """case 10 (12 bit, no pixel format): int32 planes in and out, general launches"""
    torch, orc, t2ref, ctx = env
    case = fc.CASES[9]
    W, H, Cn, prec, tile, nres = case
    plan = _plan(ctx, case)
    try:
        for family in ("noise", "impulse"):
            frm, tiles = _expectation(9, family)
            want = mc.flat_coeff(plan.planes(), tiles, int(plan.info.coeff_elems))
            coeff = plan.forward(_dev(torch, plan, frm), plan.alloc_coeff().zero_())
            plan.ctx.sync()
            assert np.array_equal(coeff.cpu().numpy()[:want.size], want)
            back = plan.inverse(coeff)
            plan.ctx.sync()
            assert np.array_equal(back.cpu().numpy(), frm)
    finally:
        plan.close()


def test_planar_gray(env):
    """case 5's geometry as an int32 frame: level 0 of a single component in plane-workgroup form with int32 planes (SRC / DST 0), three strips"""
    torch, orc, t2ref, ctx = env
    case = fc.CASES[4]
    W, H, Cn, prec, tile, nres = case
    frm, tiles = _expectation(4, "noise")
    plan = _plan(ctx, case)
    try:
        want = mc.flat_coeff(plan.planes(), tiles, int(plan.info.coeff_elems))
        coeff = plan.forward(_dev(torch, plan, frm), plan.alloc_coeff().zero_())
        plan.ctx.sync()
        assert np.array_equal(coeff.cpu().numpy()[:want.size], want)
        back = plan.inverse(coeff)
        plan.ctx.sync()
        assert np.array_equal(back.cpu().numpy(), frm)
    finally:
        plan.close()


# ---- 2, coefficients no forward transform made ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["noise", "fullrange"])
@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=[fc.case_id(c) for c in fc.CASES])
def test_arbitrary_coefficients(env, i, family):
    """inverse / inverse_pixels at reduce 0 (aligned buffer: the fused path where the table says so) and at every admissible reduce"""
    torch, orc, t2ref, ctx = env
    case = fc.CASES[i]
    W, H, Cn, prec, tile, nres = case
    fmt = fc.pix_format(case)
    plan = _plan(ctx, case)
    try:
        tiles = [np.stack([ll.coeff_plane(family, w, h, 5 * t + c) for c in range(Cn)]) for t, (x0, y0, w, h) in enumerate(mc.tiles_of(W, H, tile))]
        d_coeff = _dev(torch, plan, mc.flat_coeff(plan.planes(), tiles, max(int(plan.info.coeff_elems), 4)))
        for r in mc.admissible(W, H, tile, nres):
            want = mc.inverse_frame(orc, tiles, W, H, tile, prec, nres, reduce=r)
            Hr, Wr = want.shape[1:]
            assert plan.reduced_shape(r) == (Hr, Wr)
            frame = torch.full((Cn, Hr, Wr), -77, dtype=torch.int32, device=plan.device)
            plan.inverse(d_coeff, frame, reduce=r)
            plan.ctx.sync()
            assert np.array_equal(frame.cpu().numpy(), want), r
            if fmt is None:
                continue
            stride = _stride(case, Wr)
            out = torch.full((Hr, stride), 0x5A, dtype=torch.uint8, device=plan.device)
            if r == 0:
                assert plan.pixels_fused(fmt, out, inverse=True) == bool(fc.FUSED[i][1])
            plan.inverse_pixels(d_coeff, out, reduce=r)
            plan.ctx.sync()
            assert np.array_equal(out.cpu().numpy(), _padded(mc.pixels(orc, want, prec), Hr, stride)), r
    finally:
        plan.close()


# ---- 3, misaligned buffers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["offset4", "stride8"])
def test_misaligned(env, how):
    """case 1 with the pixel pointer 4 bytes into a 16-byte lane / a stride that is 8 mod 16: staged, same results as aligned"""
    torch, orc, t2ref, ctx = env
    case = fc.CASES[0]
    frm, tiles = _expectation(0, "noise")
    plan = _plan(ctx, case)
    try:
        aligned = _pixels_both_ways(torch, orc, plan, case, frm, tiles, _stride(case), (1, 1))
        if how == "offset4":
            other = _pixels_both_ways(torch, orc, plan, case, frm, tiles, _stride(case), (0, 0), offset=4)
        else:
            other = _pixels_both_ways(torch, orc, plan, case, frm, tiles, _stride(case) + 8, (0, 0))
        W = case[0] * fc.bpp(case)
        assert np.array_equal(other[0], aligned[0]) and np.array_equal(other[1][:, :W], aligned[1][:, :W])
    finally:
        plan.close()


# ---- 4, the options off -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 2, 4], ids=[fc.case_id(fc.CASES[i]) for i in (0, 2, 4)])
def test_options_off(env, i):
    """pix_fuse = 0, l0_wg = 0, plane_wg = 0: the general Mallat launches and staged pixels -- the same coefficients and pixels"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import Context
    case = fc.CASES[i]
    frm, tiles = _expectation(i, "noise")
    off = Context(0)
    try:
        for name in ("pix_fuse", "l0_wg", "plane_wg"):
            off.set_option(name, 0)
        results = []
        for c, fused in ((ctx, fc.FUSED[i]), (off, (0, 0))):
            plan = _plan(c, case)
            try:
                results.append(_pixels_both_ways(torch, orc, plan, case, frm, tiles, _stride(case), fused))
            finally:
                plan.close()
        assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    finally:
        off.close()


# ---- 4b, settings the Mallat kernels are not instantiated for ------------------------------------------------------------------------------
# (forward, inverse) of case 1, by hand: the forward table is built for l0_wg = 8 with l0_store = 1 only, the inverse table for four waves with
# l0_inv_wpe = 5 only and is used only while l0_wg_inv is on; whichever direction loses its table stages its pixels, the other still fuses
KNOBS = ((("l0_wg", 4), (0, 1)), (("l0_store", 0), (0, 1)), (("l0_wg_invw", 8), (1, 0)), (("l0_inv_wpe", 6), (1, 0)), (("l0_wg_inv", 0), (1, 0)))


@pytest.mark.parametrize("option,fused", KNOBS, ids=["%s=%d" % k[0] for k in KNOBS])
def test_other_settings_stage_and_say_so(env, option, fused):
    """pixels_fused tells the truth, and the results are those of the default context"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import Context
    case = fc.CASES[0]
    frm, tiles = _expectation(0, "noise")
    other = Context(0)
    try:
        other.set_option(*option)
        plan = _plan(other, case)
        try:
            _pixels_both_ways(torch, orc, plan, case, frm, tiles, _stride(case), fused)       # (checked against the expectation, as the default is)
        finally:
            plan.close()
    finally:
        other.close()


# ---- 5, dispatch counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [(), (("l0_wg", 0), ("plane_wg", 0), ("pix_fuse", 0))], ids=["default", "options-off"])
def test_dispatch_counts(env, options):
    """case 1: level 0 is ONE dispatch per direction -- the pixels are read / written by it (default) or staged by untagged pack / unpack
    launches (options off) -- and every level below is one general launch"""
    torch, orc, t2ref, _ = env
    from j2kgfx import Context
    case = fc.CASES[0]
    fmt = fc.pix_format(case)
    frm, _tiles = _expectation(0, "noise")
    ctx = Context(0)
    plan = None
    try:
        for name, v in options:
            ctx.set_option(name, v)
        plan = _plan(ctx, case)
        d_src = _dev(torch, plan, ll.pack_pixels(fmt, frm, _stride(case), pad_byte=0x5A))
        assert plan.pixels_fused(fmt, d_src) == (not options) and plan.pixels_fused(fmt, d_src, inverse=True) == (not options)
        out = torch.empty_like(d_src)
        coeff = plan.forward_pixels(fmt, d_src)
        plan.inverse_pixels(coeff, out)                # (once before: workspaces)
        ctx.profile_enable(2)
        plan.forward_pixels(fmt, d_src, coeff)
        plan.inverse_pixels(coeff, out)
        got = {tag: ctx.profile_read_tag(tag)[0] for tag in range(4)}
        ctx.profile_enable(0)
        print("dispatches per tag", options, got)
        assert got == fc.DISPATCHES_CASE1
    finally:
        if plan is not None:
            plan.close()
        ctx.close()


# ---- 6, the closed loop -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder,marks", [(0, False), (1, True)], ids=["mq-bare", "ht-sop_eph"])
@pytest.mark.parametrize("i", [0, 2], ids=[fc.case_id(fc.CASES[i]) for i in (0, 2)])
def test_closed_loop(env, i, coder, marks):
    torch, orc, t2ref, ctx = env
    case = fc.CASES[i]
    W, H, Cn, prec, tile, nres = case
    fmt = fc.pix_format(case)
    pix, Cn2, prec2, planes = ref.pixel_frame(fmt, W, H, 131 + coder, orc, noise=(1 << prec) // 16)
    assert (Cn2, prec2) == (Cn, prec) and pix.shape == (H, W * 4)
    want = mc.oracle_frame(planes, W, H, tile[0], tile[1], nres, CB, coder, marks, marks, orc, t2ref, precision=prec)
    plan = _plan(ctx, case, coder=coder)
    try:
        d_pix = _dev(torch, plan, pix)
        assert plan.pixels_fused(fmt, d_pix) and plan.pixels_fused(fmt, d_pix, inverse=True)
        cs, toffs = plan.encode_frame_pixels(fmt, d_pix, sop=marks, eph=marks)
        plan.frame_status()
        h_cs, h_toffs = cs.cpu().numpy(), toffs.cpu().numpy()
        for k, t in enumerate(sorted(want)):
            assert bytes(h_cs[int(h_toffs[k]):int(h_toffs[k + 1])]) == want[t]["part"], t
        total = int(h_toffs[-1])
        exp = mc.pixels(orc, mc.inverse_frame(orc, mc.decoded_tiles(orc, want, Cn, nres, CB, coder), W, H, tile, prec, nres), prec)
        back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=marks, eph=marks)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp)
        if coder == 0:
            assert np.array_equal(exp, pix)                # the MQ loop is lossless
        if i == 2 and coder == 0:                          # the host calls, once
            enc = plan.encode_pixels_host(fmt, pix, sop=marks, eph=marks)
            assert bytes(enc["bytes"]) == bytes(h_cs[:total])
            assert np.array_equal(plan.decode_pixels_host(enc["bytes"], exp.shape, sop=marks, eph=marks), pix)
    finally:
        plan.close()


# ---- 7, a batch, shards, a graph -------------------------------------------------------------------------------------------------------------
def test_batch(env):
    """case 3 as two frames, frame_rows = 44"""
    torch, orc, t2ref, ctx = env
    case = fc.CASES[2]
    W, H, Cn, prec, tile, nres = case
    fmt = fc.pix_format(case)
    frames = [ref.pixel_frame(fmt, W, H, 151 + b, orc, noise=16) for b in range(2)]
    pix = np.concatenate([f[0] for f in frames])
    want = ref.oracle_batch([f[3] for f in frames], W, H, tile[0], tile[1], nres, CB, 1, True, True, mc.MallatOracle(orc), t2ref)
    plan = _plan(ctx, (W, 2 * H, Cn, prec, tile, nres), coder=1, frame_rows=H)
    try:
        d_pix = _dev(torch, plan, pix)
        assert plan.pixels_fused(fmt, d_pix) and plan.pixels_fused(fmt, d_pix, inverse=True)
        cs, toffs = plan.encode_frame_pixels(fmt, d_pix, sop=True, eph=True)
        plan.frame_status()
        total = int(toffs[-1].item())
        assert bytes(cs[:total].cpu().numpy()) == b"".join(g["part"] for g in want)
        tiles = mc.decoded_tiles(orc, dict(enumerate(want)), Cn, nres, CB, 1)
        exp = mc.pixels(orc, mc.inverse_frame(orc, tiles, W, 2 * H, tile, prec, nres, frame_rows=H), prec)
        back = torch.zeros(exp.shape, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=True, eph=True)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp)
    finally:
        plan.close()


def test_shards(env):
    """case 3 as two shards (tile 0; tiles 1, 2, 3) into ONE pixel frame: each writes only its tiles"""
    torch, orc, t2ref, ctx = env
    case = fc.CASES[2]
    W, H, Cn, prec, tile, nres = case
    fmt = fc.pix_format(case)
    pix, _, _, planes = ref.pixel_frame(fmt, W, H, 161, orc, noise=16)
    want = mc.oracle_frame(planes, W, H, tile[0], tile[1], nres, CB, 0, False, False, orc, t2ref, precision=prec)
    rects = mc.tiles_of(W, H, tile)
    d_pix = None
    back = None
    seen = np.full(pix.shape, 0x5A, np.uint8)
    for first, count in ((0, 1), (1, 3)):
        plan = _plan(ctx, case, coder=0, tile_first=first, tile_count=count)
        try:
            if d_pix is None:
                d_pix = _dev(torch, plan, pix)
                back = torch.full(pix.shape, 0x5A, dtype=torch.uint8, device=plan.device)
            assert plan.pixels_fused(fmt, d_pix) and plan.pixels_fused(fmt, back, inverse=True)
            cs, toffs = plan.encode_frame_pixels(fmt, d_pix)
            plan.frame_status()
            total = int(toffs[-1].item())
            assert bytes(cs[:total].cpu().numpy()) == b"".join(want[t]["part"] for t in range(first, first + count))
            plan.decode_frame_pixels(cs, total, back)
            plan.frame_status()
            for t in range(first, first + count):
                x0, y0, w, h = rects[t]
                seen[y0:y0 + h, 4 * x0:4 * (x0 + w)] = pix[y0:y0 + h, 4 * x0:4 * (x0 + w)]
            assert np.array_equal(back.cpu().numpy(), seen), (first, count)
        finally:
            plan.close()
    assert np.array_equal(seen, pix)


def test_graph(env):
    """case 1, MQ coder: encode_frame_pixels + decode_frame_pixels run once, captured, replayed on new pixels in the same buffers"""
    torch, orc, t2ref, _ = env
    from j2kgfx import Context
    case = fc.CASES[0]
    W, H, Cn, prec, tile, nres = case
    fmt = fc.pix_format(case)
    ctx = Context(0)
    plan = _plan(ctx, case, coder=0)
    try:
        frames = [ref.pixel_frame(fmt, W, H, 171 + k, orc, noise=16)[0] for k in range(2)]
        d_pix = _dev(torch, plan, frames[0])
        back = torch.zeros_like(d_pix)
        tiles = int(plan.info.tiles)
        cs = plan.empty(plan.frame_bound(), torch.uint8)
        toffs = plan.empty(tiles + 1, torch.int64)[:tiles + 1]
        assert plan.pixels_fused(fmt, d_pix) and plan.pixels_fused(fmt, back, inverse=True)

        def code():
            plan.encode_frame_pixels(fmt, d_pix, True, True, cs, toffs)
            plan.decode_frame_pixels(cs, cs.numel(), back, toffs, True, True)
        code()
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), frames[0])
        direct = cs.clone()
        with ctx.capture() as g:
            code()
        for k in (1, 0):
            d_pix.copy_(torch.from_numpy(frames[k]).to(plan.device))
            back.zero_()
            cs.zero_()
            torch.cuda.synchronize()
            g.launch()
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), frames[k]), k
        n = int(toffs[-1].item())
        assert torch.equal(cs[:n], direct[:n])
        g.close()
    finally:
        plan.close()
        ctx.close()
