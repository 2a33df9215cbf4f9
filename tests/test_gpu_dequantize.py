"""GPU: j2k_plan_set_dequantize -- dwt.Dequantize (dwt.go:514-520) fused into the loads of every 9-7 inverse kernel form -- and the unit calls
j2k_quantize / j2k_dequantize, against the expectation of tests/dequantize_cases.py (checked on the CPU by tests/test_dequantize_ref.py).
Every comparison is bit for bit (np.array_equal / torch.equal); the only bound is the reconstruction error of the end-to-end frames, which
is the oracle's own (dequantize_cases.MAX_ERR).

Which test reaches which site of the product (csrc/dwt97.hip, csrc/dwt97_l0wg_inv.inc):

  dwt97_inv_kernel<2, 3, true>, <4, 1, true>, <2, 1, true> (inv97_load_row)      test_inverse_level0[nw0], test_planes[wg0]
  dwt97_inv_rgb_wg_kernel<6 ... 12, ., false>: half_values and the xslot row    test_inverse_level0[nw6 ... nw12] (heights of two bands)
  dwt97_inv_rgb_wg_kernel<8, ., true>                                           test_inverse_pixels, the 8-bit RGB frames of test_closed_loop_mq
  dwt97_inv_plane_wg_kernel<8, 6, false, false> (deeper levels)                 test_inverse_level0 (nres 3, 6, 1), test_planes[wg8]
  dwt97_inv_plane_wg_kernel<8, 6, false, true> (one component, image.Gray)      test_planes[wg8], test_inverse_pixels_gray
  plan_inverse_impl behind every entry point                                   test_closed_loop_mq (decode_frame_pixels, decode_pixels_host, inverse),
                                                                                test_closed_loop_ht, test_graph_keeps_the_setting_it_was_captured_with"""
import os

import numpy as np
import pytest

import closed_loop_ref as ref
import dequantize_cases as dq
import lossy97_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx_for():
    """a context per knob setting, made once for the module (the knobs are read when a context is created)"""
    from j2kgfx import Context
    cache = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in cache:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update({k: str(v) for k, v in env.items()})
            try:
                cache[key] = Context(0)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return cache[key]

    yield get
    for c in cache.values():
        c.close()


@pytest.fixture(scope="module")
def env(ctx_for):
    import torch
    import oracle as orc
    import t2ref
    return torch, orc, t2ref, ctx_for()


def _nrs(nw):
    return (nw - 3, lc.defaults()["band_prows_97"])


def _coefficient_sets(plan, nw, family):
    """(flat coefficient buffer of the plan, {(tile, comp): plane}) of one family"""
    buf = np.zeros(int(plan.info.coeff_elems), np.int32)
    per = {}
    for t, c, x0, y0, w, h, off in (tuple(int(v) for v in r) for r in plan.planes()):
        p = lc.coeff_plane(family, w, h, 3 * (x0 + y0) + c, _nrs(nw))
        per[(t, c)] = p
        buf[off:off + w * h] = p.reshape(-1)
    return buf, per


def _expected_frame(oracle, plan, per, ncomp, prec, nres, quality, W, H, multiply=True):
    rows = plan.planes()
    out = np.zeros((ncomp, H, W), np.int32)
    for t in np.unique(rows[:, 0]):
        x0, y0, w, h = (int(v) for v in rows[rows[:, 0] == t][0, 2:6])
        coefs = np.stack([per[(int(t), c)] for c in range(ncomp)])
        out[:, y0:y0 + h, x0:x0 + w] = dq.expect_dequantized(oracle, coefs, prec, nres, quality, multiply)
    return out


# ---- level 0, every form ------------------------------------------------------------------------------------------------------------------
LEVEL0 = [(i, c._replace(quality=lc.QUALITIES[i % 8])) for i, c in enumerate(lc.inverse_cases())]


@pytest.mark.parametrize("i,case", LEVEL0, ids=[c.id for _, c in LEVEL0])
def test_inverse_level0(oracle, ctx_for, i, case):
    """lossy97_cases.inverse_cases() with the qualities going round: ARBITRARY int32 coefficients (`outrange` through Go's out-of-range
    conversion) -> frame with the option on, every J2K_L0_WG97_INV, heights of two bands (the xslot row), no / one / deep float64 prefixes (a
    value from the prefix is not multiplied again), the tiled frames"""
    import torch
    from j2kgfx.codec import FramePlan
    plan = FramePlan(case.W, case.H, 3, ctx=ctx_for(J2K_L0_WG97_INV=case.nw), precision=case.prec, lossless=False, quality=case.quality,
                     num_resolutions=case.nres, cb=(64, 64), tile=case.tile, coder=0)
    try:
        plan.set_dequantize(True)
        for family in case.families:
            buf, per = _coefficient_sets(plan, case.nw, family)
            back = plan.inverse(torch.from_numpy(buf).to(plan.device))
            plan.ctx.sync()
            want = _expected_frame(oracle, plan, per, 3, case.prec, case.nres, case.quality, case.W, case.H)
            got = back.cpu().numpy()
            assert np.array_equal(got, want), family
            if case.quality == 1:            # step 1.0: the parent's result, the same bits
                assert np.array_equal(got, _expected_frame(oracle, plan, per, 3, case.prec, case.nres, 1, case.W, case.H, multiply=False)), family
                rows = plan.planes()
                t0 = rows[rows[:, 0] == 0]
                x0, y0, w, h = (int(v) for v in t0[0, 2:6])
                assert np.array_equal(got[:, y0:y0 + h, x0:x0 + w], lc.expect_inverse(oracle, np.stack([per[(0, c)] for c in range(3)]), case.prec, case.nres)), family
    finally:
        plan.close()


# ---- packed pixels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,tile", [(512, 11, (0, 0)), (24, 10, (0, 0)), (280, 13, (256, 128)), (536, 25, (256, 22)), (248, 21, (0, 0)), (16, 2, (0, 0))])
@pytest.mark.parametrize("nres", [2, 6])
@pytest.mark.parametrize("quality", [2, 75])
def test_inverse_pixels(oracle, W, H, tile, nres, quality):
    """the shapes of test_gpu_lossy97_oracle.py::test_inverse_rgba8_pixels with the option on: still the fused kernel, decoder.createImage's
    clamp of the dequantised expectation"""
    import torch
    from j2kgfx.codec import FramePlan
    nw = lc.defaults()["l0_wg97_inv"]
    plan = FramePlan(W, H, 3, precision=8, lossless=False, quality=quality, num_resolutions=nres, cb=(64, 64), tile=tile, coder=0)
    try:
        plan.set_dequantize(True)
        for family in lc.COEFF_FAMILIES:
            buf, per = _coefficient_sets(plan, nw, family)
            out = torch.full((H, W * 4), 0x5A, dtype=torch.uint8, device=plan.device)
            assert plan.pixels_fused(2, out, inverse=True)                 # the kernel writes the pixels itself
            plan.inverse_pixels(torch.from_numpy(buf).to(plan.device), out)
            plan.ctx.sync()
            want = _expected_frame(oracle, plan, per, 3, 8, nres, quality, W, H)
            assert np.array_equal(out.cpu().numpy(), oracle.create_image([p for p in want], 8)), family
    finally:
        plan.close()


@pytest.mark.parametrize("quality", [2, 75])
def test_inverse_pixels_gray(oracle, quality):
    """image.Gray (PIX_GRAY8) through the single-plane workgroup kernel's pixel store; rows 32 bytes apart (the fused path wants 16-byte rows)"""
    import torch
    from j2kgfx.codec import FramePlan
    W, H, nres, stride = 24, 17, 3, 32
    plan = FramePlan(W, H, 1, precision=8, lossless=False, quality=quality, num_resolutions=nres, cb=(64, 64), coder=0)
    try:
        plan.set_dequantize(True)
        for family in lc.COEFF_FAMILIES:
            buf, per = _coefficient_sets(plan, lc.defaults()["plane_wg97"], family)
            out = torch.full((H, stride), 0x5A, dtype=torch.uint8, device=plan.device)
            assert plan.pixels_fused(0, out, inverse=True)
            plan.inverse_pixels(torch.from_numpy(buf).to(plan.device), out)
            plan.ctx.sync()
            want = _expected_frame(oracle, plan, per, 1, 8, nres, quality, W, H)
            got = out.cpu().numpy()
            assert np.array_equal(got[:, :W], oracle.create_image([want[0]], 8)), family
            assert (got[:, W:] == 0x5A).all()
    finally:
        plan.close()


# ---- single components and deeper levels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,Cn,tile,nres,prec,quality", lc.PLANE_FRAMES)
@pytest.mark.parametrize("wg", lc.PLANE_WAVES, ids=lambda v: "wg%d" % v)
def test_planes(oracle, ctx_for, wg, W, H, Cn, tile, nres, prec, quality):
    import torch
    from j2kgfx.codec import FramePlan
    plan = FramePlan(W, H, Cn, ctx=ctx_for(J2K_PLANE_WG97=wg), precision=prec, lossless=False, quality=quality, num_resolutions=nres, cb=(64, 64),
                     tile=tile, coder=0, dequantize=True)
    try:
        for family in ("noise", "impulse"):
            buf, per = _coefficient_sets(plan, lc.defaults()["plane_wg97"], family)
            back = plan.inverse(torch.from_numpy(buf).to(plan.device))
            plan.ctx.sync()
            assert np.array_equal(back.cpu().numpy(), _expected_frame(oracle, plan, per, Cn, prec, nres, quality, W, H)), family
    finally:
        plan.close()


# ---- the switch --------------------------------------------------------------------------------------------------------------------------------
def test_switch_on_off_and_lossless_refused(oracle):
    import torch
    from j2kgfx import J2KError, _lib
    from j2kgfx.codec import FramePlan
    W, H, nres, q = 248, 21, 3, 75
    plan = FramePlan(W, H, 3, precision=8, lossless=False, quality=q, num_resolutions=nres, cb=(64, 64), coder=0)
    try:
        buf, per = _coefficient_sets(plan, lc.defaults()["l0_wg97_inv"], "noise")
        d = torch.from_numpy(buf).to(plan.device)
        plain = lc.expect_inverse(oracle, np.stack([per[(0, c)] for c in range(3)]), 8, nres)
        deq = _expected_frame(oracle, plan, per, 3, 8, nres, q, W, H)
        assert not np.array_equal(plain, deq)
        seen = []
        for on in (None, True, False, True, False):
            if on is not None:
                plan.set_dequantize(on)
            back = plan.inverse(d)
            plan.ctx.sync()
            seen.append(np.array_equal(back.cpu().numpy(), deq if on else plain))
        assert seen == [True] * 5
    finally:
        plan.close()
    lossless = FramePlan(64, 32, 3, precision=8, lossless=True, num_resolutions=3, cb=(64, 64), coder=0)
    try:
        for on in (True, False):
            with pytest.raises(J2KError) as e:
                lossless.set_dequantize(on)
            assert e.value.status == _lib.ERR_UNSUPPORTED
        with pytest.raises(J2KError) as e:
            FramePlan(64, 32, 3, precision=8, lossless=True, num_resolutions=3, cb=(64, 64), coder=0, dequantize=True)
        assert e.value.status == _lib.ERR_UNSUPPORTED
    finally:
        lossless.close()


@pytest.mark.parametrize("coder", [0, 1])
def test_the_encode_side_does_not_see_the_option(env, coder):
    """forward, encode_stream and encode_frame_pixels: the same bytes with the option on and off"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    W, H = 200, 150
    pix, Cn, prec, planes = ref.pixel_frame(_lib.PIX_RGBA8, W, H, 77, orc)
    d_pix = torch.from_numpy(pix).to("cuda:%d" % ctx.device)
    d_frame = torch.from_numpy(planes).to("cuda:%d" % ctx.device)
    outs = []
    for on in (False, True):
        plan = FramePlan(W, H, 3, precision=8, lossless=False, quality=75, num_resolutions=4, cb=(16, 16), tile=(64, 64), coder=coder, ctx=ctx, closed_loop=True,
                         dequantize=on)
        coeff = plan.forward(d_frame)
        stream, offs, lens, numbps = plan.encode_stream(coeff)
        cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA8, d_pix, sop=True, eph=True)
        plan.frame_status()
        n = int(plan.info.blocks)
        total, ftotal = int(offs[n].item()), int(toffs[-1].item())
        outs.append((coeff[:int(plan.info.coeff_elems)].cpu(), stream[:total].cpu(), lens[:n].cpu(), numbps[:n].cpu(), cs[:ftotal].cpu(), toffs.cpu()))
        plan.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- closed loop, MQ, end to end ---------------------------------------------------------------------------------------------------------------
PIX_OF = {(1, 8): 0, (1, 16): 1, (3, 8): 2, (3, 16): 3, (4, 8): 4, (4, 16): 5}     # J2K_PIX_GRAY8 ... J2K_PIX_NRGBA64
CB = 16
HOST_FRAMES = (0, 7)


def _oracle_expectation(orc, t2ref, planes, f, sop, eph):
    """the dequantised frame [Cn, H, W] from the oracle's quantised coefficients of every tile"""
    W, H, Cn, prec, tile, nres, q = f
    want = ref.oracle_frame(planes, W, H, tile[0] or W, tile[1] or H, nres, CB, 0, sop, eph, orc, t2ref, precision=prec, lossless=False, quality=q)
    out = np.zeros((Cn, H, W), np.int32)
    for t in sorted(want):
        wt = want[t]
        out[:, wt["y0"]:wt["y0"] + wt["h"], wt["x0"]:wt["x0"] + wt["w"]] = dq.expect_dequantized(orc, np.stack(wt["coeff"]), prec, nres, q)
    return out, want


@pytest.mark.parametrize("i", range(len(dq.FRAMES)), ids=[dq.frame_id(f) for f in dq.FRAMES])
def test_closed_loop_mq(env, i):
    """pixels -> tile-parts -> pixels with the option on: the pixels are decoder.createImage of the expectation computed from the ORACLE's
    quantised coefficients, and within dequantize_cases.MAX_ERR of the source.  8 and 16 bit through encode_frame_pixels / decode_frame_pixels
    (frames 0 and 7 through the host calls as well), the 12-bit frame as int32 planes through the stage calls."""
    torch, orc, t2ref, ctx = env
    from j2kgfx.codec import FramePlan
    f = dq.FRAMES[i]
    W, H, Cn, prec, tile, nres, q = f
    sop, eph = bool(i & 1), bool(i & 2)
    plan = FramePlan(W, H, Cn, precision=prec, lossless=False, quality=q, num_resolutions=nres, cb=(CB, CB), tile=tile, coder=0, ctx=ctx, closed_loop=True,
                     dequantize=True)
    try:
        if prec == 12:
            frm = dq.source_frame(f, i)
            want, _ = _oracle_expectation(orc, t2ref, frm, f, sop, eph)
            stream, offs, lens, numbps = plan.encode_stream(plan.forward(torch.from_numpy(frm).to(plan.device)))
            cs, toffs = plan.encode_tile_parts(stream, offs, lens, numbps, sop=sop, eph=eph)
            plan.frame_status()
            o2, l2, n2 = plan.decode_tile_parts(cs, int(toffs[-1].item()), sop=sop, eph=eph)
            back = plan.inverse(plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2)))
            plan.frame_status()
            got = back.cpu().numpy()
            assert np.array_equal(got, want)
            err = int(np.abs(got.astype(np.int64) - frm).max())
            print("%s: max abs err %d" % (dq.frame_id(f), err))
            assert err <= dq.MAX_ERR
            return
        fmt = PIX_OF[(Cn, prec)]
        pix, Cn_, prec_, planes = ref.pixel_frame(fmt, W, H, dq.FRAME_SEED + i, orc)
        assert (Cn_, prec_) == (Cn, prec)
        want, tiles = _oracle_expectation(orc, t2ref, planes, f, sop, eph)
        want_pix = orc.create_image([p for p in want], prec)
        d_pix = torch.from_numpy(pix).to(plan.device)
        cs, toffs = plan.encode_frame_pixels(fmt, d_pix, sop=sop, eph=eph)
        plan.frame_status()
        total = int(toffs[-1].item())
        assert bytes(cs[:total].cpu().numpy()) == b"".join(tiles[t]["part"] for t in sorted(tiles))      # (the stream does not see the option)
        back = torch.full_like(d_pix, 0x5A)
        plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=sop, eph=eph)
        plan.frame_status()
        got = back.cpu().numpy()
        assert np.array_equal(got, want_pix)
        # the truth is what extractImageData reads in the source pixels (16 bit: createImage's wrap, closed_loop_ref.pixel_frame)
        seen = np.stack(orc.extract_image_data(got, fmt, W, H))
        ncmp = 3 if fmt in (2, 3) else Cn                              # (image.RGBA / RGBA64: alpha is not a component)
        err = int(np.abs(seen[:ncmp].astype(np.int64) - planes[:ncmp]).max())
        print("%s: max abs err %d" % (dq.frame_id(f), err))
        assert err <= dq.MAX_ERR
        if i in HOST_FRAMES:
            enc = plan.encode_pixels_host(fmt, pix, sop=sop, eph=eph)
            assert bytes(enc["bytes"]) == bytes(cs[:total].cpu().numpy())
            assert np.array_equal(plan.decode_pixels_host(enc["bytes"], pix.shape, sop=sop, eph=eph), want_pix)
    finally:
        plan.close()


# ---- HT coder ----------------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_ht(env):
    """not a round trip (the reference's HT decoder writes one row in four): with the option on the frame decoder equals the stage calls, and
    the inverse of the placed coefficients equals the expectation computed from those coefficients"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    W, H, tile, nres, q = 200, 150, (64, 64), 4, 75
    pix = ref.pixel_frame(_lib.PIX_RGBA8, W, H, 91, orc)[0]
    plan = FramePlan(W, H, 3, precision=8, lossless=False, quality=q, num_resolutions=nres, cb=(16, 16), tile=tile, coder=_lib.CODER_HT, ctx=ctx, closed_loop=True)
    try:
        plan.set_dequantize(True)
        d_pix = torch.from_numpy(pix).to(plan.device)
        cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA8, d_pix, sop=True, eph=True)
        plan.frame_status()
        total = int(toffs[-1].item())
        got = torch.zeros_like(d_pix)
        plan.decode_frame_pixels(cs, total, got, tile_offs=toffs, sop=True, eph=True)
        plan.frame_status()
        o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=toffs, sop=True, eph=True)
        placed = plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2))
        stage = plan.inverse_pixels(placed, torch.zeros_like(d_pix))
        back = plan.inverse(placed)
        plan.frame_status()
        assert torch.equal(got, stage)
        hp = placed.cpu().numpy()
        per = {(int(t), int(c)): hp[int(off):int(off) + int(w) * int(h)].reshape(int(h), int(w)) for t, c, x0, y0, w, h, off in plan.planes()}
        assert any(np.any(p) for p in per.values())
        want = _expected_frame(orc, plan, per, 3, 8, nres, q, W, H)
        assert np.array_equal(back.cpu().numpy(), want)
        assert np.array_equal(got.cpu().numpy(), orc.create_image([p for p in want], 8))
    finally:
        plan.close()


# ---- graph -------------------------------------------------------------------------------------------------------------------------------------
def test_graph_keeps_the_setting_it_was_captured_with(env):
    torch, orc, t2ref, ctx0 = env
    from j2kgfx import Context, _lib
    from j2kgfx.codec import FramePlan
    i = 0
    f = dq.FRAMES[i]
    W, H, Cn, prec, tile, nres, q = f
    ctx = Context(0)
    plan = FramePlan(W, H, Cn, precision=prec, lossless=False, quality=q, num_resolutions=nres, cb=(CB, CB), tile=tile, coder=0, ctx=ctx, closed_loop=True)
    try:
        pix, _, _, planes = ref.pixel_frame(_lib.PIX_RGBA8, W, H, dq.FRAME_SEED + i, orc)
        want, _ = _oracle_expectation(orc, t2ref, planes, f, True, True)
        want_pix = orc.create_image([p for p in want], prec)
        d_pix = torch.from_numpy(pix).to(plan.device)
        cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA8, d_pix, sop=True, eph=True)
        plan.frame_status()
        back = torch.zeros_like(d_pix)
        plan.decode_frame_pixels(cs, int(cs.numel()), back, tile_offs=toffs, sop=True, eph=True)      # warm-up, option off
        plan.frame_status()
        plain = back.cpu().numpy().copy()
        assert not np.array_equal(plain, want_pix)
        plan.set_dequantize(True)
        with ctx.capture() as g:
            plan.decode_frame_pixels(cs, int(cs.numel()), back, tile_offs=toffs, sop=True, eph=True)
        for _ in range(2):
            back.zero_()
            torch.cuda.synchronize()
            g.launch()
            ctx.sync()
            assert np.array_equal(back.cpu().numpy(), want_pix)
        plan.set_dequantize(False)           # later calls change; the graph keeps what it recorded
        back.zero_()
        torch.cuda.synchronize()
        g.launch()
        ctx.sync()
        assert np.array_equal(back.cpu().numpy(), want_pix)
        plan.decode_frame_pixels(cs, int(cs.numel()), back, tile_offs=toffs, sop=True, eph=True)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), plain)
        g.close()
    finally:
        plan.close()
        ctx.close()


# ---- unit calls ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", dq.UNIT_STEPS)
def test_unit_calls(env, step):
    torch, orc, t2ref, ctx = env
    from j2kgfx import dwt
    for n in dq.UNIT_LENGTHS:
        x = dq.quantize_input(n, step, 1)
        got = dwt.quantize(x, step, ctx=ctx)
        assert got.dtype == np.int32 and got.shape == (n,)
        assert np.array_equal(got, dq.quantize_ref(x, step)), n
        y = dq.dequantize_input(n, 2)
        d = dwt.dequantize(y, step, ctx=ctx)
        assert d.dtype == np.float64 and d.shape == (n,)
        assert lc.same_floats(d, dq.dequantize_ref(y, step)), n
    # a quantised plane and back, as the two compose in the reference
    x = np.random.default_rng(9).uniform(-500, 500, 4099)
    qv = dwt.quantize(x, step, ctx=ctx)
    assert lc.same_floats(dwt.dequantize(qv, step, ctx=ctx), dq.dequantize_ref(dq.quantize_ref(x, step), step))
