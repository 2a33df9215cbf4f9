"""GPU: plans made with is_signed=True against the definition of tests/signed_cases.py, bit for bit (np.array_equal everywhere; no tolerance).
A signed plan skips the inverse DC level shift (PlanSpec::dc_shift_inv = 0, decoder.go:344-348) and nothing else: the forward path, and so the
encoded bytes, are the unsigned plan's; every inverse form must add 0 where the unsigned plan adds 2^(prec - 1); decoder.createImage clamps the
negatives to 0; the packed-pixel kernels of level 0 have the unsigned shift built in, so a signed plan stages its pixels through the int32 frame
and j2k_pack_pixels on the way out (pix_fusable) and j2k_plan_inverse_rgba8 refuses it.

  a  int32 frames          test_int32_frames_53 / _97: forward == the unsigned expectation, inverse == the signed one, on the smallest case behind every
                           inverse form label of lossless53_cases.forms() and every workgroup width of the 9-7 inverse (tests/test_signed_cases.py
                           checks that no label is missing)
  b  reduced decode        test_mallat_frames: reduce = 0 ... levels on 130 x 70 in 64 x 64 tiles, both wavelets (levels: mallat_ll_kernel alone)
  c  packed pixels         test_packed_pixels / test_packed_pixels_97 / test_inverse_rgba8_refuses_a_signed_plan
  d  frame calls           test_frame_calls: encode bytes == the unsigned plan's == the oracle's; decode_frame_pixels and decode_pixels_host plain,
                           skip_planes=2, area=, reduce=1, a frame_rows batch of two, two shards writing one frame
  e  captured decode       test_captured_decode      f  host pipe   test_host_pipe      g  two plans on one context   test_signed_and_unsigned_plans_alternate

Each test can fail.  Six scratch builds, one changed line of csrc/j2k_stages.cpp each (S.dc_shift in the place of S.dc_shift_inv, or pix_fusable
without its `inverse ?` choice), this file run once against each (81 cases):
  the 5-3 level-0 launch            59 red: all of test_int32_frames_53, test_mallat_frames[*-53-*], test_packed_pixels, test_frame_calls[mq_rgba8 |
                                    ht_gray8 | mallat_mq_gray16], test_captured_decode, test_host_pipe, test_signed_and_unsigned_plans_alternate
  the 9-7 level-0 launch            21 red: all of test_int32_frames_97, test_mallat_frames[*-97*], test_packed_pixels_97, test_frame_calls[lossy_dq_rgba8]
  launch_mallat_ll                   4 red: test_mallat_frames (reduce = levels)
  reduced decode, 5-3 final launch   3 red: test_mallat_frames[*-53-*], test_frame_calls[mallat_mq_gray16] (reduce=1)
  reduced decode, 9-7 final launch   2 red: test_mallat_frames[*-97*]
  pix_fusable                       27 red: every test_packed_pixels case whose unsigned inverse is fused (24 of 28), test_packed_pixels_97 (3)"""
import os

import numpy as np
import pytest

import closed_loop_ref as ref
import lossless53_cases as ll
import lossy97_cases as l9
import mallat_cases as mc
import signed_cases as sc

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A
PAD = 12                    # bytes after every output row of the pixel tests: stride = row + 12


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
def t2ref():
    import t2ref as t
    return t


def _plan53(case, ctx, is_signed=True):
    from j2kgfx.codec import FramePlan
    return FramePlan(case.W, case.H, case.C, ctx=ctx, precision=case.prec, lossless=True, num_resolutions=case.nres, cb=(64, 64), tile=case.tile, coder=1,
                     is_signed=is_signed)


def _tiles(plan):
    """[(tile, x0, y0, w, h, {component: coefficient offset})]"""
    rows = plan.planes()
    out = []
    for t in np.unique(rows[:, 0]):
        sel = rows[rows[:, 0] == t]
        x0, y0, w, h = (int(v) for v in sel[0, 2:6])
        out.append((int(t), x0, y0, w, h, {int(r[1]): int(r[6]) for r in sel}))
    return out


def _dev(plan, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(plan.device)


def _check_forward(plan, hc, expect_tile, what):
    """the device's coefficients == expect_tile(x0, y0, w, h) [C, h, w], per tile and component"""
    for t, x0, y0, w, h, offs in _tiles(plan):
        want = expect_tile(x0, y0, w, h)
        for c, off in offs.items():
            assert np.array_equal(hc[off:off + w * h].reshape(h, w), want[c]), (what, "tile", t, "component", c)


def _fill(plan, C, H, W, coeff_tile, expect_tile):
    """(the plan's flat coefficient buffer from coeff_tile(x0, y0, w, h) [C, h, w], the frame expect_tile(coefficients) [C, h, w] makes of it)"""
    buf = np.zeros(max(int(plan.info.coeff_elems), 4), np.int32)
    want = np.zeros((C, H, W), np.int32)
    for t, x0, y0, w, h, offs in _tiles(plan):
        co = np.asarray(coeff_tile(x0, y0, w, h))
        for c, off in offs.items():
            buf[off:off + w * h] = co[c].reshape(-1)
        want[:, y0:y0 + h, x0:x0 + w] = expect_tile(co)
    return buf, want


def _padded(plan, H, stride):
    import torch
    return torch.full((H, stride), SENTINEL, dtype=torch.uint8, device=plan.device)


def _check_pixels(out, want_pix, what):
    o = out.cpu().numpy()
    row = want_pix.shape[1]
    assert np.array_equal(o[:, :row], want_pix), what
    assert (o[:, row:] == SENTINEL).all(), (what, "row padding written")


# ---- a. int32 frames ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.cases_53(), ids=lambda c: c.id)
def test_int32_frames_53(oracle, ctx_for, case):
    """j2k_plan_forward / j2k_plan_inverse of a signed 5-3 plan on the smallest case of every inverse form: marching <2 | 4 | 8, 1 | 3, vec | scalar>,
    plane workgroup 4 / 8 waves single / multi strip, the LDS tail, the deep launch with J2K_DEEP_MID_INV 0 / 1 / 2, four components"""
    plan = _plan53(case, ctx_for(**dict(case.env)))
    seam = ll.seams(case.route)
    try:
        for family in ("noise", "impulse"):
            frame = ll.int_frame(family, case.W, case.H, case.C, case.prec, 1, case.tile, seam)
            coeff = plan.forward(_dev(plan, frame))
            plan.ctx.sync()
            _check_forward(plan, coeff.cpu().numpy(), lambda x0, y0, w, h: sc.expect_forward53(oracle, frame[:, y0:y0 + h, x0:x0 + w], case.prec, case.nres), family)
        for family in sc.COEFF_FAMILIES_53:
            def coeff_tile(x0, y0, w, h):
                cols, rows = seam.get((x0, y0), ((), ()))
                return np.stack([ll.coeff_plane(family, w, h, 3 * (x0 + y0) + c, cols, rows) for c in range(case.C)])
            buf, want = _fill(plan, case.C, case.H, case.W, coeff_tile, lambda co: sc.expect_inverse53(oracle, co, case.prec, case.nres))
            back = plan.inverse(_dev(plan, buf))
            plan.ctx.sync()
            assert np.array_equal(back.cpu().numpy(), want), (case.id, "inverse", family)
    finally:
        plan.close()


@pytest.mark.parametrize("case", sc.cases_97(), ids=lambda c: c.id)
def test_int32_frames_97(oracle, ctx_for, case):
    """the general kernel and every workgroup width of the 9-7 level-0 inverse (J2K_L0_WG97_INV), Quality 75 and 1, with and without the
    dequantiser in the kernels' loads"""
    from j2kgfx.codec import FramePlan
    nrs = (case.nw - 3, l9.defaults()["band_prows_97"])
    plan = FramePlan(case.W, case.H, 3, ctx=ctx_for(J2K_L0_WG97_INV=case.nw), precision=case.prec, lossless=False, quality=case.quality, num_resolutions=case.nres,
                     cb=(64, 64), tile=case.tile, coder=0, is_signed=True, dequantize=case.dequantize)
    try:
        frame = l9.int_frame("noise", case.W, case.H, 3, case.prec, 1, nrs)
        coeff = plan.forward(_dev(plan, frame))
        plan.ctx.sync()
        _check_forward(plan, coeff.cpu().numpy(), lambda x0, y0, w, h: np.stack(oracle.preprocess(
            [np.ascontiguousarray(frame[c, y0:y0 + h, x0:x0 + w]) for c in range(3)], w, h, case.prec, False, case.nres, case.quality)), "forward")
        for family in case.families:
            buf, want = _fill(plan, 3, case.H, case.W, lambda x0, y0, w, h: np.stack([l9.coeff_plane(family, w, h, 3 * (x0 + y0) + c, nrs) for c in range(3)]),
                              lambda co: sc.expect_inverse97(oracle, co, case.prec, case.nres, case.quality, case.dequantize))
            back = plan.inverse(_dev(plan, buf))
            plan.ctx.sync()
            assert np.array_equal(back.cpu().numpy(), want), (case.id, "inverse", family)
    finally:
        plan.close()


# ---- b. Mallat plans and the reduced decode --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", sc.MALLAT, ids=sc.mallat_id)
def test_mallat_frames(oracle, ctx_for, m):
    """plan.inverse(coeff, reduce=r), r = 0 ... levels, and inverse_pixels(reduce=r) into padded rows: the final launch of a reduced decode for both
    wavelets, and mallat_ll_kernel when no level runs"""
    import torch
    from j2kgfx.codec import FramePlan
    W, H, Cn, prec, tile, nres, lossless, quality, deq = m
    levels = mc.levels_of(nres)
    plan = FramePlan(W, H, Cn, ctx=ctx_for(), precision=prec, lossless=lossless, quality=quality, num_resolutions=nres, cb=(64, 64), tile=tile, coder=0,
                     mallat=True, is_signed=True, dequantize=deq)
    try:
        frame = sc.uniform_frame(W, H, Cn, prec, 4)
        fwd = mc.flat_coeff(plan.planes(), mc.forward_frame(oracle, frame, tile, prec, nres, lossless, quality), int(plan.info.coeff_elems))
        coeff = plan.forward(_dev(plan, frame), plan.alloc_coeff().zero_())
        plan.ctx.sync()
        assert np.array_equal(coeff.cpu().numpy()[:fwd.size], fwd)
        for family in ("noise", "signedrange") + (("fullrange",) if lossless else ()):
            tiles = sc.mallat_tiles(m, family)
            d_coeff = _dev(plan, mc.flat_coeff(plan.planes(), tiles, max(int(plan.info.coeff_elems), 4)))
            for r in range(levels + 1):
                want = sc.mallat_frame(oracle, m, tiles, r)
                if r == 0:
                    got = plan.inverse(d_coeff)
                else:
                    got = torch.full((Cn,) + want.shape[1:], -77, dtype=torch.int32, device=plan.device)
                    plan.inverse(d_coeff, got, reduce=r)
                plan.ctx.sync()
                assert np.array_equal(got.cpu().numpy(), want), (family, r)
                if (Cn, prec) not in mc.PIX_FORMAT or family == "fullrange":
                    continue
                want_pix = sc.pixels(oracle, want, prec)
                out = _padded(plan, want.shape[1], want_pix.shape[1] + PAD)
                assert not plan.pixels_fused(mc.PIX_FORMAT[(Cn, prec)], out, inverse=True)
                plan.inverse_pixels(d_coeff, out, reduce=r)
                plan.ctx.sync()
                _check_pixels(out, want_pix, (family, r, "pixels"))
    finally:
        plan.close()


# ---- c. packed pixels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.pixel_cases(), ids=lambda c: c.id)
def test_packed_pixels(oracle, ctx_for, case):
    """the six formats on the cases where an UNSIGNED plan's inverse writes the pixels in a level-0 kernel (RGBA8 workgroup and merged launch, plane
    workgroup for Gray8 / Gray16 / NRGBA / RGBA64, the pixel-writing marching kernels): the way in is the unsigned plan's, the way out is never
    fused and gives createImage of the signed planes -- at the case's own 16-byte stride, where the unsigned plan fuses, and at row + 12"""
    ctx = ctx_for(**dict(case.env))
    splan, uplan = _plan53(case, ctx), _plan53(case, ctx, is_signed=False)
    R = case.route
    seam = ll.seams(R)
    fmt, W, H, C, prec = case.fmt, case.W, case.H, case.C, case.prec
    bps, ch = ll.PIX_BPS[fmt], 1 if C == 1 else 4
    row = W * ch * (2 if prec > 8 else 1)
    try:
        probe = _padded(splan, H, case.stride)
        fused_in = ll.pix_fusable(R, bps, ch, case.stride, False, prec) is not None
        assert splan.pixels_fused(fmt, probe) == uplan.pixels_fused(fmt, probe) == fused_in, case.id
        fused_out = ll.pix_fusable(R, bps, ch, case.out_stride, True, prec) is not None
        assert fused_out == bool(sc.pixel_inverse_routes(case))
        frame = ll.int_frame("noise", W, H, 4, prec, 2, case.tile, seam)
        pix = ll.pack_pixels(fmt, frame, case.stride)
        coeff = splan.forward_pixels(fmt, _dev(splan, pix))
        splan.ctx.sync()
        planes = np.stack(oracle.extract_image_data(pix, fmt, W, H, prec))
        _check_forward(splan, coeff.cpu().numpy(), lambda x0, y0, w, h: sc.expect_forward53(oracle, planes[:, y0:y0 + h, x0:x0 + w], prec, case.nres), "forward_pixels")
        for family in ("signedrange", "fullrange"):
            def coeff_tile(x0, y0, w, h):
                if family == "signedrange":
                    return sc.signedrange_set(w, h, C, prec, case.nres, x0 + y0)[0]
                cols, rows = seam.get((x0, y0), ((), ()))
                return np.stack([ll.coeff_plane(family, w, h, 3 * (x0 + y0) + c, cols, rows) for c in range(C)])
            buf, want = _fill(splan, C, H, W, coeff_tile, lambda co: sc.expect_inverse53(oracle, co, prec, case.nres))
            if family == "signedrange":
                clamped, inside = sc.clamp_shares(want, prec)
                assert clamped >= sc.SIGNEDRANGE_MIN_SHARE and inside >= sc.SIGNEDRANGE_MIN_SHARE, (clamped, inside)
            want_pix = sc.pixels(oracle, want, prec)
            assert want_pix.shape == (H, row)
            dbuf = _dev(splan, buf)
            for stride in dict.fromkeys((case.out_stride, row + PAD)):
                out = _padded(splan, H, stride)
                splan.inverse_pixels(dbuf, out)
                splan.ctx.sync()
                _check_pixels(out, want_pix, (case.id, family, stride))
        # (asked last, so that a signed plan that did fuse shows in its pixels first)
        oprobe = _padded(splan, H, case.out_stride)
        assert uplan.pixels_fused(fmt, oprobe, inverse=True) == fused_out, case.id           # the unsigned plan takes the route that labels the case ...
        assert splan.pixels_fused(fmt, oprobe, inverse=True) is False, case.id               # ... and the signed plan never does
    finally:
        splan.close()
        uplan.close()


@pytest.mark.parametrize("W,H,tile,nres", sc.pixel_cases_97())
def test_packed_pixels_97(oracle, ctx_for, W, H, tile, nres):
    """RGB at 8 bit, Quality 75, dequantised: the unsigned plan's 9-7 workgroup inverse writes RGBA8 pixels itself, the signed plan stages them"""
    from j2kgfx.codec import FramePlan
    ctx = ctx_for()
    kw = dict(ctx=ctx, precision=8, lossless=False, quality=75, num_resolutions=nres, cb=(64, 64), tile=tile, coder=0, dequantize=True)
    splan, uplan = FramePlan(W, H, 3, is_signed=True, **kw), FramePlan(W, H, 3, **kw)
    nrs = (l9.defaults()["l0_wg97_inv"] - 3, l9.defaults()["band_prows_97"])
    try:
        probe = _padded(splan, H, W * 4)
        assert splan.pixels_fused(2, probe) == uplan.pixels_fused(2, probe)
        frame = l9.int_frame("noise", W, H, 4, 8, 3)
        pix = np.ascontiguousarray(frame.transpose(1, 2, 0).astype(np.uint8).reshape(H, W * 4))
        coeff = splan.forward_pixels(2, _dev(splan, pix))
        splan.ctx.sync()
        _check_forward(splan, coeff.cpu().numpy(), lambda x0, y0, w, h: np.stack(oracle.preprocess(
            [np.ascontiguousarray(frame[c, y0:y0 + h, x0:x0 + w]) for c in range(3)], w, h, 8, False, nres, 75)), "forward_pixels")
        for family in ("signedrange", "noise"):
            def coeff_tile(x0, y0, w, h):
                if family == "signedrange":
                    return sc.signedrange_set(w, h, 3, 8, nres, x0 + y0, lossless=False, quality=75)[0]
                return np.stack([l9.coeff_plane(family, w, h, 3 * (x0 + y0) + c, nrs) for c in range(3)])
            buf, want = _fill(splan, 3, H, W, coeff_tile, lambda co: sc.expect_inverse97(oracle, co, 8, nres, 75, True))
            if family == "signedrange":
                clamped, inside = sc.clamp_shares(want, 8)
                assert clamped >= sc.SIGNEDRANGE_MIN_SHARE and inside >= sc.SIGNEDRANGE_MIN_SHARE, (clamped, inside)
            want_pix = sc.pixels(oracle, want, 8)
            dbuf = _dev(splan, buf)
            for stride in (W * 4, W * 4 + PAD):
                out = _padded(splan, H, stride)
                splan.inverse_pixels(dbuf, out)
                splan.ctx.sync()
                _check_pixels(out, want_pix, (family, stride))
        assert uplan.pixels_fused(2, probe, inverse=True) and not splan.pixels_fused(2, probe, inverse=True)
    finally:
        splan.close()
        uplan.close()


def test_inverse_rgba8_refuses_a_signed_plan(oracle, ctx_for):
    """j2k_plan_inverse_rgba8 on a signed 8-bit plan: J2K_ERR_UNSUPPORTED, the output untouched; forward_rgba8 is the unsigned plan's"""
    import torch
    from j2kgfx import J2KError, _lib
    case = next(c for c in sc.pixel_cases() if any(f.startswith("rgba8_wg_inv") for f, _ in sc.pixel_inverse_routes(c)) and not c.env)
    splan, uplan = _plan53(case, ctx_for()), _plan53(case, ctx_for(), is_signed=False)
    try:
        frame = ll.int_frame("noise", case.W, case.H, 4, 8, 5, case.tile)
        pix = _dev(splan, ll.pack_pixels(2, frame, case.stride))
        a, b = splan.forward_rgba8(pix), uplan.forward_rgba8(pix)
        splan.ctx.sync()
        assert torch.equal(a, b)
        out = _padded(splan, case.H, case.out_stride)
        with pytest.raises(J2KError) as e:
            splan.inverse_rgba8(a, out)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        splan.ctx.sync()
        assert (out.cpu().numpy() == SENTINEL).all()
        uplan.inverse_rgba8(b, out)
        uplan.ctx.sync()
        assert np.array_equal(out.cpu().numpy()[:, :case.W * 4], oracle.create_image([frame[c] for c in range(3)], 8))     # (lossless: the source comes back)
    finally:
        splan.close()
        uplan.close()


# ---- d. the frame calls ----------------------------------------------------------------------------------------------------------------------------
class _FrameEnv:
    """one plan kind of signed_cases.FRAME_PLANS: its plans, two source frames, the oracle's streams and the definition's pixels"""

    def __init__(self, name, oracle, t2ref, ctx):
        self.name, self.orc, self.t2ref, self.ctx = name, oracle, t2ref, ctx
        self.Cn, self.prec, self.fmt, self.bpp, self.marks, self.cb, self.kw = sc.FRAME_PLANS[name]
        self.W, self.H, self.tile, self.nres = sc.FRAME_W, sc.FRAME_H, sc.FRAME_TILE, sc.FRAME_NRES
        self.mallat, self.lossless, self.coder = bool(self.kw.get("mallat")), self.kw["lossless"], self.kw["coder"]
        self.quality, self.deq = self.kw.get("quality", 0), bool(self.kw.get("dequantize"))
        self.frames = []
        for seed in (11, 12):
            pix, Cn, prec, planes = ref.pixel_frame(self.fmt, self.W, self.H, seed + 10 * len(name), oracle)
            assert (Cn, prec) == (self.Cn, self.prec)
            of = mc.oracle_frame if self.mallat else ref.oracle_frame
            want = of(planes, self.W, self.H, self.tile[0], self.tile[1], self.nres, self.cb, self.coder, self.marks, self.marks, oracle, t2ref,
                      precision=self.prec, lossless=self.lossless, quality=self.quality)
            self.frames.append(dict(pix=pix, planes=planes, want=want, stream=np.frombuffer(b"".join(want[t]["part"] for t in sorted(want)), np.uint8).copy()))

    def make(self, H=None, **extra):
        from j2kgfx.codec import FramePlan
        return FramePlan(self.W, H or self.H, self.Cn, precision=self.prec, num_resolutions=self.nres, cb=(self.cb, self.cb), tile=self.tile, ctx=self.ctx,
                         **dict(self.kw, **extra))

    def expect(self, i, reduce=0, skip_planes=0, area=None, is_signed=True, only=None, fill=0):
        """the definition's pixels of frame i: uint8 [h, w * bpp]"""
        tiles = sc.decoded_tiles(self.orc, self.frames[i]["want"], self.Cn, self.nres, self.cb, self.coder, skip_planes)
        frame = sc.closed_loop_frame(self.orc, tiles, self.W, self.H, self.tile, self.prec, self.nres, self.lossless, self.quality, self.deq, self.mallat, reduce,
                                     only=only, fill=fill, is_signed=is_signed)
        full = sc.pixels(self.orc, frame, self.prec)
        return full if area is None else sc.crop(full, area, reduce, self.bpp)

    def variants(self):
        out = [dict()]
        if self.coder == 0:
            out.append(dict(skip_planes=2))
        if self.mallat:
            out += [dict(area=sc.FRAME_AREA), dict(reduce=1), dict(reduce=mc.levels_of(self.nres)), dict(reduce=1, skip_planes=2, area=sc.FRAME_AREA)]
        return out


def _encode(plan, fmt, d_pix, marks):
    cs, toffs = plan.encode_frame_pixels(fmt, d_pix, sop=marks, eph=marks)
    plan.frame_status()
    h_t = toffs.cpu().numpy().astype(np.int64)
    return cs, toffs, h_t, cs.cpu().numpy()[:int(h_t[-1])]


@pytest.mark.parametrize("name", list(sc.FRAME_PLANS))
def test_frame_calls(oracle, t2ref, ctx_for, name):
    """200 x 72 in 64 x 64 tiles, closed loop: MQ RGBA8, HT Gray8, Mallat MQ Gray16, lossy 9-7 dequantised RGBA8"""
    import torch
    E = _FrameEnv(name, oracle, t2ref, ctx_for())
    W, H, fmt, marks, bpp = E.W, E.H, E.fmt, E.marks, E.bpp
    splan, uplan = E.make(is_signed=True), E.make()
    plans = [splan, uplan]
    try:
        f0 = E.frames[0]
        d_pix = _dev(splan, f0["pix"])
        cs, toffs, h_t, h_cs = _encode(splan, fmt, d_pix, marks)
        _, _, u_t, u_cs = _encode(uplan, fmt, d_pix, marks)
        assert np.array_equal(h_t, u_t) and np.array_equal(h_cs, u_cs) and np.array_equal(h_cs, f0["stream"])
        assert np.array_equal(splan.encode_pixels_host(fmt, f0["pix"], sop=marks, eph=marks)["bytes"], h_cs)
        total = int(h_t[-1])
        # the signed definition is not the unsigned one, and the unsigned plan still gives the unsigned one
        assert not np.array_equal(E.expect(0), E.expect(0, is_signed=False))
        back = torch.full((H, W * bpp), SENTINEL, dtype=torch.uint8, device=uplan.device)
        uplan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=marks, eph=marks)
        uplan.frame_status()
        assert np.array_equal(back.cpu().numpy(), E.expect(0, is_signed=False))
        for v in E.variants():
            exp = E.expect(0, **v)
            back = torch.full(exp.shape, SENTINEL, dtype=torch.uint8, device=splan.device)
            splan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=marks, eph=marks, **v)
            splan.frame_status()
            assert np.array_equal(back.cpu().numpy(), exp), ("decode_frame_pixels", v)
            assert np.array_equal(splan.decode_pixels_host(h_cs, exp.shape, sop=marks, eph=marks, **v), exp), ("decode_pixels_host", v)
        # a batch of two frames (frame_rows)
        batch, ubatch = E.make(H=2 * H, frame_rows=H, is_signed=True), E.make(H=2 * H, frame_rows=H)
        plans += [batch, ubatch]
        pix2 = np.concatenate([f["pix"] for f in E.frames])
        bcs, btoffs, b_t, b_cs = _encode(batch, fmt, _dev(batch, pix2), marks)
        assert np.array_equal(b_cs, _encode(ubatch, fmt, _dev(ubatch, pix2), marks)[3])
        exp2 = np.concatenate([E.expect(0), E.expect(1)])
        back = torch.full(exp2.shape, SENTINEL, dtype=torch.uint8, device=batch.device)
        batch.decode_frame_pixels(bcs, int(b_t[-1]), back, tile_offs=btoffs, sop=marks, eph=marks)
        batch.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp2), "batch"
        assert np.array_equal(batch.decode_pixels_host(b_cs, exp2.shape, sop=marks, eph=marks), exp2), "batch, host"
        # two shards write one frame
        back = torch.full((H, W * bpp), SENTINEL, dtype=torch.uint8, device=splan.device)
        rects = mc.tiles_of(W, H, E.tile)
        assert sum(n for _, n in sc.FRAME_SHARDS) == len(rects)
        for first, count in sc.FRAME_SHARDS:
            shard = E.make(is_signed=True, tile_first=first, tile_count=count)
            plans.append(shard)
            scs, stoffs, s_t, s_cs = _encode(shard, fmt, d_pix, marks)
            assert np.array_equal(s_cs, h_cs[h_t[first]:h_t[first + count]]), ("shard bytes", first)
            shard.decode_frame_pixels(scs, int(s_t[-1]), back, tile_offs=stoffs, sop=marks, eph=marks)
            shard.frame_status()
            part = E.expect(0, only=range(first, first + count), fill=0)
            host = shard.decode_pixels_host(s_cs, (H, W * bpp), sop=marks, eph=marks)
            for x0, y0, w, h in rects[first:first + count]:
                assert np.array_equal(host[y0:y0 + h, bpp * x0:bpp * (x0 + w)], part[y0:y0 + h, bpp * x0:bpp * (x0 + w)]), ("shard, host", first)
        assert np.array_equal(back.cpu().numpy(), E.expect(0)), "two shards"
    finally:
        for p in plans:
            p.close()


# ---- e. a captured decode ----------------------------------------------------------------------------------------------------------------------------
def test_captured_decode(oracle, t2ref):
    """decode_frame_pixels of the signed MQ plan captured once, replayed on a second stream of the same geometry"""
    import torch
    from j2kgfx import Context
    ctx = Context(0)
    E = _FrameEnv("mq_rgba8", oracle, t2ref, ctx)
    plan = E.make(is_signed=True)
    try:
        streams = []
        for f in E.frames:
            cs, toffs = plan.encode_frame_pixels(E.fmt, _dev(plan, f["pix"]), sop=True, eph=True)
            plan.frame_status()
            streams.append((cs.clone(), toffs.clone()))
        exp = [E.expect(0), E.expect(1)]
        assert not np.array_equal(exp[0], exp[1])
        cs, toffs = streams[0][0].clone(), streams[0][1].clone()
        back = torch.zeros((E.H, E.W * E.bpp), dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, int(cs.numel()), back, tile_offs=toffs, sop=True, eph=True)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp[0])
        with ctx.capture() as g:
            plan.decode_frame_pixels(cs, int(cs.numel()), back, tile_offs=toffs, sop=True, eph=True)
        for k in (1, 0):
            cs.copy_(streams[k][0])
            toffs.copy_(streams[k][1])
            back.fill_(SENTINEL)
            torch.cuda.synchronize()
            g.launch()
            ctx.sync()
            assert np.array_equal(back.cpu().numpy(), exp[k]), k
        g.close()
    finally:
        plan.close()
        ctx.close()


# ---- f. the host pipe ----------------------------------------------------------------------------------------------------------------------------------
POISON, GUARD = 0xA5, 64


def _guarded(codec, nbytes, pinned, offset=0):
    """(the whole poisoned buffer, the window of nbytes at GUARD + offset inside it)"""
    n = nbytes + 2 * GUARD + offset
    buf = codec.pinned_empty(n) if pinned else np.empty(n, np.uint8)
    buf[:] = POISON
    return buf, buf[GUARD + offset:GUARD + offset + nbytes]


def test_host_pipe(oracle, t2ref, ctx_for):
    """HostPipe(depth=2) on the signed MQ plan into a pinned frame (the pack kernel stores through the device address), a pinned frame 2 bytes into
    its allocation (staged) and pageable memory, guards poisoned: == decode_pixels_host on a second plan == the definition"""
    from j2kgfx import codec
    E = _FrameEnv("mq_rgba8", oracle, t2ref, ctx_for())
    plan, second = E.make(is_signed=True), E.make(is_signed=True)
    row, n = E.W * E.bpp, E.H * E.W * E.bpp
    try:
        want = []
        for i, f in enumerate(E.frames):
            host = second.decode_pixels_host(f["stream"], (E.H, row), sop=True, eph=True)
            assert np.array_equal(host, E.expect(i))
            want.append(host)
        with codec.HostPipe(plan, depth=2) as pipe:
            enc = pipe.wait(pipe.submit_encode(E.fmt, E.frames[0]["pix"], sop=True, eph=True))
            assert np.array_equal(enc["bytes"], E.frames[0]["stream"])
            flight = []

            def finish(item):
                t, buf, off, pix, i = item
                assert pipe.wait(t) is pix
                assert np.array_equal(pix, want[i]), (off, i)
                assert np.all(buf[:GUARD + off] == POISON) and np.all(buf[GUARD + off + n:] == POISON), (off, i)
            for k, (pinned, off) in enumerate([(True, 0), (True, 2), (False, 0), (True, 0), (False, 0)]):
                buf, win = _guarded(codec, n, pinned, off)
                pix = win.reshape(E.H, row)
                if len(flight) == 2:
                    finish(flight.pop(0))
                flight.append((pipe.submit_decode(E.frames[k % 2]["stream"], pix, sop=True, eph=True), buf, off, pix, k % 2))
            while flight:
                finish(flight.pop(0))
    finally:
        plan.close()
        second.close()


# ---- g. two plans on one context -------------------------------------------------------------------------------------------------------------------------
def test_signed_and_unsigned_plans_alternate(oracle, t2ref, ctx_for):
    """a signed and an unsigned plan of equal parameters on one context, used in turn: each keeps its own result (plans, tables and cached unit
    plans are keyed with dc_shift_inv)"""
    import torch
    case = next(c for c in sc.cases_53() if c.C == 3 and not c.tile[0] and "march<cpl8,nc3,vec>" in sc.inverse_labels(c))
    ctx = ctx_for(**dict(case.env))
    plans = {True: _plan53(case, ctx), False: _plan53(case, ctx, is_signed=False)}
    E = _FrameEnv("mq_rgba8", oracle, t2ref, ctx)
    frames = {True: E.make(is_signed=True), False: E.make()}
    try:
        co = np.stack([ll.coeff_plane("noise", case.W, case.H, c) for c in range(case.C)])
        buf, _ = _fill(plans[True], case.C, case.H, case.W, lambda *a: co, lambda c_: 0)
        dbuf = _dev(plans[True], buf)
        want = {s: ll.expect_inverse(oracle, co, case.prec, case.nres, is_signed=s) for s in (True, False)}
        stream = _dev(frames[True], E.frames[0]["stream"])
        exp = {s: E.expect(0, is_signed=s) for s in (True, False)}
        for s in (True, False, True, False, False, True):
            back = plans[s].inverse(dbuf)
            ctx.sync()
            assert np.array_equal(back.cpu().numpy(), want[s]), ("plan.inverse", s)
            pix = torch.full(exp[s].shape, SENTINEL, dtype=torch.uint8, device=frames[s].device)
            frames[s].decode_frame_pixels(stream, int(stream.numel()), pix, sop=True, eph=True)
            frames[s].frame_status()
            assert np.array_equal(pix.cpu().numpy(), exp[s]), ("decode_frame_pixels", s)
            assert np.array_equal(frames[s].decode_pixels_host(E.frames[0]["stream"], exp[s].shape, sop=True, eph=True), exp[s]), ("decode_pixels_host", s)
    finally:
        for p in list(plans.values()) + list(frames.values()):
            p.close()
