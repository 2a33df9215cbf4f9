"""GPU: the raw-MagRef coding style (j2k_plan_set_raw_magref, FramePlan(raw_magref=True)) against its definition, tests/raw_magref_cases.py
(checked on the CPU by tests/test_raw_magref_cases.py).  Every comparison is bit for bit.

  blocks          bodies, lens, numbps and decoded samples of every shape x band x content, through every encoder form built for the style
                  (one kernel; split + MQ lanes + pack; lane groups of 64; lists too short for the deep blocks, which then take the one-kernel
                  form) and every decoder form: the one-launch kernel (default, t1_dec_general), the plane-stepped lanes path as launches
                  per plane (t1_dec_lanes = 1, and 0, which the style maps to it) and as one launch per group (t1_dec_lanes = 2)
  foreign bodies  random byte strings as bodies: the device follows the total-function rules, and reads nothing outside offs + lens
  skip_planes     = coarse(full decode, k)
  frames          tile-parts byte for byte (bare and SOP + EPH), pixels back, reduce / area / area + skip_planes, host forms, a captured
                  replay, the style switched on and off between frames, the golden digests
  refusals        before anything is launched, outputs untouched"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import coarse_cases as cc
import mallat_cases as mc
import raw_magref_cases as rm

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5

ENC_FORMS = {
    "one_kernel": dict(t1_split=0),
    "split": dict(t1_split=1),
    "split_k64": dict(t1_split=1, t1_lanes=64),
    "split_k3": dict(t1_split=1, t1_lanes=3),
    "split_short_lists": dict(t1_split=1, t1_sym_mb=1),       # lists of 8 planes: deeper blocks are left to the one-kernel form
}
DEC_FORMS = {
    "default": {},
    "dec_split_lanes": dict(t1_dec_split=1, t1_dec_lanes=1),
    "dec_split_persist": dict(t1_dec_split=1, t1_dec_lanes=2),
    "dec_split_steps": dict(t1_dec_split=1, t1_dec_lanes=0),
    "dec_general": dict(t1_dec_general=1),
}
LANES_FORMS = ("default", "dec_split_lanes", "dec_split_persist")      # the one-launch kernel and both forms of the lanes path
# tiles per shape: 6 contents x 4 bands at least; 4 x 4 and 33 x 17 with job counts above 64 that are no multiple of 64 (68, 108)
TILES = {(1, 1): (6, 1), (1, 64): (6, 1), (64, 1): (3, 2), (3, 5): (3, 2), (4, 4): (17, 1), (33, 17): (9, 3), (64, 64): (3, 2)}


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    import t2ref
    return torch, oracle, t2ref


def _ctx(opts):
    from j2kgfx import Context
    ctx = Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def _dev(torch, plan, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(plan.device)


def _status(fn):
    from j2kgfx import J2KError
    try:
        fn()
    except J2KError as e:
        return e.status
    return 0


# ---- blocks ---------------------------------------------------------------------------------------------------------------------------------
def _block_plan(ctx, shape, raw=True):
    """a Mallat plan whose every tile is one block of `shape` per band: 2w x 2h tiles, two resolutions, one component"""
    from j2kgfx.codec import FramePlan
    (w, h), (tx, ty) = shape, TILES[shape]
    return FramePlan(2 * w * tx, 2 * h * ty, 1, precision=8, lossless=True, num_resolutions=2, cb=(64, 64), tile=(2 * w, 2 * h), coder=0, ctx=ctx, mallat=True,
                     raw_magref=raw)


_families = {}


def _family(plan, shape, orc):
    """per job of the plan: (w, h, band, data, body, numbps) by the definition, and the flat coefficient buffer holding the data; made once"""
    if shape not in _families:
        blocks, planes = plan.blocks(), plan.planes()
        coeff = np.zeros(max(int(plan.info.coeff_elems), 4), np.int32)
        jobs = []
        for j, b in enumerate(blocks):
            w, h, band = int(b["w"]), int(b["h"]), int(b["band"])
            assert (w, h) == shape
            t, _c, _x, _y, pw, ph, off = (int(v) for v in planes[int(b["plane"])])
            kind = rm.CONTENTS[t % len(rm.CONTENTS)]
            data = rm.block_content(kind, w, h, seed=j)
            view = coeff[off:off + pw * ph].reshape(ph, pw)
            view[int(b["y0"]):int(b["y0"]) + h, int(b["x0"]):int(b["x0"]) + w] = data
            body, nb = rm.encode_block(data, w, h, band, orc)
            jobs.append((w, h, band, data, body, nb))
        assert sorted({j[2] for j in jobs}) == [0, 1, 2, 3]
        _families[shape] = (jobs, coeff)
    return _families[shape]


def _check_bodies(jobs, h_stream, h_offs, h_lens, h_nb):
    for j, (w, h, band, data, body, nb) in enumerate(jobs):
        assert int(h_lens[j]) == len(body), (j, w, h, band)
        if body:
            assert int(h_nb[j]) == nb, j
        assert bytes(h_stream[int(h_offs[j]):int(h_offs[j]) + len(body)]) == body, (j, w, h, band, nb)


@pytest.mark.parametrize("form", list(ENC_FORMS))
@pytest.mark.parametrize("shape", rm.SHAPES, ids=["%dx%d" % s for s in rm.SHAPES])
def test_blocks_every_encoder_form(env, shape, form):
    torch, orc, _ = env
    ctx = _ctx(ENC_FORMS[form])
    plan = _block_plan(ctx, shape)
    try:
        assert plan.raw_magref
        jobs, coeff = _family(plan, shape, orc)
        n = len(jobs)
        if shape in ((4, 4), (33, 17)):
            assert n > 64 and n % 64
        d_coeff = _dev(torch, plan, coeff)
        slots, lens, numbps = plan.encode_blocks(d_coeff)
        offs, stream = plan.compact(slots, lens)
        decoded = plan.decode_blocks(stream, offs, lens, numbps)
        s2, o2, l2, n2 = plan.encode_stream(d_coeff)
        ctx.sync()
        h_offs, h_lens, h_nb = offs.cpu().numpy(), lens.cpu().numpy(), numbps.cpu().numpy()
        _check_bodies(jobs, stream.cpu().numpy(), h_offs, h_lens, h_nb)
        _check_bodies(jobs, s2.cpu().numpy(), o2.cpu().numpy(), l2.cpu().numpy(), n2.cpu().numpy())
        dh, doffs = decoded.cpu().numpy(), plan.decoded_offsets()
        for j, (w, h, band, data, body, nb) in enumerate(jobs):
            assert np.array_equal(dh[int(doffs[j]):int(doffs[j]) + w * h].reshape(h, w), data), (j, w, h, band)
    finally:
        plan.close()
        ctx.close()


@pytest.mark.parametrize("form", list(DEC_FORMS))
@pytest.mark.parametrize("shape", [(33, 17), (64, 64), (1, 64), (4, 4), (1, 1)], ids=["33x17", "64x64", "1x64", "4x4", "1x1"])
def test_blocks_every_decoder_knob(env, shape, form):
    """the definition's bodies, laid out by the test, decode to the data under every decoder option"""
    torch, orc, _ = env
    ctx = _ctx(DEC_FORMS[form])
    plan = _block_plan(ctx, shape)
    try:
        jobs, _ = _family(plan, shape, orc)
        stream = b"".join(j[4] for j in jobs)
        lens = np.array([len(j[4]) for j in jobs], np.int32)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        nbs = np.array([j[5] for j in jobs], np.uint8)
        d_stream = _dev(torch, plan, np.frombuffer(stream + bytes(64), np.uint8))
        decoded = plan.decode_blocks(d_stream, _dev(torch, plan, offs), _dev(torch, plan, lens), _dev(torch, plan, nbs))
        ctx.sync()
        dh, doffs = decoded.cpu().numpy(), plan.decoded_offsets()
        for j, (w, h, band, data, body, nb) in enumerate(jobs):
            assert np.array_equal(dh[int(doffs[j]):int(doffs[j]) + w * h].reshape(h, w), data), (j, w, h, band)
    finally:
        plan.close()
        ctx.close()


@pytest.mark.parametrize("form", LANES_FORMS)
@pytest.mark.parametrize("k", [1, 3, 12, 31])
def test_skip_planes_is_coarse(env, k, form):
    """k = 12: numbps of the noise blocks (11 or 12), the all-planes-skipped edge for them while the 15- and 31-plane blocks still decode"""
    torch, orc, _ = env
    ctx = _ctx(DEC_FORMS[form])
    plan = _block_plan(ctx, (33, 17))
    try:
        jobs, coeff = _family(plan, (33, 17), orc)
        assert 12 in {j[5] for j in jobs}
        stream, offs, lens, numbps = plan.encode_stream(_dev(torch, plan, coeff))
        decoded = plan.decode_blocks(stream, offs, lens, numbps, skip_planes=k)
        ctx.sync()
        dh, doffs = decoded.cpu().numpy(), plan.decoded_offsets()
        for j, (w, h, band, data, body, nb) in enumerate(jobs):
            assert np.array_equal(dh[int(doffs[j]):int(doffs[j]) + w * h].reshape(h, w), cc.coarse(data, k)), (j, band, nb)
    finally:
        plan.close()
        ctx.close()


@pytest.mark.parametrize("form", LANES_FORMS)
def test_foreign_bodies(env, form):
    """random byte strings as bodies of 8 x 8 blocks (all four bands): the samples are decode_block's; with other bytes between the bodies the
    samples are the same -- nothing a decoder reads outside offs + lens reaches its output"""
    torch, orc, _ = env
    from j2kgfx.codec import FramePlan
    ctx = _ctx(DEC_FORMS[form])
    plan = FramePlan(160, 160, 1, precision=8, lossless=True, num_resolutions=2, cb=(8, 8), tile=(0, 0), coder=0, ctx=ctx, mallat=True, raw_magref=True)
    try:
        blocks = plan.blocks()
        n = len(blocks)
        bodies = rm.foreign_bodies(n)
        assert n >= 300 and len(bodies) == n
        outs = []
        for fill in (0x00, 0xFF):
            buf, offs = bytearray(), []
            for i, (b, _nb) in enumerate(bodies):
                buf += bytes([fill]) * (i % 5)                  # gaps between the bodies
                offs.append(len(buf))
                buf += b
            buf += bytes([fill]) * 64
            offs.append(len(buf))
            lens = np.array([len(b) for b, _ in bodies], np.int32)
            nbs = np.array([nb for _, nb in bodies], np.uint8)
            decoded = plan.decode_blocks(_dev(torch, plan, np.frombuffer(bytes(buf), np.uint8)), _dev(torch, plan, np.array(offs, np.int64)),
                                         _dev(torch, plan, lens), _dev(torch, plan, nbs))
            ctx.sync()
            outs.append(decoded.cpu().numpy().copy())
        assert np.array_equal(outs[0], outs[1])
        doffs = plan.decoded_offsets()
        for j, (b, nb) in enumerate(bodies):
            w, h, band = int(blocks[j]["w"]), int(blocks[j]["h"]), int(blocks[j]["band"])
            want = rm.decode_block(b, nb, band, w, h, orc)
            assert np.array_equal(outs[0][int(doffs[j]):int(doffs[j]) + w * h].reshape(h, w), want), (j, len(b), nb, band)
    finally:
        plan.close()
        ctx.close()


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
def _frame_plan(ctx, name, raw=True):
    from j2kgfx.codec import FramePlan
    c = rm.FRAMES[name]
    return FramePlan(c["W"], c["H"], c["comps"], precision=c["prec"], lossless=c["lossless"], quality=c["quality"], num_resolutions=c["nres"], cb=(c["cb"], c["cb"]),
                     tile=c["tile"], coder=0, ctx=ctx, closed_loop=True, mallat=c["mallat"], raw_magref=raw, dequantize=not c["lossless"])


def _fmt(c):
    return mc.PIX_FORMAT[(c["comps"], c["prec"])]


@pytest.mark.parametrize("name", list(rm.FRAMES))
def test_frames_equal_the_definition(env, name):
    """tile-parts byte for byte, bare and with SOP + EPH; the pixels back are those of the same plan with the style off (lossless: the source)"""
    torch, orc, t2ref = env
    c = rm.FRAMES[name]
    ctx = _ctx({})
    plan, plain = _frame_plan(ctx, name), _frame_plan(ctx, name, raw=False)
    try:
        pix, _ = rm.frame_pixels(c, orc)
        d_pix = _dev(torch, plan, pix)
        for marks in (False, True):
            want = rm.frame_stream(name, marks, marks, orc, t2ref)
            cs, toffs = plan.encode_frame_pixels(_fmt(c), d_pix, sop=marks, eph=marks)
            plan.frame_status()
            total = int(toffs[-1].item())
            assert bytes(cs.cpu().numpy()[:total]) == want, marks
            back = torch.full(pix.shape, SENTINEL, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=marks, eph=marks)
            plan.frame_status()
            cs0, toffs0 = plain.encode_frame_pixels(_fmt(c), d_pix, sop=marks, eph=marks)
            plain.frame_status()
            assert int(toffs0[-1].item()) != total or not torch.equal(cs0[:total], cs[:total])
            back0 = torch.full(pix.shape, SENTINEL, dtype=torch.uint8, device=plan.device)
            plain.decode_frame_pixels(cs0, int(toffs0[-1].item()), back0, tile_offs=toffs0, sop=marks, eph=marks)
            plain.frame_status()
            assert torch.equal(back, back0)
            if c["lossless"]:
                assert np.array_equal(back.cpu().numpy(), pix)
    finally:
        plan.close()
        plain.close()
        ctx.close()


def test_golden_digests(env):
    """the device reproduces the digests the definition wrote (tests/golden/make_raw_magref_golden.py)"""
    torch, orc, _ = env
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", rm.GOLDEN_FILE)) as f:
        gold = json.load(f)
    ctx = _ctx({})
    try:
        for name in rm.GOLDEN_FRAMES:
            c = rm.FRAMES[name]
            sop, eph = rm.GOLDEN_FLAGS[name]
            plan = _frame_plan(ctx, name)
            pix, _ = rm.frame_pixels(c, orc)
            res = plan.encode_pixels_host(_fmt(c), pix, sop=sop, eph=eph)
            s = bytes(res["bytes"])
            assert gold[name] == dict(sop=sop, eph=eph, bytes=len(s), sha256=hashlib.sha256(s).hexdigest()), name
            plan.close()
    finally:
        ctx.close()


def test_reference_mode_plan(env):
    """a plan that is not closed-loop (the reference's overlapping windows) through encode_stream / decode_blocks"""
    torch, orc, _ = env
    from j2kgfx.codec import FramePlan
    W, H, nres, cb = 64, 48, 3, 32
    frm = rm.frame_pixels(dict(W=W, H=H, comps=3, prec=8, seed=405, noise=16), orc)[1]
    ctx = _ctx({})
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=nres, cb=(cb, cb), coder=0, ctx=ctx, raw_magref=True)
    try:
        coeff = orc.preprocess([frm[c] for c in range(3)], W, H, 8, True, nres)
        by, lens, nb = rm.encode_tile_blocks(orc, coeff, W, H, nres, cb, cb, 0)
        d_coeff = plan.forward(_dev(torch, plan, frm))
        stream, offs, d_lens, numbps = plan.encode_stream(d_coeff)
        decoded = plan.decode_blocks(stream, offs, d_lens, numbps)
        ctx.sync()
        n = int(plan.info.blocks)
        assert np.array_equal(d_lens.cpu().numpy()[:n].astype(np.uint32), lens)
        assert bytes(stream.cpu().numpy()[:int(offs[n].item())]) == bytes(by)
        assert np.array_equal(numbps.cpu().numpy()[:n][lens > 0], nb[lens > 0])
        jobs = orc.enumerate_blocks(3, W, H, nres, cb, cb, 0)
        dh, doffs = decoded.cpu().numpy(), plan.decoded_offsets()
        for j, b in enumerate(jobs):
            w, h = int(b["w"]), int(b["h"])
            assert np.array_equal(dh[int(doffs[j]):int(doffs[j]) + w * h].reshape(h, w), rm.extract(coeff[int(b["comp"])], W, H, b)), j
    finally:
        plan.close()
        ctx.close()


def test_mallat_reduce_and_area(env):
    """reduce = 1, area on a rectangle that straddles a tile corner, area + skip_planes = 2: the reduction (mallat_cases.inverse_frame) and the
    crop of the full decode, of the coarse coefficients (coarse_cases) where planes are skipped -- and what the same plan with the style off
    decodes from its own stream"""
    torch, orc, t2ref = env
    name = "mallat_130x70"
    c = rm.FRAMES[name]
    ctx = _ctx({})
    plan, plain = _frame_plan(ctx, name), _frame_plan(ctx, name, raw=False)
    try:
        pix, _ = rm.frame_pixels(c, orc)
        d_pix = _dev(torch, plan, pix)
        got = []
        for p in (plan, plain):
            cs, toffs = p.encode_frame_pixels(_fmt(c), d_pix, sop=True, eph=True)
            p.frame_status()
            total = int(toffs[-1].item())
            outs = []
            for kw in (dict(reduce=1), dict(area=(50, 20, 90, 45)), dict(area=(50, 20, 90, 45), skip_planes=2), dict(area=(60, 30, 70, 34), reduce=1), dict(skip_planes=2)):
                if "area" in kw:
                    hh, ww = p.area_shape(kw["area"], kw.get("reduce", 0))
                elif kw.get("reduce"):
                    hh, ww = p.reduced_shape(kw["reduce"])
                else:
                    hh, ww = c["H"], c["W"]
                back = torch.full((hh, ww * 4), SENTINEL, dtype=torch.uint8, device=p.device)
                p.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=True, eph=True, **kw)
                p.frame_status()
                outs.append(back.cpu().numpy().copy())
            got.append(outs)
        for a, b in zip(*got):
            assert np.array_equal(a, b)
        full = pix.reshape(c["H"], c["W"], 4)
        assert np.array_equal(got[0][1].reshape(25, 40, 4), full[20:45, 50:90])           # the rectangle straddles the corner of tiles (64, 32)
        # ... and directly: the definition's coefficients (the blocks decode to them, the style is lossless), coarse where planes are skipped,
        # through the oracle's inverse to the reduced frame, cropped to the rectangle
        _, want = rm.frame_want(name, orc, t2ref)
        tiles = [np.stack([np.asarray(p, np.int32) for p in want[t]["coeff"]]) for t in sorted(want)]

        def ref(k, r):
            f = mc.inverse_frame(orc, cc.coarse_tiles(tiles, k) if k else tiles, c["W"], c["H"], c["tile"], c["prec"], c["nres"], reduce=r)
            return mc.pixels(orc, f, c["prec"]).reshape(f.shape[1], f.shape[2], 4)
        assert np.array_equal(ref(0, 0), full)
        assert np.array_equal(got[0][0].reshape(ref(0, 1).shape), ref(0, 1))                                # reduce = 1
        assert np.array_equal(got[0][2].reshape(25, 40, 4), ref(2, 0)[20:45, 50:90])                      # area + skip_planes = 2
        assert np.array_equal(got[0][3].reshape(2, 5, 4), ref(0, 1)[15:17, 30:35])                        # area + reduce = 1
        assert np.array_equal(got[0][4].reshape(c["H"], c["W"], 4), ref(2, 0))                            # skip_planes = 2
    finally:
        plan.close()
        plain.close()
        ctx.close()


def test_host_forms_capture_and_switching(env):
    torch, orc, t2ref = env
    import go_image_ref as gref
    from j2kgfx.pixels import CMYK
    name = "mallat_130x70"
    c = rm.FRAMES[name]
    W, H = c["W"], c["H"]
    ctx = _ctx({})
    plan = _frame_plan(ctx, name)
    try:
        pix, _ = rm.frame_pixels(c, orc)
        want = rm.frame_stream(name, True, True, orc, t2ref)
        plain_want = b"".join(v["part"] for _, v in sorted(rm.repacket(rm.frame_want(name, orc, t2ref, style=False)[1], c["nres"], c["cb"], True, True, orc, t2ref).items()))
        # host one-call forms
        res = plan.encode_pixels_host(_fmt(c), pix, sop=True, eph=True)
        assert bytes(res["bytes"]) == want
        assert np.array_equal(plan.decode_pixels_host(res["bytes"], pix.shape, sop=True, eph=True), pix)
        hr, wr = plan.reduced_shape(1)
        red = plan.decode_pixels_host(res["bytes"], (hr, wr * 4), sop=True, eph=True, reduce=1)
        # an image source: the call equals the RGBA8 call on its colours
        rng = np.random.default_rng(9)
        cm = rng.integers(0, 256, size=H * 4 * W, dtype=np.uint8)
        rgb, img = gref.cmyk_image_rgb(cm, 4 * W, (0, 0, W, H)), CMYK(cm, 4 * W, (0, 0, W, H))
        a = plan.encode_pixels_host(2, gref.rgba8_frame(rgb), sop=False, eph=False)
        b = plan.encode_image_host(img, sop=False, eph=False)
        assert bytes(a["bytes"]) == bytes(b["bytes"]) and np.array_equal(a["lens"], b["lens"])
        assert np.array_equal(plan.decode_pixels_host(b["bytes"], (H, W * 4)).reshape(H, W, 4)[..., :3], rgb)
        # the style off, on, off between frames: every frame decodes under the setting it was coded with
        d_pix = _dev(torch, plan, pix)
        streams = {}
        for on in (True, False, True):
            plan.set_raw_magref(on)
            assert plan.raw_magref == on
            cs, toffs = plan.encode_frame_pixels(_fmt(c), d_pix, sop=True, eph=True)
            plan.frame_status()
            total = int(toffs[-1].item())
            assert bytes(cs.cpu().numpy()[:total]) == (want if on else plain_want), on
            streams[on] = (cs.clone(), toffs.clone(), total)
        for on in (False, True, False):
            plan.set_raw_magref(on)
            cs, toffs, total = streams[on]
            back = torch.full(pix.shape, SENTINEL, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=True, eph=True)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy(), pix), on
        # one captured replay of the frame calls; the setter is refused while the capture runs
        from j2kgfx import _lib
        plan.set_raw_magref(True)
        cs, toffs = plan.encode_frame_pixels(_fmt(c), d_pix, sop=True, eph=True)
        back = torch.zeros(pix.shape, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, int(cs.numel()), back, tile_offs=toffs, sop=True, eph=True)
        plan.frame_status()
        with ctx.capture() as g:
            assert ctx.L.j2k_plan_set_raw_magref(plan.h, 0) == _lib.ERR_INVALID_ARG
            plan.encode_frame_pixels(_fmt(c), d_pix, sop=True, eph=True, out=cs, tile_offs=toffs)
            plan.decode_frame_pixels(cs, int(cs.numel()), back, tile_offs=toffs, sop=True, eph=True)
        assert plan.raw_magref
        pix2 = np.ascontiguousarray(pix[::-1])
        d_pix.copy_(torch.from_numpy(pix2))
        cs.zero_()
        back.zero_()
        torch.cuda.synchronize()
        g.launch()
        ctx.sync()
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), pix2)
        assert bytes(cs.cpu().numpy()[:3]) != b"\0\0\0" and red.shape == (hr, wr * 4)
        g.close()
    finally:
        plan.close()
        ctx.close()


# ---- the interface and its refusals -------------------------------------------------------------------------------------------------------------
def test_setter(env):
    """fails without the feature: the symbol, the keyword and the property are new"""
    torch, orc, _ = env
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    ctx = _ctx({})
    try:
        assert "j2k_plan_set_raw_magref" in _lib.SYMBOLS and "j2k_plan_get_raw_magref" in _lib.SYMBOLS
        plan = FramePlan(64, 64, 1, num_resolutions=2, cb=(32, 32), coder=0, ctx=ctx)
        assert not plan.raw_magref
        plan.set_raw_magref()
        assert plan.raw_magref and ctx.L.j2k_plan_get_raw_magref(plan.h) == 1
        plan.set_raw_magref(False)
        assert not plan.raw_magref
        plan.close()
        assert FramePlan(64, 64, 1, num_resolutions=2, cb=(32, 32), coder=0, ctx=ctx, raw_magref=True).raw_magref
        ht = FramePlan(64, 64, 1, num_resolutions=2, cb=(32, 32), coder=1, ctx=ctx)
        assert _status(lambda: ht.set_raw_magref(True)) == _lib.ERR_UNSUPPORTED and not ht.raw_magref
        assert _status(lambda: FramePlan(64, 64, 1, num_resolutions=2, cb=(32, 32), coder=1, ctx=ctx, raw_magref=True)) == _lib.ERR_UNSUPPORTED
        big = FramePlan(256, 256, 1, num_resolutions=1, cb=(128, 128), coder=0, ctx=ctx)
        assert _status(lambda: big.set_raw_magref(True)) == _lib.ERR_UNSUPPORTED and not big.raw_magref
        assert ctx.L.j2k_plan_set_raw_magref(None, 1) == _lib.ERR_INVALID_ARG
    finally:
        ctx.close()


def test_refusals_leave_outputs_untouched(env):
    torch, orc, _ = env
    from j2kgfx import _lib
    name = "mallat_130x70"
    c = rm.FRAMES[name]
    ctx = _ctx({})
    plan = _frame_plan(ctx, name)
    try:
        pix, frm = rm.frame_pixels(c, orc)
        d_pix = _dev(torch, plan, pix)
        cs, toffs = plan.encode_frame_pixels(_fmt(c), d_pix)
        plan.frame_status()
        total = int(toffs[-1].item())
        n, nt = int(plan.info.blocks), int(plan.info.tiles)
        U = _lib.ERR_UNSUPPORTED

        def sent(numel, dtype=torch.uint8):
            size = torch.empty(0, dtype=dtype).element_size()
            return torch.full((max(int(numel), 4) * size,), SENTINEL, dtype=torch.uint8, device=plan.device).view(dtype)

        coeff = plan.forward_pixels(_fmt(c), d_pix)
        stream, offs, lens, numbps = plan.encode_stream(coeff)
        ctx.sync()
        # encode side
        slots, l2, n2 = sent(plan.info.bytes_cap), sent(n, torch.int32), sent(n)
        assert _status(lambda: plan.encode_blocks(coeff, slots=slots, lens=l2, numbps=n2, planes=True)) == U
        assert _status(lambda: plan.encode_blocks(coeff, slots=slots, lens=l2, numbps=n2, planes=True, roi=(0, 0, 32, 32))) == U
        out, to = sent(plan.frame_bound_layers(3) or plan.frame_bound()), sent(nt + 1, torch.int64)
        for kw in (dict(max_body_bytes=4000), dict(layer_bytes=[2000, 4000]), dict(max_body_bytes=4000, roi=(0, 0, 32, 32)), dict(layer_bytes=[2000, 4000], roi=(0, 0, 32, 32)),
                   dict(min_psnr=30.0), dict(max_distortion=1e6), dict(layer_psnr=[25.0, 35.0]), dict(layer_distortion=[1e7, 1e6])):
            assert _status(lambda: plan.encode_frame_pixels(_fmt(c), d_pix, out=out, tile_offs=to[:nt + 1], **kw)) == U, kw
            assert _status(lambda: plan.encode_pixels_host(_fmt(c), pix, **kw)) == U, kw
        rate = torch.zeros((n, 32), dtype=torch.int32, device=plan.device)
        dist = torch.zeros((n, 32), dtype=torch.int64, device=plan.device)
        kept = sent(3 * n)
        assert _status(lambda: plan.rate_allocate(rate, dist, numbps, 4000, kept=kept)) == U
        assert _status(lambda: plan.rate_allocate_layers(rate, dist, numbps, [2000, 4000], kept=kept)) == U
        assert _status(lambda: plan.rate_allocate_quality(rate, dist, numbps, [1e6], kept=kept)) == U
        assert _status(lambda: plan.encode_tile_parts(stream, offs, lens, numbps, out=out, tile_offs=to[:nt + 1], kept=kept, rate=rate)) == U
        assert _status(lambda: plan.encode_tile_parts(stream, offs, lens, numbps, out=out, tile_offs=to[:nt + 1], kept=kept, rate=rate, layers=2)) == U
        for t in (slots, l2, n2, out, to, kept):
            assert bool((t.view(torch.uint8) == SENTINEL).all())
        # decode side
        back = torch.full(pix.shape, SENTINEL, dtype=torch.uint8, device=plan.device)
        h_back = np.full(pix.shape, SENTINEL, np.uint8)
        for kw in (dict(truncated=True), dict(layers=1), dict(truncated=True, reduce=1), dict(layers=2, skip_planes=1)):
            assert _status(lambda: plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, **kw)) == U, kw
            assert _status(lambda: plan.decode_pixels_host(cs.cpu().numpy()[:total], pix.shape, **kw)) == U, kw
        area = (0, 0, c["W"], c["H"])
        for kw in (dict(truncated=True), dict(layers=1)):
            assert _status(lambda: plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, area=area, **kw)) == U, kw
            assert _status(lambda: plan.decode_pixels_host(cs.cpu().numpy()[:total], pix.shape, area=area, pix=h_back, **kw)) == U, kw
        o3, l3, n3, fl = sent(n + 1, torch.int64), sent(n, torch.int32), sent(n), sent(n)
        assert _status(lambda: plan.decode_tile_parts(cs, total, tile_offs=toffs, offs=o3, lens=l3, numbps=n3, floors=fl)) == U
        assert _status(lambda: plan.decode_tile_parts(cs, total, tile_offs=toffs, offs=o3, lens=l3, numbps=n3, floors=fl, layers=1)) == U
        dec = sent(plan.info.decoded_elems, torch.int32)
        floors = torch.zeros(n, dtype=torch.uint8, device=plan.device)
        assert _status(lambda: plan.decode_blocks(stream, offs, lens, numbps, decoded=dec, floors=floors)) == U
        ctx.sync()
        for t in (back, o3, l3, n3, fl, dec):
            assert bool((t.view(torch.uint8) == SENTINEL).all())
        assert (h_back == SENTINEL).all()
        # the context is usable, and with the style off every call takes the branch it took
        plan.decode_frame_pixels(cs, total, back, tile_offs=toffs)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), pix)
        plan.set_raw_magref(False)
        out, to, lo = plan.encode_frame_pixels(_fmt(c), d_pix, layer_bytes=[2000, 4000])
        plan.frame_status()
        assert int(to[-1].item()) > 0
    finally:
        plan.close()
        ctx.close()
