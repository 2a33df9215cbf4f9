"""GPU: the closed-loop mode (j2k_params.closed_loop: pixels -> tile-parts of packets -> pixels) beyond 8-bit RGB -- one, three and four
components, 8 to 16 bit, all six Go pixel formats, the BASELINE geometries C3 / C4 / C5, pixels stored into pinned host memory.  Every
comparison is HIP against the oracle (oracle/j2k_oracle.c through oracle.py, t2ref.py; composed in tests/closed_loop_ref.py) or HIP frame call
against HIP stage calls, bit for bit: there is no tolerance in this file.  Lossless MQ plans also give the source back exactly.

(a) every stage against the oracle for every shape of plan      (b) the one-call frame codec on the six pixel formats
(c) the HT frame decoder's kept state beyond RGB8                (d) C3, C4, C5 through the closed loop
(e) inverse_pixels / decode_frame_pixels into a pinned host frame"""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "go-jpeg2000_amd"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import closed_loop_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    import t2ref
    from j2kgfx.context import Context
    ctx = Context(0)
    yield torch, orc, t2ref, ctx
    ctx.close()


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------------
# (components, precision, SOP, EPH, contents): every marker combination three times over the set; "flat" = mid-grey with one spike (empty packets),
# once per precision
STAGE_CASES = [(1, 8, True, True, "noise"), (1, 12, True, False, "noise"), (1, 16, False, True, "noise"),
               (3, 10, False, False, "noise"), (3, 12, True, True, "noise"), (3, 16, False, True, "noise"),
               (4, 8, True, False, "noise"), (4, 16, False, False, "noise"),
               (4, 8, True, True, "flat"), (3, 10, True, False, "flat"), (1, 12, False, True, "flat"), (3, 16, False, False, "flat")]


@pytest.mark.parametrize("coder", [0, 1])
@pytest.mark.parametrize("Cn,prec,sop,eph,kind", STAGE_CASES)
def test_every_stage_against_the_oracle_every_shape_of_plan(env, Cn, prec, sop, eph, kind, coder):
    """job windows, block bytes, lengths, numBPS, tile-parts, parsed block tables, decoded + placed planes, the inverse -- on ragged multi-tile
    frames (odd sizes: bands of unequal widths, one-sample bands), one packet per tile-component and resolution for 1, 3 and 4 components,
    zero_bit_planes = 31 - numBPS and 3 * numBPS - 2 passes up to numBPS 17"""
    torch, orc, t2ref, ctx = env
    W, H, tw, th, nres, cb = [(301, 211, 128, 96, 4, 32), (173, 131, 64, 48, 5, 16), (97, 130, 32, 64, 3, 8)][(Cn + prec // 4) % 3]
    frame = ref.flat_spike(W, H, Cn, prec) if kind == "flat" else ref.frame_n(W, H, Cn, prec, 100 + Cn * 20 + prec + coder)
    # the oracle first, alone: an HT case inside the reference's HT-encoder panic domain is a mistake in this list (ValueError here), not a GPU matter
    want = ref.oracle_frame(frame, W, H, tw, th, nres, cb, coder, sop, eph, orc, t2ref, precision=prec)
    seen = ref.check_every_stage(torch, orc, t2ref, ctx, frame, W, H, tw, th, nres, cb, coder, sop, eph, precision=prec, want=want)
    if kind == "flat":
        assert seen["empty_blocks"] > seen["blocks"] // 2
    elif prec >= 12:
        assert seen["max_numbps"] > 9            # (or the case has silently become an 8-bit one)
    if kind == "noise":
        assert seen["empty_blocks"] == 0


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------------
FORMATS = {"GRAY8": 1, "GRAY16": 2, "RGBA8": 4, "RGBA64": 8, "NRGBA8": 4, "NRGBA64": 8}          # bytes per pixel


def _fmt(name):
    from j2kgfx import _lib
    return {"GRAY8": _lib.PIX_GRAY8, "GRAY16": _lib.PIX_GRAY16, "RGBA8": _lib.PIX_RGBA8, "RGBA64": _lib.PIX_RGBA64, "NRGBA8": _lib.PIX_NRGBA8,
            "NRGBA64": _lib.PIX_NRGBA64}[name]


def _bpp(Cn, prec):
    return (1 if Cn == 1 else 4) * (2 if prec > 8 else 1)


def _oracle_tile_pixels(orc, wt, Cn, prec, nres, cb, coder):
    """createImage(postprocess(ReconstructMultiLevel53(DecodeCodeBlock for every job))) of one tile of an oracle frame: uint8 [h, w * bpp]"""
    planes = orc.decode_tile_blocks(wt["bytes"], wt["lens"], wt["numbps"], Cn, wt["w"], wt["h"], nres, cb, cb, coder, 1)
    sub = [orc.reconstruct53(planes[c], wt["w"], wt["h"], nres - 1) for c in range(Cn)]
    return orc.create_image(orc.postprocess(sub, prec, True), prec)


def _frame_calls_against_stage_calls_and_oracle(env, plan, fmt, pix, Cn, prec, planes, geometry, coder, sop, eph, sentinel=0x5A):
    """encode_frame_pixels == forward_pixels + encode_stream + encode_tile_parts == the oracle's tile-parts; decode_frame_pixels ==
    inverse_pixels(place_blocks(decode_blocks)) == the oracle's pixels; the bytes between the rows of the output stay as they were.
    Returns (tile-parts, their positions, the pixels that came back [H, stride])."""
    torch, orc, t2ref, ctx = env
    W, H, tw, th, nres, cb = geometry
    want = ref.oracle_frame(planes, W, H, tw or W, th or H, nres, cb, coder, sop, eph, orc, t2ref, precision=prec)     # (HT: outside the panic domain, or a ValueError here)
    d_pix = torch.from_numpy(pix).to(plan.device)
    coeff = plan.forward_pixels(fmt, d_pix)
    stream, offs, lens, numbps = plan.encode_stream(coeff)
    cs1, t1 = plan.encode_tile_parts(stream, offs, lens, numbps, sop=sop, eph=eph)
    plan.frame_status()
    cs2, t2 = plan.encode_frame_pixels(fmt, d_pix, sop=sop, eph=eph)
    plan.frame_status()
    total = int(t1[-1].item())
    assert torch.equal(t1, t2) and torch.equal(cs1[:total], cs2[:total])
    h_cs, h_t = cs2.cpu().numpy(), t2.cpu().numpy()
    assert len(want) == len(h_t) - 1
    for t in sorted(want):
        assert bytes(h_cs[int(h_t[t]):int(h_t[t + 1])]) == want[t]["part"], t
    row = W * _bpp(Cn, prec)
    stride = pix.shape[1]
    outs = []
    for given in (True, False):
        got = torch.full((H, stride), sentinel, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs2, total, got, tile_offs=t2 if given else None, sop=sop, eph=eph)
        plan.frame_status()
        outs.append(got)
    o2, l2, n2 = plan.decode_tile_parts(cs2, total, tile_offs=t2, sop=sop, eph=eph)
    stage = plan.inverse_pixels(plan.place_blocks(plan.decode_blocks(cs2, o2, l2, n2)), torch.full((H, stride), sentinel, dtype=torch.uint8, device=plan.device))
    plan.frame_status()
    assert torch.equal(outs[0], stage) and torch.equal(outs[1], stage)
    back = outs[0].cpu().numpy()
    assert (back[:, row:] == sentinel).all()                       # row padding is not the image's
    for t in sorted(want):
        wt = want[t]
        b = _bpp(Cn, prec)
        assert np.array_equal(back[wt["y0"]:wt["y0"] + wt["h"], wt["x0"] * b:(wt["x0"] + wt["w"]) * b], _oracle_tile_pixels(orc, wt, Cn, prec, nres, cb, coder)), t
    if coder == 0:
        # lossless: what createImage makes of the samples that went in (alpha included where it is a component) -- at 8 bit the source's own bytes;
        # at 16 bit with the int32 wrap of decoder.go:434-451 for samples above 32768
        assert np.array_equal(back[:, :row], orc.create_image([planes[c] for c in range(Cn)], prec))
        if prec == 8:
            assert np.array_equal(back[:, :row], pix[:, :row])
    return cs2, t2, back


@pytest.mark.parametrize("coder", [0, 1])
@pytest.mark.parametrize("geometry,pad", [((328, 211, 128, 96, 4, 32), 16), ((256, 130, 0, 0, 4, 16), 32), ((100, 75, 64, 64, 3, 16), 12)],
                         ids=["ragged-tiles", "untiled", "ragged-tiles-unaligned-rows"])
@pytest.mark.parametrize("name", list(FORMATS))
def test_frame_codec_on_all_six_pixel_formats(env, name, geometry, pad, coder):
    """image.Gray, Gray16, RGBA, RGBA64, NRGBA, NRGBA64 through j2k_plan_encode_frame_pixels / j2k_plan_decode_frame_pixels of a closed-loop plan with the
    component count and precision extractImageData gives for the format; rows further apart than a row is long (16-byte multiples, where the
    level-0 kernels read and write the pixels themselves, and not, where the frame is staged)"""
    torch, orc, t2ref, ctx = env
    from j2kgfx.codec import FramePlan
    W, H, tw, th, nres, cb = geometry
    fmt, bytes_pp = _fmt(name), FORMATS[name]
    pix, Cn, prec, planes = ref.pixel_frame(fmt, W, H, 300 + fmt * 7 + coder, orc, stride=W * bytes_pp + pad, pad_byte=0x3C)
    assert _bpp(Cn, prec) == bytes_pp
    plan = FramePlan(W, H, Cn, precision=prec, lossless=True, num_resolutions=nres, cb=(cb, cb), tile=(tw, th), coder=coder, ctx=ctx, closed_loop=True)
    sop, eph = bool(fmt & 1), bool(fmt & 2) or fmt == 4
    _frame_calls_against_stage_calls_and_oracle(env, plan, fmt, pix, Cn, prec, planes, geometry, coder, sop, eph)
    plan.close()


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------------
def _ht_sequence_step(env, plan, fmt, pix, sop=True, eph=True):
    """one frame through the frame calls of an HT plan against the stage calls, which zero, decode and copy every row every time"""
    torch, orc, t2ref, ctx = env
    d_pix = torch.from_numpy(pix).to(plan.device)
    cs, toffs = plan.encode_frame_pixels(fmt, d_pix, sop=sop, eph=eph)
    plan.frame_status()
    total = int(toffs[-1].item())
    got = torch.zeros_like(d_pix)
    plan.decode_frame_pixels(cs, total, got, tile_offs=toffs, sop=sop, eph=eph)
    plan.frame_status()
    o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=toffs, sop=sop, eph=eph)
    want = plan.inverse_pixels(plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2)), torch.zeros_like(d_pix))
    plan.frame_status()
    assert torch.equal(got, want)
    return total


def _sequence_frames(orc, fmt, W, H, seed):
    """busy, flat (empty blocks where there were bytes a frame ago), busy again, busy"""
    return [ref.pixel_frame(fmt, W, H, seed, orc)[0], ref.pixel_frame(fmt, W, H, seed, orc, flat=True)[0],
            ref.pixel_frame(fmt, W, H, seed + 1, orc, noise=3)[0], ref.pixel_frame(fmt, W, H, seed + 2, orc)[0]]


@pytest.mark.parametrize("name,W,H,tile,cb,nres", [("GRAY16", 640, 360, (256, 256), 64, 5), ("RGBA64", 301, 211, (128, 96), 32, 4), ("NRGBA8", 328, 130, (0, 0), 16, 3),
                                                    ("NRGBA64", 97, 130, (32, 64), 8, 3)])
def test_ht_frame_decoder_kept_state_beyond_rgb8(env, name, W, H, tile, cb, nres):
    """j2k_plan_decode_frame_pixels on an HT plan writes the coded rows only, into coefficient planes it zeroed once: frame after frame on ONE plan the pixels
    equal those of the stage calls -- for one, three and four components at 8 and 16 bit"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    fmt = _fmt(name)
    _, Cn, prec, _ = ref.pixel_frame(fmt, 8, 8, 0, orc)
    plan = FramePlan(W, H, Cn, precision=prec, lossless=True, num_resolutions=nres, cb=(cb, cb), tile=tile, coder=_lib.CODER_HT, ctx=ctx, closed_loop=True)
    sizes = [_ht_sequence_step(env, plan, fmt, pix) for pix in _sequence_frames(orc, fmt, W, H, 500)]
    assert sizes[1] < sizes[0] // 4            # (the flat frame is one: nearly every packet empty)
    plan.close()


def test_ht_frame_decoder_two_plans_of_one_context_take_turns(env):
    """the workspaces (zeroed coefficient planes, block tables) belong to the plan, the staging buffers to the context: two HT plans of different
    geometry, component count and depth on one context, frame about"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    a = FramePlan(640, 360, 1, precision=16, lossless=True, num_resolutions=5, cb=(64, 64), tile=(256, 256), coder=_lib.CODER_HT, ctx=ctx, closed_loop=True)
    b = FramePlan(301, 211, 4, precision=8, lossless=True, num_resolutions=4, cb=(32, 32), tile=(128, 96), coder=_lib.CODER_HT, ctx=ctx, closed_loop=True)
    fa, fb = _sequence_frames(orc, _lib.PIX_GRAY16, 640, 360, 520), _sequence_frames(orc, _lib.PIX_NRGBA8, 301, 211, 530)
    for k in range(4):
        _ht_sequence_step(env, a, _lib.PIX_GRAY16, fa[k])
        _ht_sequence_step(env, b, _lib.PIX_NRGBA8, fb[k], sop=bool(k & 1), eph=True)
    a.close()
    b.close()


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------------------
def _tile_pixels_of(pix, wt, b):
    return pix[wt["y0"]:wt["y0"] + wt["h"], wt["x0"] * b:(wt["x0"] + wt["w"]) * b]


def test_c3_geometry_through_the_closed_loop(env):
    """BASELINE C3: 3840 x 2160, 3 x 12 bit, ICT + 9-7 + the encoder's quantiser at Quality 75, 512 x 512 tiles, 64 x 64 blocks, MQ (the frame of
    test_gpu_shards.test_c3_full_size_sampled_tiles_match_oracle).  The MQ coder is lossless on the quantised coefficients: what the decode body
    hands the inverse transform is exactly what the forward transform made; coefficients and tile-parts of tiles 0 (full) and 39 (256 x 112) are
    the oracle's.  Frame calls: the same frame as an image.RGBA64 (createImage's 12 -> 16 bit scaling; extractImageData scales back to the
    plan's 12 bit, encoder.go:196-210) == the stage calls.  Oracle's share (three tiles) on one CPU core: 1.5 s, making the frame included."""
    torch, orc, t2ref, ctx = env
    import bench
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    W, H, nres, cb = 3840, 2160, 6, 64
    frame = (bench.synth_frame(np, 1).astype(np.int64) * 4095 // 255).astype(np.int32)
    plan = FramePlan(W, H, 3, precision=12, lossless=False, quality=75, num_resolutions=nres, cb=(cb, cb), tile=(512, 512), coder=_lib.CODER_MQ, ctx=ctx, closed_loop=True)
    coeff = plan.forward(torch.from_numpy(frame).to(plan.device))
    stream, offs, lens, numbps = plan.encode_stream(coeff)
    cs, toffs = plan.encode_tile_parts(stream, offs, lens, numbps, sop=True, eph=True)
    plan.frame_status()
    total = int(toffs[-1].item())
    o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=None, sop=True, eph=True)
    placed = plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2))
    plan.frame_status()
    ne = int(plan.info.coeff_elems)
    assert torch.equal(placed[:ne], coeff[:ne])
    t0 = time.time()
    want = ref.oracle_frame(frame, W, H, 512, 512, nres, cb, 0, True, True, orc, t2ref, tiles={0, 39}, precision=12, lossless=False, quality=75)
    t_oracle = time.time() - t0
    h_cs, h_t, hco, rows = cs.cpu().numpy(), toffs.cpu().numpy(), coeff.cpu().numpy(), plan.planes()
    assert max(int(want[t]["numbps"].max()) for t in want) > 9
    for t in (0, 39):
        wt = want[t]
        for c in range(3):
            off = int(rows[t * 3 + c][6])
            assert np.array_equal(hco[off:off + wt["w"] * wt["h"]].reshape(wt["h"], wt["w"]), wt["coeff"][c]), (t, c)
        assert bytes(h_cs[int(h_t[t]):int(h_t[t + 1])]) == wt["part"], t
    # the frame calls
    pix = orc.create_image([frame[c] for c in range(3)], 12)
    seen = np.stack(orc.extract_image_data(pix, _lib.PIX_RGBA64, W, H, 12))             # what an encoder at 12 bit sees in that image
    assert np.abs(seen - frame).max() <= 1
    d_pix = torch.from_numpy(pix).to(plan.device)
    c1 = plan.forward_pixels(_lib.PIX_RGBA64, d_pix)
    s1 = plan.encode_stream(c1)
    cs1, t1 = plan.encode_tile_parts(*s1, sop=False, eph=True)
    plan.frame_status()
    cs2, t2 = plan.encode_frame_pixels(_lib.PIX_RGBA64, d_pix, sop=False, eph=True)
    plan.frame_status()
    n1 = int(t1[-1].item())
    assert torch.equal(t1, t2) and torch.equal(cs1[:n1], cs2[:n1])
    t0 = time.time()
    want2 = ref.oracle_frame(seen, W, H, 512, 512, nres, cb, 0, False, True, orc, t2ref, tiles={39}, precision=12, lossless=False, quality=75)
    t_oracle += time.time() - t0
    h2, ht2 = cs2.cpu().numpy(), t2.cpu().numpy()
    assert bytes(h2[int(ht2[39]):int(ht2[40])]) == want2[39]["part"]
    got = torch.zeros_like(d_pix)
    plan.decode_frame_pixels(cs2, n1, got, tile_offs=t2, sop=False, eph=True)
    o3, l3, n3 = plan.decode_tile_parts(cs2, n1, tile_offs=t2, sop=False, eph=True)
    placed2 = plan.place_blocks(plan.decode_blocks(cs2, o3, l3, n3))
    stage = plan.inverse_pixels(placed2, torch.zeros_like(d_pix))
    plan.frame_status()
    assert torch.equal(placed2[:ne], c1[:ne]) and torch.equal(got, stage)
    print("C3 closed loop: the oracle's share %.1f s" % t_oracle)
    plan.close()


def test_c4_geometry_through_the_closed_loop(env):
    """BASELINE C4: 7680 x 4320, 3 x 10 bit, 512 x 512 tiles (135; the last row 224 high), 5-3 + HT, 64 x 64 blocks (the frame of
    test_gpu_shards.test_c4_full_size_sampled_tiles_match_oracle): tile-parts and decoded planes of tiles 0 (full), 14 (right edge) and 134 (the last,
    224 rows) are the oracle's; frame decoder == stage calls is (c)'s matter.  Oracle's share (three tiles) on one CPU core: 1.8 s, making the frame included."""
    torch, orc, t2ref, ctx = env
    import bench
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    W, H, nres, cb = 7680, 4320, 6, 64
    small = bench.synth_frame(np, 4)
    frame = (np.tile(small, (1, 2, 2)).astype(np.int64) * 1023 // 255).astype(np.int32)
    sample = (0, 14, 134)
    t0 = time.time()
    want = ref.oracle_frame(frame, W, H, 512, 512, nres, cb, 1, True, True, orc, t2ref, tiles=set(sample), precision=10)     # (outside the HT panic domain, or a ValueError here)
    ref_planes = {t: orc.decode_tile_blocks(want[t]["bytes"], want[t]["lens"], want[t]["numbps"], 3, want[t]["w"], want[t]["h"], nres, cb, cb, 1, 1) for t in sample}
    t_oracle = time.time() - t0
    assert (want[14]["w"], want[134]["w"], want[134]["h"]) == (512, 512, 224) and want[14]["x0"] == 7168
    plan = FramePlan(W, H, 3, precision=10, lossless=True, num_resolutions=nres, cb=(cb, cb), tile=(512, 512), coder=_lib.CODER_HT, ctx=ctx, closed_loop=True)
    assert int(plan.info.tiles) == 135
    coeff = plan.forward(torch.from_numpy(frame).to(plan.device))
    stream, offs, lens, numbps = plan.encode_stream(coeff)
    cs, toffs = plan.encode_tile_parts(stream, offs, lens, numbps, sop=True, eph=True)
    plan.frame_status()
    total = int(toffs[-1].item())
    h_cs, h_t = cs.cpu().numpy(), toffs.cpu().numpy()
    for t in sample:
        assert bytes(h_cs[int(h_t[t]):int(h_t[t + 1])]) == want[t]["part"], t
    o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=toffs, sop=True, eph=True)
    placed = plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2))
    plan.frame_status()
    hp, rows = placed.cpu().numpy(), plan.planes()
    for t in sample:
        w, h = want[t]["w"], want[t]["h"]
        for c in range(3):
            off = int(rows[t * 3 + c][6])
            assert np.array_equal(hp[off:off + w * h].reshape(h, w), ref_planes[t][c]), (t, c)
    print("C4 closed loop: the oracle's share %.1f s" % t_oracle)
    plan.close()


def test_c5_geometry_through_the_closed_loop(env):
    """BASELINE C5: 2048 x 2048 image.Gray16, untiled, 5-3, MQ, 64 x 64 blocks, through the frame calls: the one tile-part is the oracle's, the pixels
    that come back are createImage of the samples that went in, and the samples themselves come back exactly.  Oracle's share on one CPU
    core: 1.4 s (the whole frame is one tile)."""
    torch, orc, t2ref, ctx = env
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    W = H = 2048
    pix, Cn, prec, planes = ref.pixel_frame(_lib.PIX_GRAY16, W, H, 55, orc, stride=W * 2 + 64, pad_byte=0x3C, noise=2000)
    assert (Cn, prec) == (1, 16)
    plan = FramePlan(W, H, 1, precision=16, lossless=True, num_resolutions=6, cb=(64, 64), coder=_lib.CODER_MQ, ctx=ctx, closed_loop=True)
    d_pix = torch.from_numpy(pix).to(plan.device)
    cs, toffs = plan.encode_frame_pixels(_lib.PIX_GRAY16, d_pix, sop=True, eph=False)
    plan.frame_status()
    total = int(toffs[-1].item())
    got = torch.full((H, W * 2 + 64), 0x5A, dtype=torch.uint8, device=plan.device)
    plan.decode_frame_pixels(cs, total, got, tile_offs=None, sop=True, eph=False)
    o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=toffs, sop=True, eph=False)
    samples = plan.inverse(plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2)))
    plan.frame_status()
    assert np.array_equal(samples.cpu().numpy().reshape(1, H, W), planes)                 # bit-exact round trip
    back = got.cpu().numpy()
    assert np.array_equal(back[:, :W * 2], orc.create_image([planes[0]], 16)) and (back[:, W * 2:] == 0x5A).all()
    t0 = time.time()
    want = ref.oracle_frame(planes, W, H, W, H, 6, 64, 0, True, False, orc, t2ref, precision=16)
    print("C5 closed loop: the oracle's share %.1f s" % (time.time() - t0))
    assert int(want[0]["numbps"].max()) > 9
    assert cs[:total].cpu().numpy().tobytes() == want[0]["part"]
    plan.close()


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,H,tile,nres,coder,pad", [("RGBA8", 3840, 2160, (512, 512), 6, 1, 64), ("RGBA8", 1024, 768, (512, 512), 6, 0, 48),
                                                           ("GRAY16", 640, 360, (256, 256), 5, 1, 32), ("GRAY16", 200, 96, (64, 64), 4, 0, 6)])
def test_pixels_stored_straight_into_pinned_host_memory(env, name, W, H, tile, nres, coder, pad):
    """bench_host.py's way out (J2K_BENCH_HOST_DIRECT): the destination of j2k_plan_inverse_pixels / j2k_plan_decode_frame_pixels is a pinned host frame, which
    the inverse level-0 kernel (or the pack kernel, where the frame is staged) stores into itself.  Byte for byte the device frame of the same
    call, rows further apart than a row is long, and the bytes between the rows still hold what they held"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    fmt = _fmt(name)
    bytes_pp = FORMATS[name]
    stride = W * bytes_pp + pad
    pix, Cn, prec, planes = ref.pixel_frame(fmt, W, H, 700 + W, orc, stride=stride, pad_byte=0x3C)
    if coder == 1:                                               # (outside the reference's HT-encoder panic domain, or a ValueError here)
        ref.oracle_frame(planes, W, H, tile[0], tile[1], nres, 64, 1, True, True, orc, t2ref, precision=prec)
    plan = FramePlan(W, H, Cn, precision=prec, lossless=True, num_resolutions=nres, cb=(64, 64), tile=tile, coder=coder, ctx=ctx, closed_loop=True)
    if coder == 1:
        plan.set_decode_coded_rows_only(True)                    # (as the bench sets it: decode_blocks writes the coded rows into a buffer zeroed once)
    d_pix = torch.from_numpy(pix).to(plan.device)
    cs, toffs = plan.encode_frame_pixels(fmt, d_pix, sop=True, eph=True)
    plan.frame_status()
    total = int(toffs[-1].item())

    def frames():
        return (torch.full((H, stride), 0x5A, dtype=torch.uint8, device=plan.device), torch.full((H, stride), 0x5A, dtype=torch.uint8).pin_memory())
    decoded = torch.zeros(max(int(plan.info.decoded_elems), 4), dtype=torch.int32, device=plan.device)
    for rnd in range(2):                                         # (twice: the second frame meets the kept state of the first)
        dev, pin = frames()
        plan.decode_frame_pixels(cs, total, dev, tile_offs=toffs, sop=True, eph=True)
        plan.decode_frame_pixels(cs, total, pin, tile_offs=toffs, sop=True, eph=True)
        plan.frame_status()
        o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=toffs, sop=True, eph=True)
        placed = plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2, decoded=decoded))
        dev2, pin2 = frames()
        plan.inverse_pixels(placed, dev2)
        plan.inverse_pixels(placed, pin2)
        plan.frame_status()
        h_dev = dev.cpu()
        assert torch.equal(pin, h_dev) and torch.equal(pin2, h_dev) and torch.equal(dev2.cpu(), h_dev), rnd
        assert bool((pin[:, W * bytes_pp:] == 0x5A).all()) and bool((pin2[:, W * bytes_pp:] == 0x5A).all())
        if coder == 0:
            assert np.array_equal(pin.numpy()[:, :W * bytes_pp], orc.create_image([planes[c] for c in range(Cn)], prec))
    plan.close()
