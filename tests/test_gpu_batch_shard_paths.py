"""GPU: the two plan parameters that move every tile -- j2k_params.frame_rows (a batch: frames stacked vertically, the tile grid starting
again at every frame) and tile_first / tile_count (a shard of the tile list) -- through the paths the benchmark configurations take with
them: the closed loop, the packed pixel formats, the level-0 and deep kernels that the geometry of the WHOLE plan selects, image sources,
a graph replay.  tests/test_gpu_batch.py and tests/test_gpu_shards.py have them on the planar stage calls only.

Every comparison is bit for bit; there is no tolerance in this file.  A batch is compared with its frames one by one on plans of their own
(a batch of B frames of T tiles must give B x T tile-parts equal to theirs except for the tile number) and with the oracle's composition
(tests/closed_loop_ref.py: oracle_batch), a shard with the slice of the whole plan's stream, pixels with the source.

(1) batch x closed loop      (2) shard x closed loop      (3) batch x packed pixels, six formats      (4) batch x geometry-selected kernels
(5) batch x image sources    (6) one graph replay of a closed-loop batch
Non-default kernel choices: a Context of the test's own under a patched environment (as tests/test_gpu_knobs.py), closed when the test ends."""
import contextlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "go-jpeg2000_amd"), os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import closed_loop_ref as ref  # noqa: E402
import go_image_ref as goref  # noqa: E402

GRAY8, GRAY16, RGBA8, RGBA64, NRGBA8, NRGBA64 = ref.PIX_FORMATS
BPP = [1, 2, 4, 8, 4, 8]
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    import t2ref
    from j2kgfx.context import Context
    ctx = Context(0)
    yield torch, orc, t2ref, ctx
    ctx.close()


@contextlib.contextmanager
def _ctx(**environ):
    """a Context that read its kernel choices from this environment (they are read when a context is made); closed on the way out"""
    from j2kgfx.context import Context
    old = {k: os.environ.get(k) for k in environ}
    os.environ.update({k: str(v) for k, v in environ.items()})
    try:
        ctx = Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield ctx
    finally:
        ctx.close()


def _first_difference(a, b):
    a, b = np.frombuffer(bytes(a), np.uint8), np.frombuffer(bytes(b), np.uint8)
    n = min(a.size, b.size)
    d = np.nonzero(a[:n] != b[:n])[0]
    return int(d[0]) if d.size else (n if a.size != b.size else -1)


def _tiles_per_frame(W, H, tile):
    return 1 if tile == 0 else -(-W // tile) * -(-H // tile)


# ---- (1) batch x closed loop ---------------------------------------------------------------------------------------------------------------------
# ragged 64-tiles of three components; one tile of one 16-bit component, five resolutions; the lossy path (ICT + 9-7 + the encoder's quantiser)
CL_GEOMETRIES = {
    "rgb8-tile64": dict(W=200, H=75, Cn=3, prec=8, lossless=True, quality=0, tile=64, cb=32, nres=3, B=3, fmt=RGBA8),
    "gray16-untiled": dict(W=256, H=136, Cn=1, prec=16, lossless=True, quality=0, tile=0, cb=64, nres=5, B=4, fmt=GRAY16),
    "rgb12-lossy-tile128": dict(W=320, H=200, Cn=3, prec=12, lossless=False, quality=75, tile=128, cb=32, nres=4, B=2, fmt=RGBA64),
}
_cl_inputs = {}


def _cl_frames(orc, name, coder):
    """two batches for a geometry: (pix [H, row], planes [Cn, H, W]) per frame.  Batch 0 busy; batch 1 different content with flat areas --
    whole frames of mid-grey with one spike and frames whose left five eighths are flat: blocks without bytes where batch 0 had some.
    (HT: gradients + noise of a sixteenth of the range and flat areas are inside the domain of the reference's HT encoder; oracle_batch raises
    a ValueError if a case ever is not.)"""
    key = (name, coder)
    if key in _cl_inputs:
        return _cl_inputs[key]
    g = CL_GEOMETRIES[name]
    W, H, Cn, prec, B, fmt = g["W"], g["H"], g["Cn"], g["prec"], g["B"], g["fmt"]
    batches = []
    for rnd in range(2):
        frames = []
        for b in range(B):
            if rnd == 1 and b % 2 == 0:
                vals = ref.flat_spike(W, H, Cn, prec)
            else:
                vals = ref.frame_n(W, H, Cn, prec, 900 + 10 * rnd + b + 3 * coder)
                if rnd == 1:
                    vals[:, :, :(W * 5) // 8] = 1 << (prec - 1)
            if prec == 12:
                # no Go image holds 12-bit samples as they are: createImage scales them to an image.RGBA64, extractImageData scales back to the
                # plan's 12 bit (encoder.go:196-210) -- the planes are what the encoder sees in that image
                pix = orc.create_image([vals[c] for c in range(Cn)], 12)
                planes = np.stack(orc.extract_image_data(pix, fmt, W, H, 12))
            else:
                pix = orc.create_image([vals[c] for c in range(Cn)], prec)
                planes = np.stack(orc.extract_image_data(pix, fmt, W, H))
            frames.append((pix, planes.astype(np.int32)))
        batches.append(frames)
    _cl_inputs[key] = batches
    return batches


def _plan_kw(g, coder):
    return dict(precision=g["prec"], lossless=g["lossless"], quality=g["quality"], num_resolutions=g["nres"], cb=(g["cb"], g["cb"]), coder=coder,
                closed_loop=True)


@pytest.mark.parametrize("sop,eph", [(False, False), (True, True), (True, False)], ids=["bare", "sop-eph", "sop"])
@pytest.mark.parametrize("coder", [0, 1], ids=["mq", "ht"])
@pytest.mark.parametrize("name", list(CL_GEOMETRIES))
def test_closed_loop_batch_equals_frames_one_by_one_and_the_oracle(env, name, coder, sop, eph):
    """A closed-loop plan over B stacked frames (bench.py --config cl): its tile-parts are the single-frame plans' with Isot = b * tiles + t,
    by the frame call and by the stage calls, and the oracle's; tile_offs rises strictly to the total; the parsed block tables are the single
    plans' (offsets moved to the frame's place in the batch stream); pixels come back (MQ lossless: the source; else: the single plan's
    pixels); a second batch of other content with flat areas on the SAME plan still decodes to itself (the HT frame decoder writes coded rows
    into planes it zeroed once: a block that had bytes a batch ago and has none now must read as zeros); SOP + EPH streams: every tile's
    packets were parsed side by side."""
    torch, orc, t2ref, ctx = env
    from j2kgfx.codec import FramePlan
    g = CL_GEOMETRIES[name]
    W, H, Cn, prec, B, fmt, tile = g["W"], g["H"], g["Cn"], g["prec"], g["B"], g["fmt"], g["tile"]
    kw = _plan_kw(g, coder)
    tiles1 = _tiles_per_frame(W, H, tile)
    batch = FramePlan(W, H * B, Cn, tile=(tile, tile), frame_rows=H, ctx=ctx, **kw)
    assert int(batch.info.tiles) == B * tiles1
    n1 = int(batch.info.blocks) // B
    row = W * BPP[fmt]
    for rnd, frames in enumerate(_cl_frames(orc, name, coder)):
        pix = np.concatenate([f[0] for f in frames], axis=0)
        planes = np.concatenate([f[1] for f in frames], axis=1)
        d_pix = torch.from_numpy(pix).to(batch.device)
        # the frame call and the stage calls
        cs, toffs = batch.encode_frame_pixels(fmt, d_pix, sop=sop, eph=eph)
        batch.frame_status()
        co = batch.forward(torch.from_numpy(planes).to(batch.device))
        stream, offs, lens, nb = batch.encode_stream(co)
        cs_s, toffs_s = batch.encode_tile_parts(stream, offs, lens, nb, sop=sop, eph=eph)
        batch.frame_status()
        h_t = toffs.cpu().numpy().astype(np.int64)
        total = int(h_t[-1])
        assert h_t[0] == 0 and (np.diff(h_t) > 0).all() and h_t.size == B * tiles1 + 1
        assert torch.equal(toffs, toffs_s) and torch.equal(cs[:total], cs_s[:total]), ("frame call != stage calls", rnd)
        h_cs = cs.cpu().numpy()[:total]
        # the block tables out of the batch stream, positions given and walked
        tables = []
        batch.frame_parallel_tiles()                  # (the count is "since the last query": start it here)
        for given in (True, False):
            o2, l2, n2 = batch.decode_tile_parts(cs, total, tile_offs=toffs if given else None, sop=sop, eph=eph)
            batch.frame_status()
            if sop and eph:
                assert batch.frame_parallel_tiles() == B * tiles1
            tables.append((o2.cpu().numpy()[:n1 * B].astype(np.int64), l2.cpu().numpy()[:n1 * B].astype(np.int64), n2.cpu().numpy()[:n1 * B].astype(np.int64)))
        for a, b_ in zip(*tables):
            assert np.array_equal(a, b_)
        back = torch.full((H * B, row), SENTINEL, dtype=torch.uint8, device=batch.device)
        batch.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=sop, eph=eph)
        batch.frame_status()
        h_back = back.cpu().numpy()
        # the stage calls' pixels: every buffer new, nothing kept from the batch before
        o2, l2, n2 = batch.decode_tile_parts(cs, total, tile_offs=toffs, sop=sop, eph=eph)
        stage = batch.inverse_pixels(batch.place_blocks(batch.decode_blocks(cs, o2, l2, n2)), torch.full((H * B, row), SENTINEL, dtype=torch.uint8, device=batch.device))
        batch.frame_status()
        assert torch.equal(back, stage), ("frame decoder != stage calls", rnd)
        # frames one by one
        at = 0
        for b, (pix1, planes1) in enumerate(frames):
            one = FramePlan(W, H, Cn, tile=(tile, tile), ctx=ctx, **kw)
            assert int(one.info.tiles) == tiles1 and int(one.info.blocks) == n1
            d1 = torch.from_numpy(pix1).to(one.device)
            cs1, t1 = one.encode_frame_pixels(fmt, d1, sop=sop, eph=eph)
            one.frame_status()
            h1, ht1 = cs1.cpu().numpy(), t1.cpu().numpy().astype(np.int64)
            for t in range(tiles1):
                k = b * tiles1 + t
                got, want = h_cs[h_t[k]:h_t[k + 1]], h1[ht1[t]:ht1[t + 1]].copy()
                assert int(got[4]) << 8 | int(got[5]) == k and int(want[4]) << 8 | int(want[5]) == t, ("Isot", rnd, b, t)
                want[4:6] = [k >> 8, k & 255]
                assert got.size == want.size and np.array_equal(got, want), ("tile-part", rnd, b, t, _first_difference(got, want))
                at += got.size
            o1, l1, nb1 = one.decode_tile_parts(cs1, int(ht1[-1]), tile_offs=t1, sop=sop, eph=eph)
            back1 = torch.full((H, row), SENTINEL, dtype=torch.uint8, device=one.device)
            one.decode_frame_pixels(cs1, int(ht1[-1]), back1, tile_offs=t1, sop=sop, eph=eph)
            one.frame_status()
            ho1, hl1, hn1 = (x.cpu().numpy()[:n1].astype(np.int64) for x in (o1, l1, nb1))
            j0 = b * n1
            assert np.array_equal(tables[0][1][j0:j0 + n1], hl1) and np.array_equal(tables[0][2][j0:j0 + n1], hn1), ("lens / numbps", rnd, b)
            # a block's offset is where its bytes lie in the stream the call was given (0 for a block without bytes): single plan's + where frame
            # b's first tile-part starts in the batch (every tile-part is as long as the single plan's: compared above)
            assert np.array_equal(tables[0][0][j0:j0 + n1], np.where(hl1 > 0, ho1 + h_t[b * tiles1], 0)), ("offs", rnd, b)
            assert np.array_equal(h_back[b * H:(b + 1) * H], back1.cpu().numpy()), ("pixels: batch != single plan", rnd, b)
            one.close()
        assert at == total
        if coder == 0 and g["lossless"]:
            # the samples come back exactly; as pixels they are createImage of the samples that went in (at 8 bit the source's own bytes; at 16
            # bit with createImage's int32 wrap above 32768, decoder.go:434-451)
            assert np.array_equal(h_back, orc.create_image([planes[c] for c in range(Cn)], prec)), rnd
            if prec == 8:
                assert np.array_equal(h_back, pix), rnd
        # the oracle's tile-parts (HT: inside the reference's domain, or a ValueError here)
        want = ref.oracle_batch([f[1] for f in frames], W, H, tile or W, tile or H, g["nres"], g["cb"], coder, sop, eph, orc, t2ref, precision=prec,
                                lossless=g["lossless"], quality=g["quality"])
        assert len(want) == B * tiles1
        for k, wt in enumerate(want):
            got = bytes(h_cs[h_t[k]:h_t[k + 1]])
            assert got == wt["part"], ("oracle", rnd, wt["frame"], wt["tile"], _first_difference(got, wt["part"]))
        if rnd == 1:
            assert sum(int((wt["lens"] == 0).sum()) for wt in want) > sum(len(wt["lens"]) for wt in want) // 3      # (the flat batch is one)
    batch.close()


# ---- (2) shard x closed loop ---------------------------------------------------------------------------------------------------------------------
def _rgba_of(frm):
    H, W = frm.shape[1:]
    pix = np.full((H, W, 4), 255, np.uint8)
    pix[..., :3] = frm.transpose(1, 2, 0)
    return pix.reshape(H, W * 4)


def _tile_rects(W, H, tile, frame_rows):
    """(x0, y0, w, h) of every tile of a plan in its order: frame after frame, row-major inside a frame"""
    out = []
    for b in range(H // frame_rows):
        for y0 in range(0, frame_rows, tile):
            for x0 in range(0, W, tile):
                out.append((x0, b * frame_rows + y0, min(tile, W - x0), min(tile, frame_rows - y0)))
    return out


SHARD_CASES = {"frame-3x3": dict(W=320, H=300, B=1, tile=128, shards=[(0, 4), (4, 3), (7, 2)]),          # ragged both ways: 64 columns, 44 rows at the edges
               "batch-straddle": dict(W=384, H=200, B=3, tile=128, shards=[(4, 5)]),                    # tiles 4, 5 of frame 0 and 0, 1, 2 of frame 1
               "frame-512-tiles": dict(W=1024, H=600, B=1, tile=512, shards=[(1, 2)])}                  # the level-0 kernels write the pixels themselves: top right, bottom left (88 rows)


@pytest.mark.parametrize("coder", [0, 1], ids=["mq", "ht"])
@pytest.mark.parametrize("name", list(SHARD_CASES))
def test_closed_loop_shard_is_the_slice_of_the_whole_plans_stream_and_decodes_into_its_tiles_only(env, name, coder):
    """tile_first / tile_count on a closed-loop plan (bench.py --shard tiles): the shard's tile-parts are bytes tile_offs[first] ..
    tile_offs[first + count] of the whole plan's stream, Isot = the tile's number in the whole plan included; decoded into a frame that
    holds a sentinel, the shard's tiles hold the source's pixels (MQ; HT: the whole plan's decoded pixels) and every other byte the
    sentinel -- where the pixels are staged through the context's int32 frame (128-tiles) and where the level-0 kernels write them (512).
    (This test found the staged path packing the WHOLE staging frame into the caller's: every tile outside the shard was overwritten with what
    an earlier call had left in the staging buffer.)"""
    torch, orc, t2ref, ctx = env
    from j2kgfx.codec import FramePlan
    c = SHARD_CASES[name]
    W, H, B, tile = c["W"], c["H"], c["B"], c["tile"]
    frm = np.concatenate([ref.frame(W, H, 40 + b + coder, noise=12) for b in range(B)], axis=1)
    pix = _rgba_of(frm)
    kw = dict(precision=8, lossless=True, num_resolutions=4, cb=(32, 32), tile=(tile, tile), coder=coder, closed_loop=True, frame_rows=H if B > 1 else 0, ctx=ctx)
    full = FramePlan(W, H * B, 3, **kw)
    rects = _tile_rects(W, H * B, tile, H)
    assert int(full.info.tiles) == len(rects)
    d_pix = torch.from_numpy(pix).to(full.device)
    cs, toffs = full.encode_frame_pixels(RGBA8, d_pix, sop=True, eph=True)
    full.frame_status()
    h_t = toffs.cpu().numpy().astype(np.int64)
    h_cs = cs.cpu().numpy()[:int(h_t[-1])]
    whole = torch.full_like(d_pix, SENTINEL)
    full.decode_frame_pixels(cs, int(h_t[-1]), whole, tile_offs=toffs, sop=True, eph=True)
    full.frame_status()
    h_whole = whole.cpu().numpy()
    if coder == 0:
        assert np.array_equal(h_whole, pix)
    for first, count in c["shards"]:
        shard = FramePlan(W, H * B, 3, tile_first=first, tile_count=count, **kw)
        assert int(shard.info.tiles) == count
        cs2, t2 = shard.encode_frame_pixels(RGBA8, d_pix, sop=True, eph=True)
        shard.frame_status()
        h2 = t2.cpu().numpy().astype(np.int64)
        assert np.array_equal(h2, h_t[first:first + count + 1] - h_t[first]), (first, count)
        got, want = cs2.cpu().numpy()[:int(h2[-1])], h_cs[h_t[first]:h_t[first + count]]
        assert np.array_equal(got, want), ("shard bytes", first, count, _first_difference(got, want))
        for i in range(count):
            assert int(got[h2[i] + 4]) << 8 | int(got[h2[i] + 5]) == first + i
        for given in (True, False):
            back = torch.full_like(d_pix, SENTINEL)
            shard.decode_frame_pixels(cs2, int(h2[-1]), back, tile_offs=t2 if given else None, sop=True, eph=True)
            shard.frame_status()
            assert shard.frame_parallel_tiles() == count
            want_pix = np.full_like(pix, SENTINEL)
            for (x0, y0, w, h) in rects[first:first + count]:
                want_pix[y0:y0 + h, 4 * x0:4 * (x0 + w)] = (pix if coder == 0 else h_whole)[y0:y0 + h, 4 * x0:4 * (x0 + w)]
            h_back = back.cpu().numpy()
            bad = np.argwhere(h_back != want_pix)
            assert bad.size == 0, ("shard pixels (row, byte)", first, count, given, bad[0].tolist())
        shard.close()
    full.close()


# (format, W, H, tile, lossless, tiles per shard, where the inverse writes the pixels): the staged pack kernel and each family of level-0 kernels
# that writes pixels itself -- RGBA8 workgroup form, single 16-bit planes, RGBA64 triples + an alpha plane, the 9-7 forms for RGBA8 and Gray
REFUSED_GEOMETRIES = {
    "rgba8-staged": (RGBA8, 320, 300, 128, True, 4, False),
    "rgba8-512": (RGBA8, 1024, 600, 512, True, 2, True),
    "gray16-512": (GRAY16, 1024, 600, 512, True, 2, True),
    "nrgba64-512": (NRGBA64, 1024, 600, 512, True, 2, True),
    "rgba8-lossy-512": (RGBA8, 1024, 600, 512, False, 2, True),
    "gray8-lossy-512": (GRAY8, 1024, 600, 512, False, 2, True),
}
REFUSED_CASES = [(n, 0) for n in REFUSED_GEOMETRIES] + [("rgba8-staged", 1), ("rgba8-512", 1)]
REFUSED_IDS = ["%s-%s" % (n, "ht" if c else "mq") for n, c in REFUSED_CASES]


def _wrong_shard_streams(env, name, coder):
    """shard A = the first tiles of a frame and its stream; plan B = the next tiles of the same frame (the same number of tiles: only the
    numbering says the stream is not B's).  Returns the plans, (H, bytes per row), [(what, plan, stream, its length, positions or None)]."""
    torch, orc, t2ref, ctx = env
    from j2kgfx.codec import FramePlan
    fmt, W, H, tile, lossless, count, fused = REFUSED_GEOMETRIES[name]
    if fmt == RGBA8:
        pix, Cn, prec = _rgba_of(ref.frame(W, H, 50 + coder, noise=12)), 3, 8
    else:
        pix, Cn, prec, _ = ref.pixel_frame(fmt, W, H, 50 + fmt, orc)
    kw = dict(precision=prec, lossless=lossless, quality=0 if lossless else 75, num_resolutions=4, cb=(32, 32), tile=(tile, tile), coder=coder,
              closed_loop=True, ctx=ctx)
    a = FramePlan(W, H, Cn, tile_first=0, tile_count=count, **kw)
    b = FramePlan(W, H, Cn, tile_first=count, tile_count=count, **kw)
    d_pix = torch.from_numpy(pix).to(a.device)
    cs, toffs = a.encode_frame_pixels(fmt, d_pix, sop=True, eph=True)
    a.frame_status()
    total = int(toffs[-1].item())
    good = torch.full_like(d_pix, SENTINEL)
    assert a.pixels_fused(fmt, good, inverse=True) == fused and b.pixels_fused(fmt, good, inverse=True) == fused
    a.decode_frame_pixels(cs, total, good, tile_offs=toffs, sop=True, eph=True)       # (the stream is sound: A takes it)
    a.frame_status()
    assert int((good[:64] != SENTINEL).sum().item()) > 32 * W
    cases = []
    for given in (True, False):
        cases.append(("another shard's plan", b, cs, total, toffs if given else None))
        for tile_no, byte in ((count - 1, 5), (0, 4)):
            bad = cs[:total].clone()
            at = int(toffs[tile_no].item()) + byte
            bad[at] = int(bad[at].item()) ^ 1                                       # one Isot byte changed on the host's side
            cases.append(("Isot byte %d of tile %d" % (byte, tile_no), a, bad, total, toffs if given else None))
    return (a, b), tuple(pix.shape), cases


@pytest.mark.parametrize("name,coder", REFUSED_CASES, ids=REFUSED_IDS)
def test_closed_loop_shard_stream_with_the_wrong_tile_numbers_is_invalid_arg(env, name, coder):
    """a shard's stream handed to a plan whose tile_first differs, or with one Isot byte changed: t2_tile_chain refuses the tile-part
    (J2K_ERR_INVALID_ARG); the calls are asynchronous, so the status is j2k_plan_frame_status's.  (An error path of the decoder: nothing faults.)"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import J2KError, _lib
    plans, shape, cases = _wrong_shard_streams(env, name, coder)
    for what, plan, stream, total, offs in cases:
        plan.decode_tile_parts(stream, total, tile_offs=offs, sop=True, eph=True)
        with pytest.raises(J2KError) as e:
            plan.frame_status()
        assert e.value.status == _lib.ERR_INVALID_ARG, (what, offs is not None)
        frame = torch.full(shape, SENTINEL, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(stream, total, frame, tile_offs=offs, sop=True, eph=True)
        with pytest.raises(J2KError) as e:
            plan.frame_status()
        assert e.value.status == _lib.ERR_INVALID_ARG, (what, offs is not None)
    for p in plans:
        p.close()


@pytest.mark.parametrize("name,coder", REFUSED_CASES, ids=REFUSED_IDS)
def test_closed_loop_shard_stream_with_the_wrong_tile_numbers_leaves_the_frame_alone(env, name, coder):
    """... and j2k_plan_decode_frame_pixels, having refused such a stream, has written nothing into the caller's frame -- although the calls are
    asynchronous and the block decoder and the inverse transform are queued behind the parse all the same: every launch that writes the
    caller's pixels looks at the plan's status word first.  Afterwards (the status read, which clears it) the plan decodes a sound stream as
    before.  (This test found the frame written: 382708 of the 384000 bytes of the first geometry.)"""
    torch, orc, t2ref, ctx = env
    from j2kgfx import J2KError
    plans, shape, cases = _wrong_shard_streams(env, name, coder)
    for what, plan, stream, total, offs in cases:
        frame = torch.full(shape, SENTINEL, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(stream, total, frame, tile_offs=offs, sop=True, eph=True)
        with pytest.raises(J2KError):
            plan.frame_status()
        touched = int((frame != SENTINEL).sum().item())
        assert touched == 0, (what, offs is not None, "bytes of the frame written", touched)
    # shard A's own stream on A once more
    what, a, stream, total, offs = cases[1]
    good = cases[0][2]
    frame = torch.full(shape, SENTINEL, dtype=torch.uint8, device=a.device)
    a.decode_frame_pixels(good, total, frame, tile_offs=cases[0][4], sop=True, eph=True)
    a.frame_status()
    assert int((frame[:64] != SENTINEL).sum().item()) > 32 * shape[1] // 2
    for p in plans:
        p.close()


# ---- (3) batch x packed pixels -------------------------------------------------------------------------------------------------------------------
def _stack_pix(orc, fmt, W, H, B, stride, seed):
    """B frames in pixel format fmt stacked: (pix [B * H, stride] with 0x3C between the rows, Cn, precision, planes [Cn, B * H, W])"""
    frames = [ref.pixel_frame(fmt, W, H, seed + b, orc, stride=stride, pad_byte=0x3C) for b in range(B)]
    return np.concatenate([f[0] for f in frames], axis=0), frames[0][1], frames[0][2], np.concatenate([f[3] for f in frames], axis=1)


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("fmt", list(ref.PIX_FORMATS), ids=["GRAY8", "GRAY16", "RGBA8", "RGBA64", "NRGBA8", "NRGBA64"])
def test_batch_of_packed_pixel_frames_every_format(env, fmt, tile):
    """forward_pixels / inverse_pixels on B = 3 stacked frames of an ODD height (frames 1 and 2 start at Pix rows 75 and 150: a tile's row
    parity is not the image's): coefficients equal the single-frame plans', the pixels come back and the bytes between the rows stay.  Rows
    as long as a row, rows 16-byte aligned and further apart, rows 4 bytes further apart (unaligned: staged); the level-0 kernels reading
    and writing the pixels themselves (J2K_PIX_FUSE = 1, where pixels_fused says so) and the int32 staging frame (J2K_PIX_FUSE = 0)."""
    torch, orc, t2ref, ctx0 = env
    from j2kgfx.codec import FramePlan
    W, H, B = 520, 75, 3
    row = W * BPP[fmt]
    seen = {0: set(), 1: set()}
    for fuse in (1, 0):
        with _ctx(J2K_PIX_FUSE=fuse) as ctx:
            for stride in (row, (row + 15) // 16 * 16 + 16, row + 4):
                pix, Cn, prec, planes = _stack_pix(orc, fmt, W, H, B, stride, 60 + fmt)
                kw = dict(precision=prec, lossless=True, num_resolutions=4, cb=(32, 32), tile=(tile, tile), coder=1, ctx=ctx)
                batch = FramePlan(W, H * B, Cn, frame_rows=H, **kw)
                d_pix = torch.from_numpy(pix).to(batch.device)
                out = torch.full((H * B, stride), SENTINEL, dtype=torch.uint8, device=batch.device)
                fused = (batch.pixels_fused(fmt, d_pix), batch.pixels_fused(fmt, out, inverse=True))
                seen[fuse].update(fused)
                if fuse == 0 or stride % 16:
                    assert fused == (False, False)
                co = batch.forward_pixels(fmt, d_pix)
                batch.inverse_pixels(co, out)
                batch.ctx.sync()
                h_co, h_out = co.cpu().numpy(), out.cpu().numpy()
                # the pixels back: createImage of the samples (8 bit: the source's bytes, alpha 255 where it is no component); pad bytes as they were
                assert np.array_equal(h_out[:, :row], orc.create_image([planes[c] for c in range(Cn)], prec)), (fuse, stride)
                if prec == 8:
                    assert np.array_equal(h_out[:, :row], pix[:, :row])
                assert (h_out[:, row:] == SENTINEL).all(), (fuse, stride)
                at = 0
                for b in range(B):
                    one = FramePlan(W, H, Cn, **kw)
                    d1 = torch.from_numpy(np.ascontiguousarray(pix[b * H:(b + 1) * H])).to(one.device)
                    assert (one.pixels_fused(fmt, d1), one.pixels_fused(fmt, out[:H], inverse=True)) == fused
                    c1 = one.forward_pixels(fmt, d1)
                    one.ctx.sync()
                    ne = int(one.info.coeff_elems)
                    d = np.nonzero(h_co[at:at + ne] != c1.cpu().numpy()[:ne])[0]
                    assert d.size == 0, ("coefficients", fuse, stride, b, int(d[0]))
                    at += ne
                    one.close()
                assert at == int(batch.info.coeff_elems)
                # and against the oracle: frame 1's first tile (it starts at an odd Pix row)
                tw, th = (tile or W), min(tile or H, H)
                want = orc.preprocess([np.ascontiguousarray(planes[c, H:H + th, :tw]) for c in range(Cn)], tw, th, prec, True, 4)
                rows = batch.planes()
                t0 = _tiles_per_frame(W, H, tile)
                for c in range(Cn):
                    r = rows[t0 * Cn + c]
                    assert (int(r[0]), int(r[1]), int(r[2]), int(r[3])) == (t0, c, 0, H)
                    assert np.array_equal(h_co[int(r[6]):int(r[6]) + tw * th].reshape(th, tw), want[c]), (fuse, stride, c)
                batch.close()
    assert seen[0] == {False}
    if tile == 0:
        assert seen[1] == {False, True}       # (520 columns, untiled, aligned rows: every format is fused, tests/test_gpu_pixels.py pins it; row + 4 never is)


@pytest.mark.parametrize("fmt,W,H,tile,pad", [(RGBA8, 1024, 150, 512, 0), (RGBA8, 512, 75, 0, 32), (GRAY8, 1024, 100, 512, 0), (GRAY8, 512, 77, 0, 16)],
                         ids=["rgba8-tile512", "rgba8-untiled-odd-padded", "gray8-tile512", "gray8-untiled-odd-padded"])
def test_batch_of_packed_pixel_frames_lossy(env, fmt, W, H, tile, pad):
    """image.RGBA and image.Gray through the lossy path (ICT + 9-7 + quantisation; the workgroup level-0 kernels read and write the pixels) as
    B = 2 stacked frames: coefficients and pixels back equal the single-frame plans', pad bytes stay"""
    torch, orc, t2ref, ctx = env
    from j2kgfx.codec import FramePlan
    B = 2
    row = W * BPP[fmt]
    stride = row + pad
    Cn = 3 if fmt == RGBA8 else 1
    rng = np.random.default_rng(W + H + fmt)
    pix = rng.integers(0, 256, (H * B, stride)).astype(np.uint8)
    pix[:, 0:row:BPP[fmt]] = np.clip(np.arange(W) * 255 // W + rng.integers(-9, 10, (H * B, W)), 0, 255)      # something smoother in the first channel
    kw = dict(precision=8, lossless=False, quality=75, num_resolutions=4, cb=(64, 64), tile=(tile, tile), coder=0 if fmt == RGBA8 else 1, ctx=ctx)
    batch = FramePlan(W, H * B, Cn, frame_rows=H, **kw)
    d_pix = torch.from_numpy(pix).to(batch.device)
    out = torch.full((H * B, stride), SENTINEL, dtype=torch.uint8, device=batch.device)
    fused = (batch.pixels_fused(fmt, d_pix), batch.pixels_fused(fmt, out, inverse=True))
    assert fused == (True, True)              # (aligned rows, planes of 512 columns: tests/test_gpu_pixels.py pins these geometries for one frame)
    co = batch.forward_pixels(fmt, d_pix)
    batch.inverse_pixels(co, out)
    batch.ctx.sync()
    h_co, h_out = co.cpu().numpy(), out.cpu().numpy()
    assert (h_out[:, row:] == SENTINEL).all()
    at = 0
    for b in range(B):
        one = FramePlan(W, H, Cn, **kw)
        d1 = torch.from_numpy(np.ascontiguousarray(pix[b * H:(b + 1) * H])).to(one.device)
        o1 = torch.full((H, stride), SENTINEL, dtype=torch.uint8, device=one.device)
        assert (one.pixels_fused(fmt, d1), one.pixels_fused(fmt, o1, inverse=True)) == fused
        c1 = one.forward_pixels(fmt, d1)
        one.inverse_pixels(c1, o1)
        # ... and the planar path of the same plan on the oracle's planes
        planes = np.stack(orc.extract_image_data(pix[b * H:(b + 1) * H], fmt, W, H, 8))
        c2 = one.forward(torch.from_numpy(planes).to(one.device))
        one.ctx.sync()
        ne = int(one.info.coeff_elems)
        assert np.array_equal(h_co[at:at + ne], c1.cpu().numpy()[:ne]) and torch.equal(c1[:ne], c2[:ne]), ("coefficients", b)
        assert np.array_equal(h_out[b * H:(b + 1) * H], o1.cpu().numpy()), ("pixels back", b)
        at += ne
        one.close()
    batch.close()


# ---- (4) batch x the kernels that the plan's geometry selects ------------------------------------------------------------------------------------
def _rgba8_batch_against_frames(torch, orc, ctx, W, H, B, seed):
    """packed RGBA8, 512 x 512 tiles, 5-3, six resolutions: forward_rgba8 / inverse_rgba8 of B stacked frames against the frames one by one on
    the same context; the inverse also on full-range int32 coefficients (a decoder's input is arbitrary).  Returns the batch's coefficients."""
    from j2kgfx.codec import FramePlan
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, 256, (H * B, W * 4)).astype(np.uint8)
    pix.reshape(H * B, W, 4)[..., 3] = 255
    kw = dict(precision=8, lossless=True, num_resolutions=6, cb=(64, 64), tile=(512, 512), coder=1, ctx=ctx)
    batch = FramePlan(W, H * B, 3, frame_rows=H, **kw)
    ne = int(batch.info.coeff_elems)
    junk = rng.integers(-2 ** 31, 2 ** 31, batch.alloc_coeff().numel(), dtype=np.int64).astype(np.int32)
    d_pix = torch.from_numpy(pix).to(batch.device)
    for rep in range(2):                              # (the second pass starts on an idle device)
        co = batch.forward_rgba8(d_pix)
        back = batch.inverse_rgba8(co)
        back2 = batch.inverse_rgba8(torch.from_numpy(junk).to(batch.device))
        batch.ctx.sync()
        assert np.array_equal(back.cpu().numpy(), pix), rep
    h_co, h_b2 = co.cpu().numpy(), back2.cpu().numpy()
    ne1 = ne // B
    for b in range(B):
        one = FramePlan(W, H, 3, **kw)
        assert int(one.info.coeff_elems) == ne1 and int(one.info.planes) * B == int(batch.info.planes)
        c1 = one.forward_rgba8(torch.from_numpy(np.ascontiguousarray(pix[b * H:(b + 1) * H])).to(one.device))
        j1 = torch.zeros(one.alloc_coeff().numel(), dtype=torch.int32)
        j1[:ne1] = torch.from_numpy(junk[b * ne1:(b + 1) * ne1])
        k1 = one.inverse_rgba8(j1.to(one.device))
        one.ctx.sync()
        d = np.nonzero(h_co[b * ne1:(b + 1) * ne1] != c1.cpu().numpy()[:ne1])[0]
        assert d.size == 0, ("coefficients", b, int(d[0]))
        bad = np.argwhere(h_b2[b * H:(b + 1) * H] != k1.cpu().numpy())
        assert bad.size == 0, ("inverse of arbitrary coefficients (row, byte)", b, bad[0].tolist())
        one.close()
    # frame 0's top-left tile against the oracle's pipeline on the cropped image
    tw, th = min(512, W), min(512, H)
    crop = np.ascontiguousarray(pix.reshape(H * B, W, 4)[:th, :tw].reshape(th, tw * 4))
    want = orc.preprocess(orc.extract_image_data(crop, RGBA8, tw, th), tw, th, 8, True, 6)
    for c in range(3):
        assert np.array_equal(h_co[c * tw * th:(c + 1) * tw * th].reshape(th, tw), want[c]), c
    tc = int(batch.info.planes)
    batch.close()
    return tc


@pytest.mark.parametrize("W,H,B,environ", [(512, 520, 2, {}), (1280, 624, 3, {}), (512, 520, 2, {"J2K_DEEP": 0}), (512, 520, 2, {"J2K_MEGA": 1}),
                                          (512, 520, 2, {"J2K_MEGA": 2}), (512, 520, 2, {"J2K_L0_WG": 0}), (512, 520, 2, {"J2K_L0_FUSE": 8})],
                         ids=["512x520x2", "1280x624x3", "deep0", "mega1", "mega2", "l0wg0", "l0fuse8"])
def test_batch_rgba8_512_tiles_where_only_the_batch_reaches_the_deep_kernels(env, W, H, B, environ):
    """deep_min_planes = 12 (left alone on purpose): two 512 x 520 frames are 2 x 2 x 3 = 12 tile-components, so the BATCH takes the
    one-launch deep 5-3 kernels -- with an 8-row ragged tile among its planes -- while each frame alone (6) stays on per-level launches: two
    different sets of kernels, the same coefficients and pixels.  Also three 1280 x 624 frames (256-column and 112-row edge tiles), and the
    first shape with the deep kernels off, both merged-launch forms, the general level-0 kernels, and level 1 fused into level 0."""
    torch, orc, t2ref, ctx0 = env
    with _ctx(**environ) as ctx:
        tc = _rgba8_batch_against_frames(torch, orc, ctx, W, H, B, W + H + B)
    if (W, H, B) == (512, 520, 2):
        assert tc // B < 12 <= tc                      # tile-components: the batch is over deep_min_planes, a frame alone is not


@pytest.mark.parametrize("environ", [{"J2K_L0_WG97": 0}, {"J2K_L0_WG97": 8}, {"J2K_L0_WG97_INV": 0}, {"J2K_L0_WG97_INV": 8}, {"J2K_PLANE_WG97": 0},
                                     {"J2K_PLANE_WG97": 8}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_batch_lossy_rgb12_512_tiles(env, environ):
    """bench.py --config c3's kind at a small size: B = 2 frames of 1024 x 300, 3 x 12 bit, ICT + 9-7 + quantiser, 512 x 512 tiles.  forward, and
    inverse from arbitrary int32 coefficients, equal the single-frame plans' -- workgroup and general kernels of level 0 (both directions) and
    of the deeper levels"""
    torch, orc, t2ref, ctx0 = env
    from j2kgfx.codec import FramePlan
    W, H, B = 1024, 300, 2
    rng = np.random.default_rng(97)
    frame = rng.integers(0, 4096, (3, H * B, W)).astype(np.int32)
    with _ctx(**environ) as ctx:
        kw = dict(precision=12, lossless=False, quality=75, num_resolutions=6, cb=(64, 64), tile=(512, 512), coder=0, ctx=ctx)
        batch = FramePlan(W, H * B, 3, frame_rows=H, **kw)
        ne1 = int(batch.info.coeff_elems) // B
        junk = rng.integers(-(1 << 20), 1 << 20, batch.alloc_coeff().numel()).astype(np.int32)
        co = batch.forward(torch.from_numpy(frame).to(batch.device))
        back = batch.inverse(torch.from_numpy(junk).to(batch.device))
        batch.ctx.sync()
        h_co, h_back = co.cpu().numpy(), back.cpu().numpy().reshape(3, H * B, W)
        for b in range(B):
            one = FramePlan(W, H, 3, **kw)
            assert int(one.info.coeff_elems) == ne1
            c1 = one.forward(torch.from_numpy(np.ascontiguousarray(frame[:, b * H:(b + 1) * H])).to(one.device))
            j1 = torch.zeros(one.alloc_coeff().numel(), dtype=torch.int32)
            j1[:ne1] = torch.from_numpy(junk[b * ne1:(b + 1) * ne1])
            k1 = one.inverse(j1.to(one.device))
            one.ctx.sync()
            d = np.nonzero(h_co[b * ne1:(b + 1) * ne1] != c1.cpu().numpy()[:ne1])[0]
            assert d.size == 0, ("coefficients", b, int(d[0]))
            bad = np.argwhere(h_back[:, b * H:(b + 1) * H] != k1.cpu().numpy().reshape(3, H, W))
            assert bad.size == 0, ("inverse of arbitrary coefficients (component, row, column)", b, bad[0].tolist())
            one.close()
        # frame 1's first tile against the oracle's preprocess
        want = orc.preprocess([np.ascontiguousarray(frame[c, H:2 * H, :512]) for c in range(3)], 512, H, 12, False, 6, 75)
        rows = batch.planes()
        for c in range(3):
            r = rows[2 * 3 + c]
            assert (int(r[0]), int(r[1]), int(r[2]), int(r[3])) == (2, c, 0, H)
            assert np.array_equal(h_co[int(r[6]):int(r[6]) + 512 * H].reshape(H, 512), want[c]), c
        batch.close()


@pytest.mark.parametrize("wg", [0, 4, 8])
def test_batch_gray16_untiled_frames(env, wg):
    """bench.py --config c5's kind at a small size: B = 4 image.Gray16 frames of 1024 x 130, untiled, 5-3, through forward_pixels /
    inverse_pixels -- the general single-component kernels and the workgroup forms of 4 and 8 waves"""
    torch, orc, t2ref, ctx0 = env
    from j2kgfx.codec import FramePlan
    W, H, B = 1024, 130, 4
    pix, Cn, prec, planes = _stack_pix(orc, GRAY16, W, H, B, W * 2, 500)
    assert (Cn, prec) == (1, 16)
    with _ctx(J2K_PLANE_WG=wg) as ctx:
        kw = dict(precision=16, lossless=True, num_resolutions=6, cb=(64, 64), coder=0, ctx=ctx)
        batch = FramePlan(W, H * B, 1, frame_rows=H, **kw)
        d_pix = torch.from_numpy(pix).to(batch.device)
        co = batch.forward_pixels(GRAY16, d_pix)
        out = batch.inverse_pixels(co, torch.zeros_like(d_pix))
        samples = batch.inverse(co)
        batch.ctx.sync()
        assert np.array_equal(samples.cpu().numpy().reshape(1, H * B, W), planes)
        assert np.array_equal(out.cpu().numpy(), orc.create_image([planes[0]], 16))
        h_co = co.cpu().numpy()
        ne1 = int(batch.info.coeff_elems) // B
        for b in range(B):
            one = FramePlan(W, H, 1, **kw)
            c1 = one.forward_pixels(GRAY16, torch.from_numpy(np.ascontiguousarray(pix[b * H:(b + 1) * H])).to(one.device))
            one.ctx.sync()
            d = np.nonzero(h_co[b * ne1:(b + 1) * ne1] != c1.cpu().numpy()[:ne1])[0]
            assert d.size == 0, ("coefficients", b, int(d[0]))
            one.close()
        want = orc.preprocess([np.ascontiguousarray(planes[0, 3 * H:4 * H])], W, H, 16, True, 6)
        assert np.array_equal(h_co[3 * ne1:4 * ne1].reshape(H, W), want[0])
        batch.close()


# ---- (5) batch x image sources -------------------------------------------------------------------------------------------------------------------
def _dev(torch, a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.mark.parametrize("ratio", [2, 1], ids=["420", "422"])
@pytest.mark.parametrize("W,H,B,tile,fused", [(64, 37, 3, 32, False), (512, 37, 2, 512, True)], ids=["64x37x3", "512x37x2-fused"])
def test_batch_of_ycbcr_frames_with_an_odd_frame_height(env, W, H, B, tile, fused, ratio):
    """One image.YCbCr of B x 37 rows as a batch (j2k_plan_image_fused takes img->height == the plan's): with 4:2:0 the chroma row of Pix row
    37 -- frame 1's first -- is the one of row 36, frame 0's last, so a tile's row parity is not the image's.  forward_image equals
    forward_rgba8 of image_to_rgba8 of the same image (the module's own identity), that frame is what tests/go_image_ref.py restates
    without the library, and the coefficients are those of the frames' rows one by one; 512-column tiles take the fused YCbCr kernel."""
    torch, orc, t2ref, ctx = env
    from j2kgfx.codec import FramePlan
    from j2kgfx.pixels import YCbCr, image_to_rgba8
    rng = np.random.default_rng(W + ratio)
    rect = (0, 0, W, H * B)
    y, cb, cr, ys, cs = goref.random_ycbcr(rng, ratio, rect)
    want_rgba = goref.rgba8_frame(goref.ycbcr_image_rgb(y, cb, cr, ys, cs, ratio, rect))
    kw = dict(precision=8, lossless=True, num_resolutions=4, cb=(32, 32), tile=(tile, tile), coder=1, ctx=ctx)
    batch = FramePlan(W, H * B, 3, frame_rows=H, **kw)
    dimg = YCbCr(_dev(torch, y, batch.device), _dev(torch, cb, batch.device), _dev(torch, cr, batch.device), ys, cs, ratio, rect)
    if fused:
        assert batch.image_fused(dimg)
    rgba = image_to_rgba8(dimg, ctx=ctx)
    assert np.array_equal(rgba.cpu().numpy(), want_rgba)
    got = batch.forward_image(dimg)
    same = batch.forward_rgba8(rgba)
    batch.ctx.sync()
    ne = int(batch.info.coeff_elems)
    d = torch.nonzero(got[:ne] != same[:ne])
    assert d.numel() == 0, ("forward_image != forward_rgba8", int(d[0]))
    h_co = got.cpu().numpy()
    ne1 = ne // B
    for b in range(B):
        one = FramePlan(W, H, 3, **kw)
        c1 = one.forward_rgba8(_dev(torch, want_rgba[b * H:(b + 1) * H], one.device))
        one.ctx.sync()
        d = np.nonzero(h_co[b * ne1:(b + 1) * ne1] != c1.cpu().numpy()[:ne1])[0]
        assert d.size == 0, ("coefficients of frame", b, int(d[0]))
        one.close()
    batch.close()


@pytest.mark.parametrize("coder", [0, 1], ids=["mq", "ht"])
def test_encode_frame_image_on_a_closed_loop_batch(env, coder):
    """j2k_plan_encode_frame_image on a closed-loop batch of B = 2 YCbCr 4:2:0 frames of 512 x 37 (the fused source): the stream of
    encode_frame_pixels of the converted frame, and (MQ) it decodes to the restated colours"""
    torch, orc, t2ref, ctx = env
    from j2kgfx.codec import FramePlan
    from j2kgfx.pixels import YCbCr
    W, H, B = 512, 37, 2
    rng = np.random.default_rng(3 + coder)
    rect = (0, 0, W, H * B)
    cw, ch = goref.chroma_dims(2, rect)
    yy, xx = np.mgrid[0:H * B, 0:W]
    content = (np.clip(xx // 3 + yy + rng.integers(-6, 7, (H * B, W)), 0, 255), np.clip(128 + rng.integers(-20, 21, (ch, cw)), 0, 255),
               np.clip(100 + rng.integers(-20, 21, (ch, cw)), 0, 255))                  # (smooth enough for the reference's HT encoder)
    (y, cb, cr), spans, ys, cs = goref.ycbcr_layout(rng, 2, rect, content=content)
    want_rgba = goref.rgba8_frame(goref.ycbcr_image_rgb(y, cb, cr, ys, cs, 2, rect))
    plan = FramePlan(W, H * B, 3, precision=8, lossless=True, num_resolutions=4, cb=(64, 64), tile=(512, 512), coder=coder, closed_loop=True, frame_rows=H, ctx=ctx)
    dimg = YCbCr(_dev(torch, y, plan.device), _dev(torch, cb, plan.device), _dev(torch, cr, plan.device), ys, cs, 2, rect)
    assert plan.image_fused(dimg) and int(plan.info.tiles) == B
    out1, to1 = plan.encode_frame_pixels(RGBA8, _dev(torch, want_rgba, plan.device), sop=True, eph=True)
    plan.frame_status()
    out2, to2 = plan.encode_frame_image(dimg, sop=True, eph=True)
    plan.frame_status()
    n = int(to1[-1].item())
    assert torch.equal(to1, to2) and torch.equal(out1[:n], out2[:n])
    assert [int(out2[int(to2[k].item()) + 5].item()) for k in range(B)] == [0, 1]
    back = torch.zeros((H * B, W * 4), dtype=torch.uint8, device=plan.device)
    plan.decode_frame_pixels(out2, n, back, sop=True, eph=True)
    plan.frame_status()
    if coder == 0:
        assert np.array_equal(back.cpu().numpy(), want_rgba)
    plan.close()


# ---- (6) one graph replay ------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_batch_frame_calls_replay_from_a_hip_graph(env):
    """a closed-loop batch plan (B = 2 frames of 200 x 150, ragged 128-tiles, MQ coder): encode_frame_pixels + decode_frame_pixels run once,
    are captured, and replayed twice on new pixels in the same buffers -- the direct calls' stream and pixels.  (The one-kernel HT path is
    refused under capture by design: MQ only.)"""
    torch, orc, t2ref, ctx = env
    from j2kgfx.codec import FramePlan
    W, H, B = 200, 150, 2

    def pixels(seed):
        return torch.from_numpy(_rgba_of(np.concatenate([ref.frame(W, H, seed + b, noise=5 + 4 * b) for b in range(B)], axis=1)))
    plan = FramePlan(W, H * B, 3, precision=8, lossless=True, num_resolutions=4, cb=(32, 32), tile=(128, 128), coder=0, closed_loop=True, frame_rows=H, ctx=ctx)
    tiles = int(plan.info.tiles)
    assert tiles == B * 4
    d_pix = pixels(70).to(plan.device)
    back = torch.zeros_like(d_pix)
    cs = plan.empty(plan.frame_bound(), torch.uint8)
    toffs = plan.empty(tiles + 1, torch.int64)[:tiles + 1]

    def code():
        plan.encode_frame_pixels(RGBA8, d_pix, True, True, cs, toffs)
        plan.decode_frame_pixels(cs, cs.numel(), back, toffs, True, True)
    code()
    plan.frame_status()
    assert torch.equal(back, d_pix)
    with ctx.capture() as g:
        code()
    for seed in (80, 90):
        d_pix.copy_(pixels(seed).to(plan.device))
        torch.cuda.synchronize()
        back.zero_()
        cs.zero_()
        g.launch()
        plan.frame_status()
        got, cs_g, t_g = back.clone(), cs.clone(), toffs.clone()
        back.zero_()
        code()
        plan.frame_status()
        n = int(toffs[-1].item())
        assert torch.equal(t_g, toffs) and torch.equal(cs[:n], cs_g[:n]) and torch.equal(back, got), seed
        assert torch.equal(got, d_pix), seed
        assert [int(cs_g[int(t_g[k].item()) + 5].item()) for k in range(tiles)] == list(range(tiles))
    g.close()
    plan.close()
