"""The closed-loop frame by the ORACLE (test infrastructure): the reference's own functions composed per tile -- preprocess (DC shift, RCT, 5-3),
the job list with partitioning windows, the block coder, one packet per (component, resolution) through the restated PacketEncoder with the
closed-loop flags, createTileHeader.  Used by tests/test_gpu_decode_body.py, tests/test_gpu_closed_loop_formats.py, tests/test_gpu_batch_shard_paths.py, tests/test_closed_loop_golden.py, tools/fuzz_gpu_closed_loop.py and tests/golden/make_closed_loop_golden.py."""
import numpy as np


def frame(W, H, seed, noise=16):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.stack([xx * 255 // W, yy * 255 // H, (xx + yy) * 127 // max(W, H)]) + rng.integers(-noise, noise + 1, (3, H, W))
    return np.clip(f, 0, 255).astype(np.uint8)


def frame_n(W, H, Cn, prec, seed, noise=None):
    """Cn components at `prec` bits: gradients over the whole range plus noise (default: a sixteenth of the range, so that the high bit
    planes of the detail bands are in use), int32 [Cn, H, W]"""
    rng = np.random.default_rng(seed)
    top = (1 << prec) - 1
    noise = top // 16 if noise is None else noise
    yy, xx = np.mgrid[0:H, 0:W]
    grads = [xx * top // W, yy * top // H, (xx + yy) * (top // 2) // max(W, H), (W - 1 - xx + yy) * (top // 2) // max(W, H)]
    f = np.stack([grads[c % 4] for c in range(Cn)]) + rng.integers(-noise, noise + 1, (Cn, H, W))
    return np.clip(f, 0, top).astype(np.int32)


def flat_spike(W, H, Cn, prec):
    """mid-grey with one full-scale sample per component: all-zero bands, empty packets (the contents of ht_flat_empty_packets at any depth)"""
    f = np.full((Cn, H, W), 1 << (prec - 1), np.int32)
    f[:, H // 2, W // 3] = (1 << prec) - 1
    return f


# the six Go image types of encoder.extractImageData, by the library's constants J2K_PIX_GRAY8 ... J2K_PIX_NRGBA64 (include/j2kgfx.h)
PIX_FORMATS = (0, 1, 2, 3, 4, 5)


def pixel_frame(fmt, W, H, seed, orc, stride=None, pad_byte=0, noise=None, flat=False):
    """A packed frame in the Go Pix layout of pixel format `fmt`, by the oracle alone: createImage writes the layout (decoder.go:417-588),
    extractImageData reads it back (encoder.go:79-213) and says how many components at which precision an encoder sees in it.
    Returns (pix uint8 [H, stride], Cn, precision, planes int32 [Cn, H, W]); bytes between rows hold pad_byte; flat: flat_spike instead of frame_n."""
    probe = orc.extract_image_data(np.zeros((1, 8), np.uint8), fmt, 1, 1)
    Cn = len(probe)
    prec = 16 if int(orc.extract_image_data(np.full((1, 8), 255, np.uint8), fmt, 1, 1)[0][0, 0]) > 255 else 8
    vals = flat_spike(W, H, Cn, prec) if flat else frame_n(W, H, Cn, prec, seed, noise)
    # (16 bit: createImage's v * 65535 / 65535 wraps in int32 above 32768, decoder.go:434-451 -- the samples it writes are then not `vals`, but they
    # are samples over the whole range in the right layout all the same; what the frame holds is what extractImageData reads, below)
    tight = orc.create_image([vals[c] for c in range(Cn)], prec)
    row = tight.shape[1]
    stride = stride or row
    assert stride >= row
    pix = np.full((H, stride), pad_byte, np.uint8)
    pix[:, :row] = tight
    planes = np.stack(orc.extract_image_data(pix, fmt, W, H))
    assert planes.shape == (Cn, H, W) and (prec == 16 or np.array_equal(planes, vals))
    return pix, Cn, prec, planes


def oracle_frame(frm, W, H, tw, th, nres, cb, coder, sop, eph, orc, t2ref, tiles=None, precision=8, lossless=True, quality=0):
    """Returns per tile: dict(coeff, bytes, lens, numbps, part, w, h, x0, y0).  frm: [components, H, W] at `precision` bits; lossless = False:
    ICT + 9-7 + the encoder's quantiser at `quality` (encoder.preprocess), the block coder on the quantised coefficients."""
    out = {}
    tx_n, ty_n = (W + tw - 1) // tw, (H + th - 1) // th
    for t in range(tx_n * ty_n):
        if tiles is not None and t not in tiles:
            continue
        tx, ty = t % tx_n, t // tx_n
        x0, y0 = tx * tw, ty * th
        w, h = min(tw, W - x0), min(th, H - y0)
        sub = [np.ascontiguousarray(frm[c, y0:y0 + h, x0:x0 + w]).astype(np.int32) for c in range(frm.shape[0])]
        coeff = orc.preprocess(sub, w, h, precision, lossless, nres, quality)
        by, lens, nb = orc.encode_tile_blocks(coeff, w, h, nres, cb, cb, coder, windows=1)
        jobs = orc.enumerate_blocks(len(sub), w, h, nres, cb, cb, 1)
        enc = t2ref.PacketEncoder(len_bits=5)
        pos, j = 0, 0
        while j < len(jobs):
            k = j
            blocks = []
            while k < len(jobs) and jobs[k]["comp"] == jobs[j]["comp"] and jobs[k]["res"] == jobs[j]["res"]:
                ln, n_b = int(lens[k]), int(nb[k])
                blocks.append(t2ref.CodeBlock(bytes(by[pos:pos + ln]), 1 if ln == 0 else 0, max(31 - n_b, 0), 0 if n_b == 0 else (1 if coder == 1 else 3 * n_b - 2)))
                pos += ln
                k += 1
            enc.encode_packet(t2ref.Precinct([blocks]), 0, sop, eph)
            j = k
        out[t] = dict(coeff=coeff, bytes=by, lens=lens, numbps=nb, part=orc.create_tile_header(t, bytes(enc.out)), w=w, h=h, x0=x0, y0=y0)
    return out


def oracle_batch(frames, W, H, tw, th, nres, cb, coder, sop, eph, orc, t2ref, **kw):
    """A batch plan's tile-parts (j2k_params.frame_rows: the tile grid starts again at every frame, the tiles are numbered through the
    batch) by the oracle: oracle_frame once per frame of `frames` ([components, H, W] each), frame 0's tiles first, every tile-part made
    again by createTileHeader at index b * tiles_per_frame + t around the packets of tile t of frame b.  Returns a list of oracle_frame's
    dicts in batch order, each with frame = b, tile = t, index = its number in the batch, and `part` the tile-part at that number."""
    out = []
    tiles1 = ((W + tw - 1) // tw) * ((H + th - 1) // th)
    for b, frm in enumerate(frames):
        want = oracle_frame(frm, W, H, tw, th, nres, cb, coder, sop, eph, orc, t2ref, **kw)
        assert sorted(want) == list(range(tiles1))
        for t in range(tiles1):
            k = b * tiles1 + t
            out.append(dict(want[t], frame=b, tile=t, index=k, part=orc.create_tile_header(k, want[t]["part"][14:])))
    return out


def check_every_stage(torch, orc, t2ref, ctx, frame, W, H, tw, th, nres, cb, coder, sop, eph, precision=8, want=None):
    """GPU: every stage of a lossless closed-loop plan against the oracle's composition, each where it first can differ -- job windows,
    block bytes, lengths, numBPS, tile-parts, parsed block tables, decoded + placed planes, the inverse.  frame: [components, H, W] at
    `precision` bits.  want: the oracle's frame if the caller has it (oracle_frame with the same arguments).  Returns dict(max_numbps,
    empty_blocks, blocks) of the oracle's tables, for the caller to assert that the case is the one it means to be."""
    from j2kgfx.codec import FramePlan
    Cn = frame.shape[0]
    plan = FramePlan(W, H, Cn, precision=precision, lossless=True, num_resolutions=nres, cb=(cb, cb), tile=(tw, th), coder=coder, ctx=ctx, closed_loop=True)
    if want is None:
        want = oracle_frame(frame, W, H, tw, th, nres, cb, coder, sop, eph, orc, t2ref, precision=precision)
    # job windows
    blocks = plan.blocks()
    planes = plan.planes()
    j = 0
    for t in sorted(want):
        jobs = orc.enumerate_blocks(Cn, want[t]["w"], want[t]["h"], nres, cb, cb, 1)
        for b in jobs:
            g = blocks[j]
            assert (int(planes[g["plane"]][0]), int(planes[g["plane"]][1]), g["band"], g["x0"], g["y0"], g["w"], g["h"]) == \
                (t, b["comp"], b["band"], b["x0"], b["y0"], b["w"], b["h"])
            j += 1
    assert j == len(blocks)
    # forward + block coder
    d_frame = torch.from_numpy(frame.astype(np.int32)).to(plan.device)
    coeff = plan.forward(d_frame)
    stream, offs, lens, numbps = plan.encode_stream(coeff)
    cs, toffs = plan.encode_tile_parts(stream, offs, lens, numbps, sop=sop, eph=eph)
    plan.frame_status()
    h_lens, h_nb = lens.cpu().numpy(), numbps.cpu().numpy()
    h_stream = stream.cpu().numpy()[:int(offs[-1].item())]
    want_lens = np.concatenate([want[t]["lens"] for t in sorted(want)])
    want_nb = np.concatenate([want[t]["numbps"] for t in sorted(want)])
    assert np.array_equal(h_lens[:len(blocks)].astype(np.uint32), want_lens)
    assert bytes(h_stream) == b"".join(bytes(want[t]["bytes"]) for t in sorted(want))
    coded = want_lens > 0
    assert np.array_equal(h_nb[:len(blocks)][coded], want_nb[coded])       # (a block without bytes has no bit planes to speak of: the packet says "not included")
    h_toffs = toffs.cpu().numpy()
    h_cs = cs.cpu().numpy()
    for i, t in enumerate(sorted(want)):
        assert bytes(h_cs[int(h_toffs[i]):int(h_toffs[i + 1])]) == want[t]["part"], t
    total = int(h_toffs[-1])
    # parse: the block tables point into the tile-parts
    offs2, lens2, nb2 = plan.decode_tile_parts(cs, total, tile_offs=None, sop=sop, eph=eph)
    plan.frame_status()
    o2, l2, n2 = offs2.cpu().numpy(), lens2.cpu().numpy(), nb2.cpu().numpy()
    assert np.array_equal(l2[:len(blocks)], h_lens[:len(blocks)])
    pos = 0
    for k in range(len(blocks)):
        ln = int(l2[k])
        if ln:
            assert bytes(h_cs[int(o2[k]):int(o2[k]) + ln]) == bytes(h_stream[pos:pos + ln]), k
            assert int(n2[k]) == int(h_nb[k])
        else:
            assert int(n2[k]) == 0
        pos += ln
    # block decode + placement against DecodeCodeBlock for every job of the oracle's list
    decoded = plan.decode_blocks(cs, offs2, lens2, nb2)
    placed = plan.place_blocks(decoded)
    back = plan.inverse(placed)
    ctx.sync()
    hp, hb = placed.cpu().numpy(), back.cpu().numpy()
    for t in sorted(want):
        wt = want[t]
        ref_planes = orc.decode_tile_blocks(wt["bytes"], wt["lens"], wt["numbps"], Cn, wt["w"], wt["h"], nres, cb, cb, coder, 1)
        for c in range(Cn):
            row = [r for r in planes if int(r[0]) == t and int(r[1]) == c][0]
            got = hp[int(row[6]):int(row[6]) + wt["w"] * wt["h"]].reshape(wt["h"], wt["w"])
            assert np.array_equal(got, ref_planes[c]), (t, c)
            if coder == 0:
                assert np.array_equal(got, wt["coeff"][c])        # the MQ coder is lossless: the coefficients come back
        sub = [orc.reconstruct53(ref_planes[c], wt["w"], wt["h"], nres - 1) for c in range(Cn)]
        px = orc.postprocess(sub, precision, True)
        for c in range(Cn):
            assert np.array_equal(hb[c, wt["y0"]:wt["y0"] + wt["h"], wt["x0"]:wt["x0"] + wt["w"]], px[c]), (t, c)
    if coder == 0:
        assert np.array_equal(hb, frame.astype(np.int32))
    plan.close()
    return dict(max_numbps=int(want_nb.max()), empty_blocks=int((~coded).sum()), blocks=len(blocks))


# the frames whose closed-loop tile-parts are pinned by digest (tests/golden/closed_loop_v1.json)
GOLDEN_CASES = [
    dict(name="mq_ragged_sop_eph", W=97, H=70, tile=(32, 48), cb=8, nres=3, coder=0, sop=True, eph=True, seed=201, noise=20),
    dict(name="ht_ragged_sop_eph", W=97, H=70, tile=(32, 48), cb=8, nres=3, coder=1, sop=True, eph=True, seed=202, noise=6),
    dict(name="mq_one_tile_bare", W=64, H=64, tile=(64, 64), cb=16, nres=4, coder=0, sop=False, eph=False, seed=203, noise=40),
    dict(name="ht_flat_empty_packets", W=80, H=48, tile=(40, 48), cb=16, nres=3, coder=1, sop=True, eph=False, seed=204, noise=0),
]

# ... and beyond 8-bit RGB (tests/golden/closed_loop_v2.json): one and four components, 12 and 16 bit (comps / prec; frames by frame_n)
GOLDEN_CASES_V2 = [
    dict(name="gray16_mq_ragged_sop", W=97, H=70, tile=(32, 48), cb=8, nres=3, coder=0, sop=True, eph=False, seed=211, noise=None, comps=1, prec=16),
    dict(name="gray8_ht_ragged_eph", W=97, H=70, tile=(48, 32), cb=16, nres=3, coder=1, sop=False, eph=True, seed=212, noise=5, comps=1, prec=8),
    dict(name="rgb12_mq_ragged_sop_eph", W=75, H=52, tile=(32, 32), cb=8, nres=4, coder=0, sop=True, eph=True, seed=213, noise=None, comps=3, prec=12),
    dict(name="four8_ht_ragged_bare", W=70, H=45, tile=(40, 24), cb=8, nres=3, coder=1, sop=False, eph=False, seed=214, noise=6, comps=4, prec=8),
]
GOLDEN_FILES = {"closed_loop_v1.json": GOLDEN_CASES, "closed_loop_v2.json": GOLDEN_CASES_V2}


def golden_frame(case):
    if "comps" in case:
        return frame_n(case["W"], case["H"], case["comps"], case["prec"], case["seed"], case["noise"])
    frm = frame(case["W"], case["H"], case["seed"], noise=case["noise"])
    if case["noise"] == 0:
        frm = np.full_like(frm, 128)
        frm[:, case["H"] // 2, case["W"] // 3] = 255
    return frm


def golden_stream(case, orc, t2ref):
    """the frame of a golden case and its tile-parts end to end, by the oracle"""
    frm = golden_frame(case)
    want = oracle_frame(frm, case["W"], case["H"], case["tile"][0], case["tile"][1], case["nres"], case["cb"], case["coder"], case["sop"], case["eph"], orc, t2ref,
                        precision=case.get("prec", 8))
    return frm, b"".join(want[t]["part"] for t in sorted(want))
