"""The closed-loop mode is this library's own stream format (no reference behaviour to be equal to): its tile-parts for
four small 8-bit RGB frames are pinned by digest in tests/golden/closed_loop_v1.json, and for four frames beyond that (Gray16 MQ, Gray8 HT,
3 x 12-bit MQ, four components HT) in closed_loop_v2.json (both written by tests/golden/make_closed_loop_golden.py from the oracle's
composition of the reference's functions).  CPU: the oracle still composes exactly those bytes, and the restated packet decoder reads
them back.  GPU: the product writes exactly those bytes -- stage calls and the one-call frame encoder -- and decodes them."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "go-jpeg2000_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import closed_loop_ref as ref  # noqa: E402

GOLDEN_BY_FILE = {name: json.load(open(os.path.join(HERE, "golden", name))) for name in ref.GOLDEN_FILES}
GOLDEN = {k: v for g in GOLDEN_BY_FILE.values() for k, v in g.items()}
ALL_CASES = [c for cases in ref.GOLDEN_FILES.values() for c in cases]


def test_golden_file_covers_the_cases():
    assert sorted(GOLDEN_BY_FILE) == ["closed_loop_v1.json", "closed_loop_v2.json"]
    for name, cases in ref.GOLDEN_FILES.items():
        assert sorted(GOLDEN_BY_FILE[name]) == sorted(c["name"] for c in cases)
    assert len(GOLDEN) == len(ALL_CASES) == 8


@pytest.mark.parametrize("case", ALL_CASES, ids=[c["name"] for c in ALL_CASES])
def test_oracle_composes_the_pinned_tile_parts_and_reads_them_back(case):
    import oracle as orc
    import t2ref
    frm, stream = ref.golden_stream(case, orc, t2ref)
    g = GOLDEN[case["name"]]
    assert len(stream) == g["bytes"] and stream[:24].hex() == g["head"]
    assert hashlib.sha256(stream).hexdigest() == g["sha256"]
    # read back with the restated PacketDecoder (closed-loop flags): every tile-part's packets give the block lengths that went in
    tw, th = case["tile"]
    want = ref.oracle_frame(frm, case["W"], case["H"], tw, th, case["nres"], case["cb"], case["coder"], case["sop"], case["eph"], orc, t2ref,
                            precision=case.get("prec", 8))
    at = 0
    for t in sorted(want):
        part = want[t]["part"]
        assert stream[at:at + len(part)] == part
        assert part[:2] == b"\xff\x90" and part[12:14] == b"\xff\x93" and int.from_bytes(part[6:10], "big") == len(part)
        jobs = orc.enumerate_blocks(frm.shape[0], want[t]["w"], want[t]["h"], case["nres"], case["cb"], case["cb"], 1)
        dec = t2ref.PacketDecoder(part[14:], len_bits=5, seated=True)
        j, got = 0, []
        while j < len(jobs):
            k = j
            while k < len(jobs) and jobs[k]["comp"] == jobs[j]["comp"] and jobs[k]["res"] == jobs[j]["res"]:
                k += 1
            blocks = [t2ref.CodeBlock(None, 0, 0, 0) for _ in range(k - j)]
            dec.decode_packet(t2ref.Precinct([blocks]), 0, case["sop"], case["eph"])
            got += [b.dlen() for b in blocks]
            j = k
        assert got == [int(x) for x in want[t]["lens"]], t
        at += len(part)
    assert at == len(stream)


def test_oracle_batch_renumbers_the_tile_parts_and_nothing_else():
    """closed_loop_ref.oracle_batch (what the batch tests on the GPU compare with): frame b's tile t is tile-part number b * tiles + t of the
    batch, made by the oracle's createTileHeader around the same packets -- it differs from the part at number t (oracle_frame's) in bytes 4
    and 5 only, Isot, which hold the number big-endian.  The same frame three times over, so that part k of the batch and part k % tiles of
    the frame wrap the same packets."""
    import oracle as orc
    import t2ref
    W, H, tw, th, nres, cb = 75, 52, 32, 32, 3, 8
    frm = ref.frame_n(W, H, 3, 8, 77)
    one = ref.oracle_frame(frm, W, H, tw, th, nres, cb, 0, True, True, orc, t2ref)
    tiles = len(one)
    assert tiles == 6
    got = ref.oracle_batch([frm, frm, frm], W, H, tw, th, nres, cb, 0, True, True, orc, t2ref)
    assert [(g["frame"], g["tile"], g["index"]) for g in got] == [(k // tiles, k % tiles, k) for k in range(3 * tiles)]
    for k, g in enumerate(got):
        a, b = np.frombuffer(one[k % tiles]["part"], np.uint8), np.frombuffer(g["part"], np.uint8)
        assert a.size == b.size
        differ = set(np.nonzero(a != b)[0].tolist())
        assert differ <= {4, 5}, (k, sorted(differ))
        assert int.from_bytes(g["part"][4:6], "big") == k
        assert int.from_bytes(g["part"][6:10], "big") == len(g["part"]) and g["part"][14:] == one[k % tiles]["part"][14:]
    assert got[0]["part"] == one[0]["part"] and got[tiles + 1]["part"] != one[1]["part"]
    # the part at index k against the part at index 0 of the SAME packets, as the header function makes them
    body = one[0]["part"][14:]
    p0 = orc.create_tile_header(0, body)
    for k in (1, 255, 256, 0x1234, 0xFFFF):
        pk = orc.create_tile_header(k, body)
        assert pk[:4] == p0[:4] and pk[6:] == p0[6:] and pk[4:6] == k.to_bytes(2, "big")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=[c["name"] for c in ALL_CASES])
def test_product_writes_the_pinned_tile_parts(case):
    import torch
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    from j2kgfx.context import Context
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    ctx = Context(0)
    frm = ref.golden_frame(case)
    W, H = case["W"], case["H"]
    Cn, prec = frm.shape[0], case.get("prec", 8)
    plan = FramePlan(W, H, Cn, precision=prec, lossless=True, num_resolutions=case["nres"], cb=(case["cb"], case["cb"]), tile=case["tile"], coder=case["coder"],
                     ctx=ctx, closed_loop=True)
    g = GOLDEN[case["name"]]
    if (Cn, prec) == (3, 8):
        pix = np.full((H, W, 4), 255, np.uint8)
        pix[..., :3] = frm.transpose(1, 2, 0)
        d_pix, fmt = torch.from_numpy(pix.reshape(H, W * 4)).to(plan.device), _lib.PIX_RGBA8
        want_back = pix.reshape(H, W * 4)
    elif prec in (8, 16):
        # the Go image of this component count and depth: image.Gray16.Pix is big-endian; 8 bit: createImage's own layout (decoder.go:417-588)
        import oracle as orc
        fmt = {(1, 8): _lib.PIX_GRAY8, (1, 16): _lib.PIX_GRAY16, (4, 8): _lib.PIX_NRGBA8}[(Cn, prec)]
        want_back = orc.create_image([frm[c] for c in range(Cn)], prec)       # (16 bit: with the int32 wrap of decoder.go:434-451 above 32768)
        pix = np.ascontiguousarray(frm[0].astype(">u2").view(np.uint8).reshape(H, W * 2)) if prec == 16 else want_back
        assert np.array_equal(np.stack(orc.extract_image_data(pix, fmt, W, H)), frm)
        d_pix = torch.from_numpy(pix).to(plan.device)
    else:
        d_pix = fmt = None                    # 12 bit: no Go image type holds the samples as they are (extractImageData would rescale): stage calls only
    # stage calls
    coeff = plan.forward(torch.from_numpy(frm.astype(np.int32)).to(plan.device))
    stream, offs, lens, numbps = plan.encode_stream(coeff)
    cs, toffs = plan.encode_tile_parts(stream, offs, lens, numbps, sop=case["sop"], eph=case["eph"])
    plan.frame_status()
    total = int(toffs[-1].item())
    assert total == g["bytes"]
    assert hashlib.sha256(cs[:total].cpu().numpy().tobytes()).hexdigest() == g["sha256"]
    if case["coder"] == 0:
        o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=None, sop=case["sop"], eph=case["eph"])
        back = plan.inverse(plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2)))
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), frm.astype(np.int32))
    if d_pix is None:
        plan.close()
        ctx.close()
        return
    # the one-call frame encoder
    cs2, toffs2 = plan.encode_frame_pixels(fmt, d_pix, sop=case["sop"], eph=case["eph"])
    plan.frame_status()
    assert int(toffs2[-1].item()) == total and hashlib.sha256(cs2[:total].cpu().numpy().tobytes()).hexdigest() == g["sha256"]
    # and back (MQ: to the source)
    back = torch.zeros_like(d_pix)
    plan.decode_frame_pixels(cs2, total, back, tile_offs=None, sop=case["sop"], eph=case["eph"])
    plan.frame_status()
    if case["coder"] == 0:
        assert np.array_equal(back.cpu().numpy(), want_back)
    plan.close()
    ctx.close()
