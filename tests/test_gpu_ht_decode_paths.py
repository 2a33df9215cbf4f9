"""GPU: the two forms of the third HT decode kernel -- ht_decode_lean_kernel (option ht_dec_lean = 1, the default: blocks 8, 16, 32 or 64 wide with a
16-byte aligned window and every u <= 31 take its written-out path, everything else the general decoder behind it) and ht_decode_kernel (ht_dec_lean = 0) -- on
the block shapes and stream contents that decide between their paths, bit-exact against the C oracle's HTDecoder.Decode (orc_ht_decode).

Shapes (w x h): 64x64, 64x61, 64x4, 64x1 (the written-out path: two rounds of pairs, a last stripe of one row, one round, one row);
32x32, 16x16 and 8x12 (its narrow form: a pair's 32 bytes stored as they lie); 60x64 and 4x64 (the general decoder's vector stores); 13x7 (scalar stores); 64x68 (more than 1024 coded samples: lane 0 alone, host call only).
Contents per shape: no bytes at all (an all-zero block), one non-zero sample, inputs of magnitude 1..2, inputs up to 2^30 (or as far as the
reference's encoder takes the shape: segments of several KB with 0xFF bytes on the 64-wide blocks, every u <= 31), a suffix
with a u of exactly 32 and one with a u above 32 (tests/ht_stream_cases.find_suffixes) behind random MagSgn bytes and behind 0xFF-rich ones,
one byte (len < 2), and an SCUP field larger than the stream (refused: the output stays zero).

Every case runs under both option values, and a second time after a device synchronisation (an idle device: the non-temporal stores of the
coded rows and the zero rows then meet an empty write path, docs/KERNEL_NOTES.md 4d)."""
import numpy as np
import pytest

import ht_stream_cases as hc

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (64, 61), (64, 4), (64, 1), (32, 32), (16, 16), (8, 12), (60, 64), (4, 64), (13, 7)]
KINDS = ["empty", "one", "small", "full", "u32", "u33", "u33_ff", "len1", "scup"]
MARK = -123456789


@pytest.fixture(scope="module")
def ctxs():
    """{option value: context}"""
    from j2kgfx import Context
    out = {}
    for lean in (0, 1):
        out[lean] = Context(0)
        out[lean].set_option("ht_dec_lean", lean)
    return out


def _encoded(oracle, x):
    h, w = x.shape
    return bytes(oracle.ht_encode(np.ascontiguousarray(x, np.int32), w, h))


def _case(oracle, w, h, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "empty":
        return hc.Case(w, h, b"", kind)
    if kind == "len1":
        return hc.Case(w, h, b"\x5a", kind)
    if kind == "one":
        x = np.zeros((h, w), np.int32)
        x[int(rng.integers(0, h)), int(rng.integers(0, w))] = int(rng.integers(1, 1000)) * (1 if seed % 2 else -1)
        return hc.Case(w, h, _encoded(oracle, x), kind)
    if kind == "small":
        x = (rng.integers(1, 3, (h, w)) * rng.choice([-1, 1], (h, w))).astype(np.int32)
        return hc.Case(w, h, _encoded(oracle, x), kind)
    if kind == "full":                                       # magnitudes up to 2^30, or the largest power of four below that the reference's encoder takes
        for e in range(30, 0, -2):                           # (it panics where a small block's bytes outgrow its buffer: ht_stream_cases.encoder_output)
            try:
                return hc.Case(w, h, _encoded(oracle, rng.integers(-(1 << e), (1 << e) + 1, (h, w))), kind)
            except ValueError:
                continue
        raise AssertionError("no encoder output for %dx%d" % (w, h))
    if kind == "scup":
        good = hc.encoder_output(rng, w, h, 300)
        return hc.Case(w, h, hc.with_scup(good, len(good) + 1), kind)
    found = hc.find_suffixes(w, h, 2, 600)[0]
    sufs = found["=32" if kind == "u32" else ">=33"]
    if (w, h) not in SHAPES:                                 # the plans' other blocks (60x61, 4x4, ...): whatever u their few pairs can reach
        sufs = sufs or found[">=33"] or found["=32"] or found["<=31"]
    assert sufs, "no suffix with such a u on %dx%d" % (w, h)
    content, n = ("ff63", 257) if kind == "u33_ff" else ("random", int(rng.integers(40, 1200)))
    return hc.Case(w, h, hc.splice(hc.magsgn_content(rng, content, n), sufs[seed % len(sufs)]), kind)


_CASES, _WANT = {}, {}


def _get(oracle, w, h, kind, seed):
    key = (w, h, kind, seed)
    if key not in _CASES:
        c = _CASES[key] = _case(oracle, w, h, kind, seed)
        _WANT[key] = oracle.ht_decode(np.frombuffer(c.data, np.uint8), w, h)
    return _CASES[key], _WANT[key]


def test_the_cases_are_what_their_names_say(oracle):
    """(no kernel runs here: the streams' own properties, by ht_stream_cases.classify)"""
    for w, h in SHAPES:
        for kind in KINDS:
            c, want = _get(oracle, w, h, kind, 1)
            info = hc.classify(c.data, w, h)
            if kind in ("empty", "len1"):
                assert info.reject == "len<2"
            elif kind == "scup":
                assert info.reject == "scup>len"
            else:
                assert info.reject == "none", (w, h, kind)
                if kind == "u32":
                    assert info.max_u == 32
                elif kind in ("u33", "u33_ff"):
                    assert info.max_u >= 33 and (kind == "u33" or info.n_ff == 63)
                else:                                        # (this coder's u is not the magnitude's width: small inputs reach u > 31 on some shapes)
                    assert want.any(), (w, h, kind, info)
                    if w == 64 and kind == "full":           # the written-out path of the lean kernel, with 0xFF bytes where the segment has thousands of bytes
                        assert info.max_u <= 31 and (h < 61 or (info.seg_len > 3000 and info.n_ff >= 4)), (w, h, kind, info)
            if kind in ("empty", "len1", "scup"):
                assert not want.any()


# ---- 1. the host call (dense blocks, every row written): all shapes x contents, and the blocks beyond 1024 coded samples ---------------------
@pytest.mark.parametrize("lean", [0, 1])
def test_every_shape_and_content_in_one_host_call(ctxs, oracle, lean):
    import torch
    from j2kgfx import CODER_HT, entropy
    cases, want = [], []
    for w, h in SHAPES:
        for kind in KINDS:
            c, x = _get(oracle, w, h, kind, 2)
            cases.append(c); want.append(x)
    rng = np.random.default_rng(0x6801)
    for k, data in enumerate((hc.encoder_output(rng, 64, 68, 300), hc.random_stream(rng, 64, 68), hc.encoder_output(rng, 72, 61, 40000))):
        w, h = (72, 61) if k == 2 else (64, 68)
        assert hc.is_large(w, h)
        cases.append(hc.Case(w, h, data, "large")); want.append(oracle.ht_decode(np.frombuffer(data, np.uint8), w, h))
    offs = np.cumsum([0] + [len(c.data) for c in cases[:-1]]).astype(np.uint64)
    lens = np.array([len(c.data) for c in cases], np.uint32)
    stream = np.frombuffer(b"".join(c.data for c in cases) + b"\xff" * 16, np.uint8)
    blocks = np.zeros(len(cases), entropy.BLOCK_DTYPE)
    blocks["w"] = [c.w for c in cases]
    blocks["h"] = [c.h for c in cases]
    for rep in range(2):
        torch.cuda.synchronize()
        got = entropy.decode_blocks(CODER_HT, stream, offs, lens, np.zeros(len(cases), np.uint8), blocks, ctx=ctxs[lean])
        bad = [(c.w, c.h, c.label) for c, g, x in zip(cases, got, want) if not np.array_equal(g, x)]
        assert not bad, (rep, bad)


# ---- 2. plans of one resolution: the blocks are the 64 x 64 grid over the plane, so the plane's size picks the shapes -------------------------
PLANS = [(124, 125), (68, 68), (64, 65), (96, 80), (72, 76), (13, 7)]   # 64|60 x 64|61; 64|4 x 64|4; 64 x 64|1; 64|32 x 64|16; 64|8 x 64|12; 13 x 7


def _plan_shapes(W, H):
    return sorted({(w, h) for w in ([64] * (W // 64) + ([W % 64] if W % 64 else [])) for h in ([64] * (H // 64) + ([H % 64] if H % 64 else []))})


@pytest.mark.parametrize("lean", [0, 1])
@pytest.mark.parametrize("WH", PLANS, ids=["124x125", "68x68", "64x65", "96x80", "72x76", "13x7"])
def test_plan_decode_every_row_mode_and_window_alignment(ctxs, oracle, WH, lean):
    """j2k_plan_decode_blocks into a buffer filled with a marker, the contents dealt over the jobs by turns (nine rounds: every shape of the plan
    meets every content).  Rows mode off: the whole block equals the oracle's, so the rows y % 4 != 0 are zero.  Rows mode on: the coded rows
    equal the oracle's and every other row keeps the marker.  Both again with the buffer one sample further on, so that no window is 16-byte
    aligned (the 64-wide blocks then leave the written-out path).  What lies between the blocks keeps the marker."""
    import torch
    from j2kgfx.codec import FramePlan
    W, H = WH
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=1, cb=(64, 64), coder=1, ctx=ctxs[lean])
    blocks, doffs = plan.blocks(), plan.decoded_offsets()
    n, total = int(plan.info.blocks), int(plan.info.decoded_elems)
    shapes = [(int(b["w"]), int(b["h"])) for b in blocks]
    assert sorted(set(shapes)) == _plan_shapes(W, H), shapes
    nb = torch.zeros(n, dtype=torch.uint8, device=plan.device)
    covered = np.zeros(total + 1, bool)
    for j, (w, h) in enumerate(shapes):
        covered[int(doffs[j]):int(doffs[j]) + w * h] = True
    for rnd in range(len(KINDS)):
        picked = [_get(oracle, w, h, KINDS[(j + rnd) % len(KINDS)], 3 + j % 3) for j, (w, h) in enumerate(shapes)]
        cases = [c for c, _ in picked]
        data = b"".join(c.data for c in cases)
        ho = np.cumsum([0] + [len(c.data) for c in cases]).astype(np.int64)
        buf = torch.full((len(data) + 8192,), 0xFF, dtype=torch.uint8, device=plan.device)
        if data:
            buf[4096:4096 + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(plan.device)
        stream, offs = buf[4096:], torch.from_numpy(ho).to(plan.device)
        lens = torch.from_numpy(np.diff(ho).astype(np.int32)).to(plan.device)
        for rep in range(2):
            for rows_only in (False, True):
                for shift in (0, 1):
                    torch.cuda.synchronize()
                    plan.set_decode_coded_rows_only(rows_only)
                    out = torch.full((total + 1,), MARK, dtype=torch.int32, device=plan.device)
                    plan.decode_blocks(stream, offs, lens, nb, decoded=out[shift:])
                    plan.ctx.sync()
                    got = out.cpu().numpy()[shift:]
                    where = (W, H, lean, rnd, rep, rows_only, shift)
                    for j, ((c, want), (w, h)) in enumerate(zip(picked, shapes)):
                        g = got[int(doffs[j]):int(doffs[j]) + w * h].reshape(h, w)
                        assert np.array_equal(g[0::4], want[0::4]), ("coded rows", where, j, w, h, c.label)
                        for r in (1, 2, 3):
                            assert (g[r::4] == (MARK if rows_only else 0)).all(), ("other rows", where, j, w, h, r, c.label)
                            assert not want[r::4].any()
                    assert (got[:total][~covered[:total]] == MARK).all() and (out.cpu().numpy()[:shift] == MARK).all(), ("between the blocks", where)
    plan.set_decode_coded_rows_only(False)
    plan.close()


# ---- 3. the closed-loop frame decoder: ht_decode_kernel<true> / ht_decode_lean_kernel<true>, blocks written into their windows of the planes -----
def test_closed_loop_frame_both_forms(ctxs):
    """pixels -> tile-parts -> pixels, 328 x 211 with 64 x 64 blocks (windows of every width, 16-byte aligned and not): under both forms
    j2k_plan_decode_frame_pixels equals the stage calls on the same tile-parts (parse, dense block decode -- pinned to the oracle above --
    placement, inverse), twice, and the two forms agree with each other"""
    import torch
    from closed_loop_ref import frame as make_frame
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    W, H = 328, 211
    frm = make_frame(W, H, 78, noise=40)
    rgba = np.concatenate([frm.transpose(1, 2, 0), np.full((H, W, 1), 255, np.uint8)], axis=2).reshape(H, W * 4)
    pix = {}
    for lean in (0, 1):
        plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=3, cb=(64, 64), coder=_lib.CODER_HT, closed_loop=True, ctx=ctxs[lean])
        d_pix = torch.from_numpy(np.ascontiguousarray(rgba)).to(plan.device)
        cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA8, d_pix, sop=True, eph=True)
        plan.frame_status()
        total = int(toffs[-1].item())
        o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=toffs, sop=True, eph=True)
        want = plan.inverse_pixels(plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2)), torch.zeros_like(d_pix))
        plan.frame_status()
        assert want.any()
        for rep in range(2):
            torch.cuda.synchronize()
            back = torch.zeros_like(d_pix)
            plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=True, eph=True)
            plan.frame_status()
            assert torch.equal(back, want), (lean, rep)
        pix[lean] = want.cpu().numpy()
        plan.close()
    assert np.array_equal(pix[0], pix[1])
