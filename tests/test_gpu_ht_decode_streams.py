"""GPU: the three-kernel HT block decoder (ht_vlcprep_kernel, ht_walk_kernel, ht_decode_kernel<STRIDED>, csrc/ht.hip) on streams its encoder
never writes -- the case lists of tests/ht_stream_cases.py (checked on the CPU by tests/test_ht_stream_cases.py) -- bit-exact against the C
oracle's HTDecoder.Decode (orc_ht_decode) everywhere, no tolerance.

Which test and group feeds which of the decoder's choices (block counts: tests/test_ht_stream_cases.py prints them per group):
  large blocks, serial by geometry (> 1024 coded samples, or > 128 quad pairs)   G in test_batches..., test_a_launch_of_large_blocks_only
  refused streams (len < 2, SCUP < 2, SCUP > len, MEL start)                     V, E, S("ones") in test_batches..., test_a_launch_of_refused_streams_only, plan tests
  every u <= 31: dword and per-byte deposits next to 0xFF                        M("<=31"), G, S, E
  some u >= 32                                                                   M("=32", ">=33"), and about a fifth of G / S / E
  u >= 32 with more 0xFF bytes or a longer segment than the parallel path takes  M at "ones" / FF7F / ff65 / ff200 and at 4241 bytes and more
  MagSgn staging at every pointer residue, first KB and later rounds             M lengths 0 .. 8000 packed back to back, and shifted by 1, 2, 3 bytes
  VLC unstuffing steps and its cap, the 7-bit rule                               S
  cleared coded rows on the routes that write nothing / through lane 0           test_plan_path_both_row_modes
  ht_decode_kernel<true>                                                         test_closed_loop_frame_decoder_on_replaced_bodies

What a subtly wrong rewrite would trip over, by reading csrc/ht.hip (one deliberate change each):
  the u >= 32 test moved to u > 32: a sample with u = 32 then needs 33 bits (magnitude and sign) from the 32-bit window of the u <= 31 extraction -- M("=32") in every test of M
      and in both plan tests;
  room for 32 positions of 0xFF while up to 64 are accepted: the bits loaded before a u > 32 advance come out wrong once more than 32 bytes of 0xFF
      precede it -- M(">=33") with ff63 / ff64 at 257, 1025 and 4240 bytes;
  no clearing of the coded rows for a refused stream under coded_rows_only: the sentinel stays in rows y % 4 == 0 -- test_plan_path_both_row_modes;
  no clamp on the staging loads past the first KB (wsrc[j] for j >= ndw): lanes with j >= ndw are marked invalid, deposit nothing and hand no byte to a
      valid lane, so the output is the same -- an over-read only, which no comparison of outputs can see (the plan tests keep 4096 guard bytes around
      the stream for that reason)."""
import collections

import numpy as np
import pytest

import ht_stream_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ent():
    from j2kgfx import entropy
    return entropy


_WANT = {}


def _want(oracle, c):
    key = (c.w, c.h, c.data)
    if key not in _WANT:
        _WANT[key] = oracle.ht_decode(np.frombuffer(c.data, np.uint8), c.w, c.h)
    return _WANT[key]


def _pack(cases, gap=b"", front=0, reverse=False):
    """the streams back to back (offsets take every residue mod 4), job order kept: (stream, offs, lens)"""
    n = len(cases)
    offs = np.zeros(n, np.uint64)
    lens = np.array([len(c.data) for c in cases], np.uint32)
    parts, pos = [b"\xa5" * front], front
    for j in (range(n - 1, -1, -1) if reverse else range(n)):
        offs[j] = pos
        parts += [cases[j].data, gap]
        pos += len(cases[j].data) + len(gap)
    return np.frombuffer(b"".join(parts), np.uint8), offs, lens


def _decode(ent, cases, **how):
    from j2kgfx import CODER_HT
    stream, offs, lens = _pack(cases, **how)
    blocks = np.zeros(len(cases), ent.BLOCK_DTYPE)
    blocks["w"] = [c.w for c in cases]
    blocks["h"] = [c.h for c in cases]
    return ent.decode_blocks(CODER_HT, stream, offs, lens, np.zeros(len(cases), np.uint8), blocks)


def _check(oracle, cases, outs, what):
    bad = [(j, c.label, c.w, c.h, len(c.data)) for j, (c, got) in enumerate(zip(cases, outs)) if not np.array_equal(got, _want(oracle, c))]
    assert not bad, "%s: %d of %d blocks differ from the oracle, first: %s" % (what, len(bad), len(cases), bad[:5])


def _calls(cases, seed, most=400):
    """the group shuffled with a fixed seed, cut into calls of at most `most` blocks of near-equal size"""
    order = np.random.default_rng(seed).permutation(len(cases))
    k = -(-len(cases) // most)
    return [[cases[int(i)] for i in part] for part in np.array_split(order, k)]


def _group(name):
    if name == "GV":                                          # (G alone is 92 blocks: run with V, 236 in one call)
        return hc.group_G() + hc.group_V()
    return hc.GROUPS[name]()


# ---- 1. batches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["GV", "M", "S", "E"])
def test_batches_of_mixed_blocks_equal_the_oracle(ent, oracle, name):
    """calls of 130-400 blocks of mixed shape and kind: a walk workgroup of 64 lanes holds large, refused, u <= 31 and u >= 32 blocks side by
    side, and the last workgroup of every kernel is partial"""
    for k, cases in enumerate(_calls(_group(name), 0x6201)):
        assert 130 <= len(cases) <= 400
        _check(oracle, cases, _decode(ent, cases), "%s call %d" % (name, k))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes_around_the_walk_workgroup(ent, oracle, n):
    pool = _calls(hc.group_G(), 0x6202)[0] + _calls(hc.group_V(), 0x6202)[0]       # G first: 129 takes all of G and 37 of V
    cases = pool[:n]
    _check(oracle, cases, _decode(ent, cases), "batch of %d" % n)


@pytest.mark.parametrize("front", [1, 2, 3])
def test_m_shifted_by_one_two_three_bytes(ent, oracle, front):
    for k, cases in enumerate(_calls(hc.group_M(), 0x6203)):
        _check(oracle, cases, _decode(ent, cases, front=front), "M + %d, call %d" % (front, k))


# ---- 2. neighbour independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["M", "S"])
def test_a_blocks_output_does_not_depend_on_its_neighbours_bytes(ent, oracle, name):
    """what the suite can see of an over-read: the same blocks packed tightly, with 8 bytes of 0x00 and of 0xFF between them, and in reversed
    order of packing -- every block decodes to the same samples, the oracle's"""
    for k, cases in enumerate(_calls(_group(name), 0x6204)):
        for what, how in (("tight", {}), ("0x00 between", dict(gap=bytes(8))), ("0xFF between", dict(gap=b"\xff" * 8)), ("reversed", dict(reverse=True)),
                          ("reversed, 0xFF between, + 1", dict(reverse=True, gap=b"\xff" * 8, front=1))):
            _check(oracle, cases, _decode(ent, cases, **how), "%s call %d, %s" % (name, k, what))


# ---- 5. wave-uniform early exits with nothing else in the launch ---------------------------------------------------------------------------------
def test_a_launch_of_refused_streams_only(ent, oracle):
    cases = [c for c in hc.group_V() if c.expect != "none"] + [c for c in hc.group_E() if "scup_ones" in c.label or "scup_zero" in c.label]
    cases += [c for c in hc.group_S() if " ones " in c.label]
    cases = [c for c in cases if hc.classify(c.data, c.w, c.h).reject != "none"]       # (SCUP 4095 is valid on a block of 4095 bytes and more)
    assert len(cases) >= 130
    why = collections.Counter(hc.classify(c.data, c.w, c.h).reject for c in cases)
    assert "none" not in why and all(why[k] >= 4 for k in ("len<2", "scup<2", "scup>len", "mel")), why
    _check(oracle, cases, _decode(ent, cases), "refused only")


def test_a_launch_of_large_blocks_only(ent, oracle):
    """every block beyond 1024 coded samples or 128 quad pairs (each rule alone, and both)"""
    rng = np.random.default_rng(0x6205)
    shapes = [(65, 60), (64, 68), (1028, 4), (4, 516), (129, 32), (8, 516), (68, 64), (1025, 1), (72, 61)]
    cases = [c for c in hc.group_G() if (c.w, c.h) in shapes]
    for k in range(130):
        w, h = shapes[k % len(shapes)]
        cases.append(hc.Case(w, h, hc.random_stream(rng, w, h) if k % 4 else hc.damage(rng, hc.encoder_output(rng, w, h, 300), hc.E_KINDS[k % 7]), "large %d" % k))
    for c in cases:
        assert hc.is_large(c.w, c.h)
    assert sum(1 for c in cases if _want(oracle, c).any()) > len(cases) // 2
    _check(oracle, cases, _decode(ent, cases), "large only")


# ---- 3. + 4. plans whose jobs carry the cases ------------------------------------------------------------------------------------------------------
PLANS = hc.PLANS


def _shapes(blocks):
    return [(int(b["w"]), int(b["h"])) for b in blocks]


def _guarded(torch, device, stream, guard=4096):
    """the stream inside a larger device tensor, `guard` bytes either side: no version of the code reads outside an allocation"""
    buf = torch.full((stream.size + 2 * guard,), 0xFF, dtype=torch.uint8, device=device)
    if stream.size:
        buf[guard:guard + stream.size] = torch.from_numpy(stream.copy()).to(device)
    return buf[guard:]


@pytest.mark.parametrize("geo", PLANS, ids=["328x211_cb64", "200x150_cb16_tile64"])
def test_plan_path_both_row_modes(oracle, geo):
    """j2k_plan_decode_blocks with every job's body replaced by a case of its shape, then the four checks of test_plan_decode_coded_rows_only:
    fresh; poisoned buffer with coded rows only (coded rows = the oracle's, every other row keeps the sentinel -- the refused streams and the
    blocks that go through lane 0 must have cleared their coded rows themselves); zeroed buffer == fresh; switched off again"""
    import torch
    from j2kgfx.codec import FramePlan
    plan = FramePlan(geo["W"], geo["H"], 3, precision=8, lossless=True, num_resolutions=geo["nres"], cb=(geo["cb"], geo["cb"]), tile=geo["tile"], coder=1)
    blocks, doffs = plan.blocks(), plan.decoded_offsets()
    n = int(plan.info.blocks)
    cases = hc.bodies_for(_shapes(blocks), 0x6300 + geo["W"])
    kinds = hc.kinds(cases)
    print("plan %s: %d blocks, %s" % (geo, n, dict(kinds)))
    assert kinds["refused"] >= 5 and kinds["=32"] >= 5 and kinds[">=33"] >= 5 and kinds["<=31"] >= 5 and kinds["far"] >= 5, kinds
    hs, ho, hl = _pack(cases)
    stream = _guarded(torch, plan.device, hs)
    offs = torch.from_numpy(np.append(ho, hs.size).astype(np.int64)).to(plan.device)
    lens = torch.from_numpy(hl.astype(np.int32)).to(plan.device)
    nb = torch.zeros(n, dtype=torch.uint8, device=plan.device)
    fresh = plan.decode_blocks(stream, offs, lens, nb)
    plan.ctx.sync()
    plan.set_decode_coded_rows_only(True)
    SENT = -123456789
    poisoned = torch.full((int(plan.info.decoded_elems),), SENT, dtype=torch.int32, device=plan.device)
    zeroed = torch.zeros_like(poisoned)
    plan.decode_blocks(stream, offs, lens, nb, decoded=poisoned)
    plan.decode_blocks(stream, offs, lens, nb, decoded=zeroed)
    plan.ctx.sync()
    plan.set_decode_coded_rows_only(False)
    again = plan.decode_blocks(stream, offs, lens, nb)
    plan.ctx.sync()
    hf, hp, hz, ha = fresh.cpu().numpy(), poisoned.cpu().numpy(), zeroed.cpu().numpy(), again.cpu().numpy()
    for j, c in enumerate(cases):
        w, h, o = c.w, c.h, int(doffs[j])
        want = _want(oracle, c)
        assert np.array_equal(hf[o:o + w * h].reshape(h, w), want), ("fresh", j, c.label)
        assert np.array_equal(ha[o:o + w * h].reshape(h, w), want), ("switched off again", j, c.label)
        got = hp[o:o + w * h].reshape(h, w)
        assert np.array_equal(got[0::4], want[0::4]), ("coded rows", j, c.label)
        for r in (1, 2, 3):
            assert (got[r::4] == SENT).all(), ("untouched rows", j, r, c.label)
        assert np.array_equal(hz[o:o + w * h].reshape(h, w), want), ("zeroed buffer == fresh decoder", j, c.label)
    plan.close()


@pytest.mark.parametrize("geo", PLANS, ids=["328x211_cb64", "200x150_cb16_tile64"])
def test_closed_loop_frame_decoder_on_replaced_bodies(oracle, geo):
    """ht_decode_kernel<true>: tile-parts made by the project's own packet encoder from replaced bodies (numbps as the block coder gave it; HT
    ignores it), decoded to pixels by j2k_plan_decode_frame_pixels == the stage calls on the same tile-parts (parse, dense block decode, placement,
    inverse), whose blocks are compared with the oracle one by one here as well.  A job the block coder left without bytes keeps its empty
    body (its packet says `not included`); every other job carries a case."""
    import torch
    from closed_loop_ref import frame as make_frame
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    W, H = geo["W"], geo["H"]
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=geo["nres"], cb=(geo["cb"], geo["cb"]), tile=geo["tile"], coder=_lib.CODER_HT, closed_loop=True)
    frm = make_frame(W, H, 77, noise=40)
    rgba = np.concatenate([frm.transpose(1, 2, 0), np.full((H, W, 1), 255, np.uint8)], axis=2).reshape(H, W * 4)
    d_pix = torch.from_numpy(np.ascontiguousarray(rgba)).to(plan.device)
    coeff = plan.forward_pixels(_lib.PIX_RGBA8, d_pix)
    stream, offs, lens, numbps = plan.encode_stream(coeff)
    plan.frame_status()
    n = int(plan.info.blocks)
    blocks = plan.blocks()
    e_len, e_off, e_str = lens.cpu().numpy()[:n], offs.cpu().numpy()[:n], stream.cpu().numpy()
    keep = [int(e_len[j]) == 0 for j in range(n)]
    picked = hc.bodies_for(_shapes(blocks), 0x6400 + W, keep=keep)
    cases = [c if c is not None else hc.Case(int(blocks[j]["w"]), int(blocks[j]["h"]), b"", "encoder: empty") for j, c in enumerate(picked)]
    replaced = [c for c in picked if c is not None]
    kinds = hc.kinds(replaced)
    print("closed-loop plan %s: %d blocks, %d replaced, %s" % (geo, n, len(replaced), dict(kinds)))
    assert len(replaced) * 10 >= 3 * n and kinds["=32"] >= 5 and kinds[">=33"] >= 5, (n, len(replaced), kinds)
    hs, ho, hl = _pack(cases)
    stream2 = _guarded(torch, plan.device, hs)
    offs2 = torch.from_numpy(np.append(ho, hs.size).astype(np.int64)).to(plan.device)
    lens2 = torch.from_numpy(hl.astype(np.int32)).to(plan.device)
    out = torch.zeros(plan.frame_bound() + 2 * hs.size + 8192, dtype=torch.uint8, device=plan.device)
    cs, toffs = plan.encode_tile_parts(stream2, offs2, lens2, numbps, sop=True, eph=True, out=out[4096:])
    plan.frame_status()
    total = int(toffs[-1].item())
    # the bodies arrive: every length could be expressed by the packet encoder, every byte is where the parse says
    o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=toffs, sop=True, eph=True)
    plan.frame_status()
    h_cs, p_off, p_len = cs.cpu().numpy(), o2.cpu().numpy()[:n], l2.cpu().numpy()[:n]
    assert np.array_equal(p_len.astype(np.int64), hl.astype(np.int64))
    for j, c in enumerate(cases):
        assert bytes(h_cs[int(p_off[j]):int(p_off[j]) + len(c.data)]) == c.data, j
    dense = plan.decode_blocks(cs, o2, l2, n2)
    want_pix = plan.inverse_pixels(plan.place_blocks(dense), torch.zeros_like(d_pix))
    plan.frame_status()
    hd, doffs = dense.cpu().numpy(), plan.decoded_offsets()
    for j, c in enumerate(cases):
        o = int(doffs[j])
        assert np.array_equal(hd[o:o + c.w * c.h].reshape(c.h, c.w), _want(oracle, c)), ("stage calls", j, c.label)
    for tile_offs in (toffs, None):
        got = torch.zeros_like(d_pix)
        plan.decode_frame_pixels(cs, total, got, tile_offs=tile_offs, sop=True, eph=True)
        plan.frame_status()
        assert torch.equal(got, want_pix)
    plan.close()
