"""GPU: the two forms of the HT block decoder's front end -- ht_vlcprep_kernel + ht_walk_kernel (option ht_dec_front = 3, two launches, the unstuffed
VLC strings travel through global memory) and ht_front_kernel (ht_dec_front = 1: one launch, every walk workgroup unstuffs the strings of its own 64
blocks into the rows its wavefront 0 then walks) -- bit-exact against the C oracle's HTDecoder.Decode (orc_ht_decode).  Never one form against the other.

Every case runs under both values, each with ht_dec_lean = 0 and 1 behind it (the third kernel reads the records and the SCUP word the front end
leaves), and a second time after a device synchronisation (an idle device, docs/KERNEL_NOTES.md 4d).

What decides between the paths of the fused kernel, and the test that holds it:
  workgroups of 64 blocks, prep wavefronts of 64 / NW blocks: batches of 1, 3, 63, 64, 65, 130      test_batch_sizes
      (a lone block; prep wavefronts without a block; a full workgroup; a last workgroup of one and of two blocks)
  tags side by side in one workgroup -- refused (len < 2, SCUP < 2, SCUP > len, MEL start), empty,     test_mixed_tags_in_one_workgroup,
      serial by geometry, ordinary -- in fixed and in shuffled places: a refused or serial block's       test_refused_streams_only
      row is never written, its lane must not walk, its neighbours' rows and records stay theirs
  VLC segments of SCUP - 2 = 0, 1, 3, 4, 255, 256, 257, 512 bytes and one beyond the cap               test_vlc_segment_lengths
      (the ends of the four-byte groups of a lane and of the 256-byte steps)
  the 7-bit rule at every place of a lane's group, across lanes and across steps                      test_stuffed_vlc_tails
  j2k_plan_decode_blocks in both row modes, the closed-loop frame decoder                              test_plan_*, test_closed_loop_*

The serial path by geometry: ht_vlc_head (csrc/ht.hip) takes a block as fast iff ceil(h/4) * w <= 1024 and ceil(h/4) * ceil(ceil(w/4)/2) <= 128.
The smallest block it sends to the serial path is 1 x 513 (129 quad pairs of one column; 1 x 512 is fast) -- ht_stream_cases.is_large states the
same rule, asserted below.

test_stuffed_vlc_tails builds its tails directly (bytes above 0x8F followed, in the reverse reader's order, by x7F bytes); a tail the oracle refuses
is a case too (the output is zero).  test_the_constructed_tails_mostly_decode checks, with the oracle alone, that at least half of them decode to
something (measured when written: all 30)."""
import numpy as np
import pytest

import ht_stream_cases as hc

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (64, 61), (64, 1), (32, 32), (16, 16), (8, 12), (60, 64), (4, 64), (13, 7)]
SERIAL = (1, 513)
FORMS = [(front, lean) for front in (3, 1) for lean in (0, 1)]


@pytest.fixture(scope="module")
def ctxs():
    """{(ht_dec_front, ht_dec_lean): context}"""
    from j2kgfx import Context
    out = {}
    for front, lean in FORMS:
        c = out[(front, lean)] = Context(0)
        c.set_option("ht_dec_front", front)
        c.set_option("ht_dec_lean", lean)
    return out


_WANT = {}


def _want(oracle, c):
    key = (c.w, c.h, c.data)
    if key not in _WANT:
        _WANT[key] = oracle.ht_decode(np.frombuffer(c.data, np.uint8), c.w, c.h)
    return _WANT[key]


def _pack(cases):
    offs = np.cumsum([0] + [len(c.data) for c in cases[:-1]]).astype(np.uint64)
    lens = np.array([len(c.data) for c in cases], np.uint32)
    return np.frombuffer(b"".join(c.data for c in cases) + b"\xff" * 16, np.uint8), offs, lens


def _check_all_forms(ctxs, oracle, cases, what):
    """the host decode call on the batch: every form, twice, every block against the oracle"""
    import torch
    from j2kgfx import CODER_HT, entropy
    stream, offs, lens = _pack(cases)
    blocks = np.zeros(len(cases), entropy.BLOCK_DTYPE)
    blocks["w"] = [c.w for c in cases]
    blocks["h"] = [c.h for c in cases]
    want = [_want(oracle, c) for c in cases]
    for form in FORMS:
        for rep in range(2):
            torch.cuda.synchronize()
            got = entropy.decode_blocks(CODER_HT, stream, offs, lens, np.zeros(len(cases), np.uint8), blocks, ctx=ctxs[form])
            bad = [(j, c.w, c.h, c.label) for j, (c, g, x) in enumerate(zip(cases, got, want)) if not np.array_equal(g, x)]
            assert not bad, "%s, front %d lean %d, run %d: %d of %d blocks differ from the oracle, first: %s" % ((what,) + form + (rep, len(bad), len(cases), bad[:5]))


# ---- streams -----------------------------------------------------------------------------------------------------------------------------
_POOL = []


def _pool():
    """130 ordinary blocks, the nine shapes by turns (any 63 in a row hold each seven times): encoder output of three amplitudes and, every
    fifth, random bytes with a valid SCUP field"""
    if not _POOL:
        rng = np.random.default_rng(0x7801)
        for i in range(130):
            w, h = SHAPES[i % len(SHAPES)]
            if i % 5 == 4:
                _POOL.append(hc.Case(w, h, hc.random_stream(rng, w, h), "random"))
            else:
                _POOL.append(hc.Case(w, h, hc.encoder_output(rng, w, h, (3, 300, 40000)[i % 3]), "encoder"))
    return _POOL


def _refused(rng, w, h, why):
    good = hc.encoder_output(rng, w, h, 300)
    if why == "len<2":
        return hc.Case(w, h, b"\x5a", why)
    if why == "scup<2":
        return hc.Case(w, h, hc.with_scup(good, int(rng.integers(0, 2))), why)
    if why == "scup>len":
        return hc.Case(w, h, hc.with_scup(good, len(good) + 1), why)
    suf = bytearray(hc._rand_no_ff(rng, 40))                 # "mel": 0xFF, then a byte above 0x8F, where the MEL reader starts (an empty MagSgn segment: pos = 0)
    suf[0], suf[1] = 0xFF, 0x95
    return hc.Case(w, h, hc.with_scup(bytes(suf), 40), why)


WHYS = ["len<2", "scup<2", "scup>len", "mel"]


def _mixed(seed, shuffled):
    """64 blocks: the four refusals four times each (on shapes by turns), 6 empty, 6 serial by geometry, 36 ordinary"""
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(16):
        w, h = SHAPES[k % len(SHAPES)]
        cases.append(_refused(rng, w, h, WHYS[k % 4]))
    for k in range(6):
        w, h = SHAPES[(2 * k) % len(SHAPES)]
        cases.append(hc.Case(w, h, b"", "empty"))
    for k in range(6):
        w, h = SERIAL
        cases.append(hc.Case(w, h, hc.random_stream(rng, w, h) if k % 2 else hc.encoder_output(rng, w, h, 300), "serial"))
    cases += _pool()[:36]
    assert len(cases) == 64
    if shuffled:
        cases = [cases[int(i)] for i in rng.permutation(64)]
    else:                                                       # fixed places: the kinds dealt round the workgroup, so every prep wavefront meets several
        cases = [cases[(i * 37) % 64] for i in range(64)]
    return cases


def test_the_cases_are_what_their_names_say(oracle):
    """(no kernel runs here)"""
    assert hc.is_large(*SERIAL) and not hc.is_large(1, 512) and not any(hc.is_large(w, h) for w, h in SHAPES)
    assert not any(hc.is_large(w, h) and w * h < SERIAL[0] * SERIAL[1] for w in range(1, 70) for h in range(1, 520))
    for shuffled in (False, True):
        cases = _mixed(0x7802, shuffled)
        for c in cases:
            info = hc.classify(c.data, c.w, c.h)
            if c.label in WHYS:
                assert info.reject == c.label and not _want(oracle, c).any(), (c.label, info)
            elif c.label == "empty":
                assert info.reject == "len<2"
        assert sum(1 for c in cases if _want(oracle, c).any()) >= 36
    assert any(_want(oracle, c).any() for c in _mixed(0x7802, False) if c.label == "serial")


# ---- batch sizes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 130])
def test_batch_sizes(ctxs, oracle, n):
    cases = _pool()[:n]
    if n >= 63:
        assert {(c.w, c.h) for c in cases} == set(SHAPES)
    _check_all_forms(ctxs, oracle, cases, "batch of %d" % n)


# ---- tags ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True], ids=["fixed", "shuffled"])
def test_mixed_tags_in_one_workgroup(ctxs, oracle, shuffled):
    _check_all_forms(ctxs, oracle, _mixed(0x7802, shuffled), "mixed tags")


def test_refused_streams_only(ctxs, oracle):
    rng = np.random.default_rng(0x7803)
    cases = [_refused(rng, *SHAPES[k % len(SHAPES)], WHYS[k % 4]) for k in range(70)]
    assert not any(_want(oracle, c).any() for c in cases)
    _check_all_forms(ctxs, oracle, cases, "refused only")


# ---- VLC segment lengths ---------------------------------------------------------------------------------------------------------------------
def _cap(w, h):
    """bytes of the VLC segment the reverse reader can reach: 46 bits per quad pair, and the read-ahead (ht_vlc_nbytes, csrc/ht.hip)"""
    pairs = ((h + 3) // 4) * ((((w + 3) // 4) + 1) // 2)
    return (46 * pairs + 7) // 8 + 8


def _length_cases():
    rng = np.random.default_rng(0x7804)
    cases = []
    for w, h in ((8, 12), (16, 16)):
        for vlc in (0, 1, 3, 4, 255, 256, 257, 512, _cap(w, h) + 1):
            for k in range(2):
                n = vlc + 2                                  # SCUP: the suffix is the MEL/VLC bytes and the two of the field
                suf = bytearray(hc._rand(rng, n))
                for i in range(min(4, n)):
                    suf[i] &= 0x7F                           # (nothing the MEL start refuses)
                mag = hc._rand(rng, (0, 33)[k])
                cases.append(hc.Case(w, h, hc.splice(mag, hc.with_scup(bytes(suf), n)), "VLC segment of %d" % vlc))
    return cases


def test_vlc_segment_lengths(ctxs, oracle):
    cases = _length_cases()
    for c in cases:
        assert hc.scup_of(c.data) - 2 == int(c.label.split()[-1])
    assert sum(1 for c in cases if _want(oracle, c).any()) * 2 >= len(cases)
    _check_all_forms(ctxs, oracle, cases, "segment lengths")


# ---- stuffing ----------------------------------------------------------------------------------------------------------------------------------
def _tail(rng, n, ks, second):
    """a suffix of n bytes whose reverse-reader byte k (k >= 1: suffix[n - 2 - k]; a lane of step c holds k = 256 c + 4 l + 1 .. + 4) is a byte with its low
    seven bits set, behind a byte above 0x8F, for every k of ks; everything else below 0x80, so these are the only 7-bit bytes.  k = 1 follows the
    byte the reader starts in, whose low nibble counts as ones: its high nibble is raised above 8."""
    b = bytearray(int(x) & 0x7F for x in rng.integers(0, 256, n))
    for k in ks:
        assert 1 <= k <= n - 3
        b[n - 2 - k] = second
        b[n - 2 - (k - 1)] = int(rng.integers(0x90, 0x100)) if k > 1 else (b[n - 2] & 0x0F) | 0x90
    return hc.with_scup(bytes(b), n)


def _stuffed_cases():
    rng = np.random.default_rng(0x7805)
    cases = []
    for c in range(3):                                       # the 256-byte step
        n = 760 if c == 2 else 300 + 256 * c                 # the suffix reaches into step c (64 x 64: the cap is 744 bytes)
        for j in range(4):                                   # the place in a lane's group; j = 0 follows the last byte of the lane before (l = 0: of the step before)
            for second in (0x7F, 0xFF):
                ks = sorted({256 * cc + 4 * l + 1 + j for cc in range(c + 1) for l in (0, 1, 31, 63) if 256 * cc + 4 * l + 1 + j <= min(n - 8, 744)})
                cases.append(hc.Case(64, 64, hc.splice(hc._rand(rng, 200), _tail(rng, n, ks, second)), "tail: step <= %d, place %d, %02X" % (c, j, second)))
    for n in (40, 300, 760):                                 # pairs back to back: x7F bytes that are themselves above 0x8F
        ks = list(range(1, min(n - 8, 744), 3))
        cases.append(hc.Case(64, 64, hc.splice(hc._rand(rng, 64), _tail(rng, n, ks, 0xFF)), "tail: every third of %d" % n))
        cases.append(hc.Case(16, 16, hc.splice(hc._rand(rng, 64), _tail(rng, n, ks, 0xFF)), "tail: every third of %d, 16 x 16" % n))
    return cases


def test_the_constructed_tails_mostly_decode(oracle):
    """(no kernel runs here: the oracle alone)"""
    cases = _stuffed_cases()
    ok = sum(1 for c in cases if _want(oracle, c).any())
    print("stuffed tails: %d of %d decode to something" % (ok, len(cases)))
    assert 2 * ok >= len(cases)


def test_stuffed_vlc_tails(ctxs, oracle):
    _check_all_forms(ctxs, oracle, _stuffed_cases(), "stuffed tails")


# ---- plan level: 128 x 128 RGB8, 64 x 64 tiles, 3 resolutions, 32 x 32 code-blocks ---------------------------------------------------------------
GEO = dict(W=128, H=128, nres=3, cb=32, tile=(64, 64))
MARK = -123456789


@pytest.mark.parametrize("form", FORMS, ids=["front%d_lean%d" % f for f in FORMS])
def test_plan_decode_blocks_both_row_modes(ctxs, oracle, form):
    """j2k_plan_decode_blocks, every job's body a stream of its shape (tests/ht_stream_cases.bodies_for: ordinary, refused, u >= 32, damaged):
    rows mode off -- the block is the oracle's; on, into a buffer of markers -- the coded rows are the oracle's and every other row keeps the marker"""
    import torch
    from j2kgfx.codec import FramePlan
    plan = FramePlan(GEO["W"], GEO["H"], 3, precision=8, lossless=True, num_resolutions=GEO["nres"], cb=(GEO["cb"], GEO["cb"]), tile=GEO["tile"], coder=1, ctx=ctxs[form])
    blocks, doffs = plan.blocks(), plan.decoded_offsets()
    n = int(plan.info.blocks)
    cases = hc.bodies_for([(int(b["w"]), int(b["h"])) for b in blocks], 0x7806)
    assert n > 64 and sum(1 for c in cases if _want(oracle, c).any()) * 2 >= n
    data = b"".join(c.data for c in cases)
    ho = np.cumsum([0] + [len(c.data) for c in cases]).astype(np.int64)
    buf = torch.full((len(data) + 8192,), 0xFF, dtype=torch.uint8, device=plan.device)
    buf[4096:4096 + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(plan.device)
    stream, offs = buf[4096:], torch.from_numpy(ho).to(plan.device)
    lens = torch.from_numpy(np.diff(ho).astype(np.int32)).to(plan.device)
    nb = torch.zeros(n, dtype=torch.uint8, device=plan.device)
    for rep in range(2):
        for rows_only in (False, True):
            torch.cuda.synchronize()
            plan.set_decode_coded_rows_only(rows_only)
            out = torch.full((int(plan.info.decoded_elems),), MARK, dtype=torch.int32, device=plan.device)
            plan.decode_blocks(stream, offs, lens, nb, decoded=out)
            plan.ctx.sync()
            got = out.cpu().numpy()
            for j, c in enumerate(cases):
                g = got[int(doffs[j]):int(doffs[j]) + c.w * c.h].reshape(c.h, c.w)
                want = _want(oracle, c)
                assert np.array_equal(g[0::4], want[0::4]), ("coded rows", form, rep, rows_only, j, c.label)
                for r in (1, 2, 3):
                    assert (g[r::4] == (MARK if rows_only else 0)).all(), ("other rows", form, rep, rows_only, j, r, c.label)
    plan.set_decode_coded_rows_only(False)
    plan.close()


@pytest.mark.parametrize("form", FORMS, ids=["front%d_lean%d" % f for f in FORMS])
def test_closed_loop_frame_round_trip(ctxs, oracle, form):
    """pixels -> tile-parts -> pixels through the HT coder (the <true> instantiations of the third kernel behind either front end).  The reference's HT
    coder codes one row in four, so an HT frame does not come back as its input ("not a round trip"): what comes back is held to the
    oracle instead -- the blocks the stage calls decode from the same tile-parts are the oracle's one by one, and the frame decoder's pixels, twice,
    are those blocks placed and inverse-transformed (placement and the 5-3 are pinned to the oracle by their own tests)"""
    import torch
    from closed_loop_ref import frame as make_frame
    from j2kgfx import _lib
    from j2kgfx.codec import FramePlan
    W, H = GEO["W"], GEO["H"]
    frm = make_frame(W, H, 79, noise=40)
    rgba = np.concatenate([frm.transpose(1, 2, 0), np.full((H, W, 1), 255, np.uint8)], axis=2).reshape(H, W * 4)
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=GEO["nres"], cb=(GEO["cb"], GEO["cb"]), tile=GEO["tile"], coder=_lib.CODER_HT, closed_loop=True, ctx=ctxs[form])
    d_pix = torch.from_numpy(np.ascontiguousarray(rgba)).to(plan.device)
    cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA8, d_pix, sop=True, eph=True)
    plan.frame_status()
    total = int(toffs[-1].item())
    o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=toffs, sop=True, eph=True)
    dense = plan.decode_blocks(cs, o2, l2, n2)
    want_pix = plan.inverse_pixels(plan.place_blocks(dense), torch.zeros_like(d_pix))
    plan.frame_status()
    n = int(plan.info.blocks)
    h_cs, p_off, p_len, hd = cs.cpu().numpy(), o2.cpu().numpy()[:n], l2.cpu().numpy()[:n], dense.cpu().numpy()
    blocks, doffs = plan.blocks(), plan.decoded_offsets()
    some = 0
    for j in range(n):
        w, h = int(blocks[j]["w"]), int(blocks[j]["h"])
        want = oracle.ht_decode(h_cs[int(p_off[j]):int(p_off[j]) + int(p_len[j])], w, h)
        some += bool(want.any())
        assert np.array_equal(hd[int(doffs[j]):int(doffs[j]) + w * h].reshape(h, w), want), (form, j, w, h)
    assert some * 2 >= n and want_pix.any()
    for rep in range(2):
        torch.cuda.synchronize()
        back = torch.zeros_like(d_pix)
        plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=True, eph=True)
        plan.frame_status()
        assert torch.equal(back, want_pix), (form, rep)
    plan.close()
