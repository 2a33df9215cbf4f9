"""CPU: tests/raw_magref_cases.py, the definition of the raw-MagRef coding style (j2k_plan_set_raw_magref), holds together -- round trips, the
RAW part against the oracle's raw_encode, the total-function rules on truncated and random bodies, the golden digests.  The device is held
against the same definition by tests/test_gpu_raw_magref.py."""
import hashlib
import json
import os

import numpy as np
import pytest

import coarse_cases as cc
import raw_magref_cases as rm

BANDS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def t2ref():
    import t2ref as t
    return t


@pytest.mark.parametrize("kind", rm.CONTENTS)
def test_round_trip_and_numbps(oracle, kind):
    """decode_block(encode_block(x)) == x, numbps is the oracle's t1_encode's, on every shape and band"""
    for w, h in rm.SHAPES:
        for band in BANDS if (w, h) in ((33, 17), (4, 4)) else (band_of(w, h),):
            x = rm.block_content(kind, w, h)
            body, nb = rm.encode_block(x, w, h, band, oracle)
            assert nb == oracle.t1_encode(x, w, h, band)[1], (w, h, band)
            assert (len(body) == 0) == (nb == 0)
            assert np.array_equal(rm.decode_block(body, nb, band, w, h, oracle), x), (w, h, band)


def band_of(w, h):
    return (w + 2 * h) % 4


@pytest.mark.parametrize("kind", ["spike", "all7fff", "all4000", "noise12", "deep"])
def test_body_layout(oracle, kind):
    """H holds len(MQ) in 7-bit groups below 0x80; RAW is the oracle's raw_encode of the diverted bits; MQ is the codeword of the rest"""
    for w, h in ((33, 17), (64, 64), (1, 1)):
        x = rm.block_content(kind, w, h)
        body, nb = rm.encode_block(x, w, h, 1, oracle)
        mq, bits, nb2 = rm.encode_parts(x, w, h, 1)
        assert nb == nb2 and all(b < 0x80 for b in body[:3])
        m = body[0] << 14 | body[1] << 7 | body[2]
        assert m == len(mq) and body[3:3 + m] == mq
        assert body[3 + m:] == (bytes(oracle.raw_encode(bits)) if bits.size else b"")
        assert rm.split_body(body) == (mq, body[3 + m:])
        if kind == "all7fff" and w * h > 8:
            assert body[3 + m:3 + m + 4] == b"\xff\x7f\xff\x7f"         # every refinement bit 1: stuffing after every 0xFF
        if kind == "all4000":
            assert not any(body[3 + m:])


def test_total_function_rules(oracle):
    """short bodies, m beyond the body, truncated bodies, a 0xFF 0x90 pair in RAW: decode_block is defined, and is what the rules say"""
    w, h, band = 8, 8, 2
    x = rm.block_content("noise12", w, h)
    body, nb = rm.encode_block(x, w, h, band, oracle)
    mq, raw = rm.split_body(body)
    # a body shorter than the header: empty MQ and RAW, whatever its bytes
    empty = rm.decode_block(b"", nb, band, w, h, oracle)
    for short in (b"\x00", b"\x7f\x7f", b"\xff\xff"):
        assert rm.split_body(short) == (b"", b"")
        assert np.array_equal(rm.decode_block(short, nb, band, w, h, oracle), empty)
    # m beyond the body: clamped, RAW empty -> the raw reader returns ones
    over = rm.header(len(body) + 100) + body[3:]
    assert rm.split_body(over) == (body[3:], b"")
    # truncation anywhere decodes; cutting RAW only changes refinement bits (the MQ part, hence every significance and sign, is intact)
    full = rm.decode_block(body, nb, band, w, h, oracle)
    assert np.array_equal(full, x)
    for cut in range(len(body) + 1):
        got = rm.decode_block(body[:cut], nb, band, w, h, oracle)
        assert got.shape == (h, w)
        if cut >= 3 + len(mq):
            assert np.array_equal(np.sign(got), np.sign(x))
            assert np.array_equal(np.abs(got) >> (nb - 1) > 0, np.abs(x) >> (nb - 1) > 0)
    # 0xFF followed by a byte above 0x8F inside RAW: ones from there on (RawDecoder.DecodeBit, mqc.go:535-562)
    bad = rm.header(len(mq)) + mq + b"\xff\x90" + raw
    ones = rm.header(len(mq)) + mq + b"\xff"
    assert np.array_equal(rm.decode_block(bad, nb, band, w, h, oracle), rm.decode_block(ones, nb, band, w, h, oracle))
    # random bodies
    for fb, fnb in rm.foreign_bodies(60):
        assert rm.decode_block(fb, fnb, band, w, h, oracle).shape == (h, w)


def test_foreign_bodies_cover_the_rules():
    bodies = rm.foreign_bodies()
    assert len(bodies) >= 300
    beyond = ff90 = short = 0
    for b, nb in bodies:
        assert 0 <= len(b) <= 40 and 1 <= nb <= 12
        if len(b) < 3:
            short += 1
            continue
        m = b[0] << 14 | b[1] << 7 | b[2]
        beyond += m > len(b) - 3
        raw = rm.split_body(b)[1]
        ff90 += any(raw[i] == 0xFF and raw[i + 1] > 0x8F for i in range(len(raw) - 1))
    assert beyond >= 20 and ff90 >= 20 and short >= 5


@pytest.mark.parametrize("k", [1, 3, 12, 31])
def test_skip_planes_is_coarse_of_the_full_decode(oracle, k):
    """the style keeps 'all three passes of a plane or none': stopping k planes early = coarse(full decode, k).  The definition's own decoder
    stopped early (numbps - k planes decoded, magnitudes shifted back by the caller) says the same."""
    w, h, band = 33, 17, 3
    x = rm.block_content("noise12", w, h)
    body, nb = rm.encode_block(x, w, h, band, oracle)
    want = cc.coarse(x, k)
    # a decoder that runs nb - k planes sees the same decisions in the same order; its samples are the top planes of the full decode
    if k < nb:
        top = rm.decode_block(body, nb - k, band, w, h, oracle).astype(np.int64)
        mid = 1 << (k - 1)
        got = np.where(top != 0, np.sign(top) * ((np.abs(top) << k) | mid), 0).astype(np.int32)
        assert np.array_equal(got, want)
    else:
        assert not want.any()


def test_frames_sizes_and_golden(oracle, t2ref):
    """prints the size table (plain codeword vs style, header included) of the frames the GPU tests use; the golden digests are the definition's"""
    print()
    print("%-18s %8s %8s %7s" % ("frame", "plain", "style", "change"))
    for name in rm.FRAMES:
        _, want = rm.frame_want(name, oracle, t2ref)
        _, plain = rm.frame_want(name, oracle, t2ref, style=False)
        a = sum(len(plain[t]["bytes"]) for t in plain)
        b = sum(len(want[t]["bytes"]) for t in want)
        for t in want:
            assert np.array_equal(want[t]["numbps"], plain[t]["numbps"])
            assert np.array_equal(want[t]["lens"] == 0, plain[t]["lens"] == 0)
        print("%-18s %8d %8d %+6.1f%%" % (name, a, b, 100.0 * (b - a) / a))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", rm.GOLDEN_FILE)
    with open(path) as f:
        gold = json.load(f)
    for name in rm.GOLDEN_FRAMES:
        sop, eph = rm.GOLDEN_FLAGS[name]
        s = rm.frame_stream(name, sop, eph, oracle, t2ref)
        assert gold[name] == dict(sop=sop, eph=eph, bytes=len(s), sha256=hashlib.sha256(s).hexdigest()), name


def test_frame_bodies_decode_to_the_coefficients(oracle, t2ref):
    """every body of a frame decodes, by the definition, to the window it was coded from"""
    c = rm.FRAMES["gray16_96x40"]
    _, want = rm.frame_want("gray16_96x40", oracle, t2ref)
    wt = want[0]
    jobs = oracle.enumerate_blocks(1, wt["w"], wt["h"], c["nres"], c["cb"], c["cb"], 1)
    pos = 0
    for k, j in enumerate(jobs):
        ln = int(wt["lens"][k])
        got = rm.decode_block(bytes(wt["bytes"][pos:pos + ln]), int(wt["numbps"][k]), int(j["band"]), int(j["w"]), int(j["h"]), oracle)
        assert np.array_equal(got, rm.extract(wt["coeff"][0], wt["w"], wt["h"], j)), k
        pos += ln
