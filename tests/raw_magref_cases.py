"""The definition of the raw-MagRef coding style (j2k_plan_set_raw_magref, FramePlan(raw_magref=True)), importable without a GPU:
tests/test_raw_magref_cases.py checks it on the CPU, tests/test_gpu_raw_magref.py holds the device against it bit for bit.

The style is the reference's T1 (oracle/pyref.py T1.encode / T1.decode: decisions, their order, numbps and the contexts of every symbol that is
not a refinement, all unchanged) with two differences.

1. A decision the reference codes in context CTX_MAG0, CTX_MAG1 or CTX_MAG2 never reaches the MQ coder.  It is appended, in coding order across
   all bit planes, to one raw bit string per block, which is coded as the reference's RawEncoder codes it (mqc.go:560-600: MSB first, a 7-bit
   byte after every 0xFF, Flush as written) -- here through the oracle's raw_encode, the restatement the reference's own vectors pin.  The MQ
   coder codes the remaining symbols as if the diverted ones had never existed: one codeword, one flush.
2. A block's body is H | MQ | RAW.  H is three bytes holding m = len(MQ) in 7-bit groups, most significant first: (m >> 14) & 0x7F,
   (m >> 7) & 0x7F, m & 0x7F -- every byte below 0x80, so no marker pattern begins in the header.  RAW takes the rest of the body.  A block
   without bit planes has an empty body.

The decoder is a total function of (bytes, numbps):
  * a body shorter than three bytes has empty MQ and RAW (its bytes are ignored);
  * m is clamped to len(body) - 3;
  * past the end of MQ the MQ decoder reads what the reference's reads (mqc.go:402-439; pyref.MQDecoder._byte_in);
  * past the end of RAW, and after a 0xFF followed by a byte above 0x8F, the raw reader does what RawDecoder.DecodeBit does (mqc.go:535-562):
    it stays at 0xFF and returns ones (the oracle's raw_decode).

Everything above the block body -- packet headers, lens, numbps, zero bit planes, the pass count 3 * numbps - 2, SOP / EPH, tile-parts -- is the
plain codec's: frames are closed_loop_ref.oracle_frame / mallat_cases.oracle_frame with the block coder swapped (RawMagrefOracle).  The style
keeps "all three passes of a plane or none", so a decode with skip_planes = k is coarse_cases.coarse(full decode, k)."""
import contextlib

import numpy as np

import pyref

MAG_CTXS = (pyref.CTX_MAG0, pyref.CTX_MAG1, pyref.CTX_MAG2)
HEADER = 3


@contextlib.contextmanager
def _coders(enc=None, dec=None):
    """pyref.MQEncoder / pyref.MQDecoder replaced for the duration of a call"""
    old = pyref.MQEncoder, pyref.MQDecoder
    try:
        if enc is not None:
            pyref.MQEncoder = enc
        if dec is not None:
            pyref.MQDecoder = dec
        yield
    finally:
        pyref.MQEncoder, pyref.MQDecoder = old


def header(m):
    assert 0 <= m < 1 << 21
    return bytes(((m >> 14) & 0x7F, (m >> 7) & 0x7F, m & 0x7F))


def split_body(body):
    """body -> (MQ, RAW) by the total-function rules"""
    body = bytes(body)
    if len(body) < HEADER:
        return b"", b""
    m = min(body[0] << 14 | body[1] << 7 | body[2], len(body) - HEADER)      # (foreign bytes may be >= 0x80: the groups then overlap, by this formula)
    return body[HEADER:HEADER + m], body[HEADER + m:]


def encode_parts(data, w, h, band):
    """(MQ bytes, diverted bits uint8, numbps) of one block"""
    bits = []

    class Enc(pyref.MQEncoder):
        def encode(self, ctx, decision):
            if ctx in MAG_CTXS:
                bits.append(int(decision))
            else:
                super().encode(ctx, decision)

    t = pyref.T1(w, h)
    t.set_data([int(v) for v in np.asarray(data).reshape(-1)])
    with _coders(enc=Enc):
        mq, numbps = t.encode(band)
    return bytes(mq), np.array(bits, np.uint8), int(numbps)


def encode_block(data, w, h, band, orc=None):
    """-> (body bytes, numbps)"""
    orc = orc or _oracle()
    mq, bits, numbps = encode_parts(data, w, h, band)
    if numbps == 0:
        return b"", 0
    raw = bytes(orc.raw_encode(bits)) if bits.size else b""
    return header(len(mq)) + mq + raw, numbps


def decode_block(body, numbps, band, w, h, orc=None):
    """-> samples int32 [h, w]"""
    orc = orc or _oracle()
    mq, raw = split_body(body)
    nbits = max(int(numbps), 0) * w * h                          # no block refines more than every sample in every plane
    bits = orc.raw_decode(np.frombuffer(raw, np.uint8), nbits) if nbits else np.zeros(0, np.uint8)
    pos = [0]

    class Dec(pyref.MQDecoder):
        def decode(self, ctx):
            if ctx in MAG_CTXS:
                pos[0] += 1
                return int(bits[pos[0] - 1])
            return super().decode(ctx)

    with _coders(dec=Dec):
        out = pyref.T1(w, h).decode(mq, int(numbps), band)
    return np.array(out, np.int64).astype(np.int32).reshape(h, w)


def _oracle():
    import oracle
    return oracle


def extract(plane, pw, ph, job):
    """encoder.go:763-795: the block's window of a plane, zero beyond the plane"""
    x0, y0, w, h = int(job["x0"]), int(job["y0"]), int(job["w"]), int(job["h"])
    out = np.zeros((h, w), np.int32)
    p = np.asarray(plane, np.int32).reshape(ph, pw)
    ww, hh = max(min(w, pw - x0), 0), max(min(h, ph - y0), 0)
    out[:hh, :ww] = p[y0:y0 + hh, x0:x0 + ww]
    return out


def encode_tile_blocks(orc, planes, w, h, nres, cbw, cbh, windows):
    """oracle.encode_tile_blocks in the style: (bytes, lens uint32, numbps uint8) over the oracle's own job list"""
    jobs = orc.enumerate_blocks(len(planes), w, h, nres, cbw, cbh, windows)
    by, lens, nb = [], [], []
    for j in jobs:
        body, n = encode_block(extract(planes[int(j["comp"])], w, h, j), int(j["w"]), int(j["h"]), int(j["band"]), orc)
        by.append(body); lens.append(len(body)); nb.append(n)
    return np.frombuffer(b"".join(by), np.uint8).copy(), np.array(lens, np.uint32), np.array(nb, np.uint8)


class RawMagrefOracle:
    """the oracle with the MQ block coder of encode_tile_blocks swapped for encode_block: whatever a frame composer does around it stays its own"""

    def __init__(self, oracle):
        self._o = oracle

    def __getattr__(self, name):
        return getattr(self._o, name)

    def encode_tile_blocks(self, planes, w, h, num_resolutions, cb_w, cb_h, coder, windows=0):
        assert coder == 0, "the style is the MQ coder's"
        return encode_tile_blocks(self._o, planes, w, h, num_resolutions, cb_w, cb_h, windows)


def oracle_frame(frm, W, H, tw, th, nres, cb, sop, eph, orc, t2ref, mallat=False, **kw):
    """closed_loop_ref.oracle_frame (mallat: mallat_cases.oracle_frame) in the style: per tile dict(coeff, bytes, lens, numbps, part, w, h, x0, y0)"""
    import closed_loop_ref as ref
    import mallat_cases as mc
    o = RawMagrefOracle(orc)
    if mallat:
        return mc.oracle_frame(frm, W, H, tw, th, nres, cb, 0, sop, eph, o, t2ref, **kw)
    return ref.oracle_frame(frm, W, H, tw or W, th or H, nres, cb, 0, sop, eph, o, t2ref, **kw)


def repacket(want, nres, cb, sop, eph, orc, t2ref):
    """the tile-parts of oracle_frame's tiles with other SOP / EPH flags, without coding the blocks again: the packet loop of
    closed_loop_ref.oracle_frame over the same bodies"""
    out = {}
    for t in sorted(want):
        wt = want[t]
        jobs = orc.enumerate_blocks(len(wt["coeff"]), wt["w"], wt["h"], nres, cb, cb, 1)
        enc = t2ref.PacketEncoder(len_bits=5)
        pos, j = 0, 0
        while j < len(jobs):
            k = j
            blocks = []
            while k < len(jobs) and jobs[k]["comp"] == jobs[j]["comp"] and jobs[k]["res"] == jobs[j]["res"]:
                ln, n_b = int(wt["lens"][k]), int(wt["numbps"][k])
                blocks.append(t2ref.CodeBlock(bytes(wt["bytes"][pos:pos + ln]), 1 if ln == 0 else 0, max(31 - n_b, 0), 0 if n_b == 0 else 3 * n_b - 2))
                pos += ln
                k += 1
            enc.encode_packet(t2ref.Precinct([blocks]), 0, sop, eph)
            j = k
        out[t] = dict(wt, part=orc.create_tile_header(t, bytes(enc.out)))
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 64), (64, 1), (3, 5), (4, 4), (33, 17), (64, 64))          # (w, h)
CONTENTS = ("zeros", "spike", "all7fff", "all4000", "noise12", "deep")


def block_content(kind, w, h, seed=0):
    """int32 [h, w]"""
    d = np.zeros((h, w), np.int32)
    if kind == "zeros":
        return d
    if kind == "spike":
        d[h // 2, w // 3] = -37
        return d
    if kind == "all7fff":                   # every refinement bit 1: the raw string is FF 7F FF 7F ... (stuffing)
        return np.full((h, w), 0x7FFF, np.int32)
    if kind == "all4000":                   # every refinement bit 0
        return np.full((h, w), 0x4000, np.int32)
    if kind == "noise12":
        rng = np.random.default_rng(1000 + seed + 64 * w + h)
        return rng.integers(-(1 << 11), 1 << 11, (h, w)).astype(np.int32)
    if kind == "deep":                      # one sample of 2^30 among zeros: 31 planes
        d[h - 1, w - 1] = 1 << 30
        return d
    raise ValueError(kind)


def foreign_bodies(count=300, seed=77):
    """[(body bytes, numbps)]: random byte strings of length 0 ... 40 as block bodies, numbps 1 ... 12; among them bodies whose m lies beyond the
    body and bodies with a 0xFF 0x90 pair inside RAW"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(0, 41))
        b = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        kind = i % 4
        if kind == 1 and n >= 3:            # a well-formed header, m inside the body
            b[0:3] = header(int(rng.integers(0, n - 2)))
        elif kind == 2 and n >= 3:          # m beyond the body
            b[0:3] = header(n + int(rng.integers(0, 5000)))
        elif kind == 3 and n >= 8:          # 0xFF 0x90 inside RAW
            m = int(rng.integers(0, n - 7))
            b[0:3] = header(m)
            at = 3 + m + int(rng.integers(0, n - 3 - m - 1))
            b[at] = 0xFF; b[at + 1] = 0x90 + int(rng.integers(0, 0x70))
        out.append((bytes(b), int(rng.integers(1, 13))))
    return out


# frames: name -> dict(W, H, comps, prec, tile, cb, nres, mallat, lossless, quality, seed, noise, closed_loop)
FRAMES = {
    "mallat_130x70": dict(W=130, H=70, comps=3, prec=8, tile=(64, 32), cb=32, nres=4, mallat=True, lossless=True, quality=0, seed=401, noise=16),
    "prefix_130x70": dict(W=130, H=70, comps=3, prec=8, tile=(64, 32), cb=32, nres=4, mallat=False, lossless=True, quality=0, seed=402, noise=16),
    "gray16_96x40": dict(W=96, H=40, comps=1, prec=16, tile=(0, 0), cb=32, nres=3, mallat=False, lossless=True, quality=0, seed=403, noise=None),
    "lossy_q75_64x48": dict(W=64, H=48, comps=3, prec=8, tile=(0, 0), cb=32, nres=3, mallat=True, lossless=False, quality=75, seed=404, noise=16),
}
GOLDEN_FRAMES = ("mallat_130x70", "gray16_96x40", "lossy_q75_64x48")          # (name, sop, eph) = (.., False, False) except the first: SOP + EPH
GOLDEN_FLAGS = {"mallat_130x70": (True, True), "gray16_96x40": (False, False), "lossy_q75_64x48": (False, False)}
GOLDEN_FILE = "closed_loop_raw_magref_v1.json"


def frame_pixels(case, orc):
    """(pix uint8 [H, row] in the Go Pix layout of the case's components and precision, the samples an encoder reads from it int32 [C, H, W])"""
    import closed_loop_ref as ref
    import mallat_cases as mc
    if case["comps"] == 3 and case["prec"] == 8:
        vals = ref.frame(case["W"], case["H"], case["seed"], noise=case["noise"]).astype(np.int32)
    else:
        # (decoder.createImage's v * 65535 / 65535 wraps in int32 above 32768, decoder.go:434-451: a 16-bit frame keeps to 15 bits of range, so
        #  that the pixels a lossless decode writes are the pixels the encoder read)
        vals = ref.frame_n(case["W"], case["H"], case["comps"], min(case["prec"], 15), case["seed"], case["noise"])
    pix = orc.create_image([vals[c] for c in range(vals.shape[0])], case["prec"])
    planes = np.stack(orc.extract_image_data(pix, mc.PIX_FORMAT[(case["comps"], case["prec"])], case["W"], case["H"]))[:case["comps"]]
    return np.ascontiguousarray(pix), planes.astype(np.int32)


_frames = {}


def frame_want(name, orc, t2ref, style=True):
    """(samples int32 [C, H, W], oracle_frame's tiles with bare packets) of a case of FRAMES, computed once per process; style = False: the plain codec's"""
    key = (name, style)
    if key not in _frames:
        import closed_loop_ref as ref
        import mallat_cases as mc
        c = FRAMES[name]
        frm = frame_pixels(c, orc)[1]
        kw = dict(precision=c["prec"], lossless=c["lossless"], quality=c["quality"])
        tw, th = c["tile"]
        if style:
            want = oracle_frame(frm, c["W"], c["H"], tw, th, c["nres"], c["cb"], False, False, orc, t2ref, mallat=c["mallat"], **kw)
        elif c["mallat"]:
            want = mc.oracle_frame(frm, c["W"], c["H"], tw, th, c["nres"], c["cb"], 0, False, False, orc, t2ref, **kw)
        else:
            want = ref.oracle_frame(frm, c["W"], c["H"], tw or c["W"], th or c["H"], c["nres"], c["cb"], 0, False, False, orc, t2ref, **kw)
        _frames[key] = (frm, want)
    return _frames[key]


def frame_stream(name, sop, eph, orc, t2ref):
    """the definition's tile-parts of a case end to end"""
    c = FRAMES[name]
    _, want = frame_want(name, orc, t2ref)
    if sop or eph:
        want = repacket(want, c["nres"], c["cb"], sop, eph, orc, t2ref)
    return b"".join(want[t]["part"] for t in sorted(want))
