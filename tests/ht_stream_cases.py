"""HT block streams that the encoder never writes (test infrastructure, CPU only): builders, a classifier and the case groups G, V, M, S, E.
Used by tests/test_ht_stream_cases.py (the case lists against the two restatements of the reference) and tests/test_gpu_ht_decode_streams.py
(the three-kernel HT decoder against the C oracle on the same lists).

A block's bytes are `MagSgn segment | suffix`: the suffix is the last SCUP bytes (MEL, VLC, the 12-bit SCUP field in its last two bytes) and alone
fixes every rho and u (ht.go:589-660 reads nothing else); the MagSgn segment only feeds the magnitudes (ht.go:661-710).  So a suffix with a known
largest u can be put behind any MagSgn segment, and the decoder's choices that depend on the one can be driven independently of those that
depend on the other.

classify() restates properties of the STREAM with oracle/pyref.py -- it never looks at the kernels.  Numbers such as 31/32, 64 or 4240 appear here
only as edges of the case lists."""
import functools
import os
from typing import NamedTuple

import numpy as np

import oracle as _orc
import pyref

TABLES = pyref.load_ht_tables(os.path.join(os.path.dirname(os.path.abspath(pyref.__file__)), "ht_tables.h"))


class Case(NamedTuple):
    w: int
    h: int
    data: bytes
    label: str = ""          # how it was made
    rand: bool = False       # suffix of random bytes (counts for the "not everything decodes to zero" cap)
    bucket: str = ""         # M only: "<=31", "=32", ">=33" -- the largest u of its suffix on (w, h)
    expect: str = ""         # V only: the reject reason written down with the case ("none": decoded)


class Info(NamedTuple):
    reject: str              # "len<2", "scup<2", "scup>len", "mel" or "none"
    max_u: int               # largest u of the pairs that exist (0 when rejected)
    seg_len: int             # MagSgn segment length (0 when rejected before SCUP is known)
    n_ff: int                # 0xFF bytes in the MagSgn segment


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def with_scup(buf, scup):
    """the 12-bit SCUP field: low byte in buf[-1], high nibble in the low nibble of buf[-2] (ht.go:104)"""
    b = bytearray(buf)
    b[-1] = scup & 0xFF
    b[-2] = (b[-2] & 0xF0) | ((scup >> 8) & 0x0F)
    return bytes(b)


def scup_of(stream):
    return stream[-1] + ((stream[-2] & 0x0F) << 8)


def split(stream):
    """(magsgn, suffix) of a stream whose SCUP field is valid"""
    scup = scup_of(stream)
    assert 2 <= scup <= len(stream)
    return bytes(stream[:len(stream) - scup]), bytes(stream[len(stream) - scup:])


def splice(magsgn, suffix):
    assert len(suffix) >= 2 and scup_of(suffix) == len(suffix), "a suffix names its own length"
    return bytes(magsgn) + bytes(suffix)


def _rand(rng, n):
    return bytes(rng.integers(0, 256, n).astype(np.uint8))


def _rand_no_ff(rng, n):
    return bytes(rng.integers(0, 255, n).astype(np.uint8))


def random_suffix(rng, n):
    return with_scup(_rand(rng, n), n)


def random_stream(rng, w, h):
    """random bytes with a valid SCUP field: length and SCUP drawn, not constructed"""
    coded = ((h + 3) // 4) * w
    n = int(rng.integers(2, 2 * coded + 48))
    return with_scup(_rand(rng, n), int(rng.integers(2, min(n, 4095) + 1)))


def encoder_output(rng, w, h, amp):
    for _ in range(8):
        x = rng.integers(-amp, amp + 1, (h, w)).astype(np.int32)
        try:
            out = bytes(_orc.ht_encode(x, w, h))
        except ValueError:                                  # input the reference's encoder panics on: draw again, smaller
            amp = max(amp // 2, 1)
            continue
        if len(out) >= 2:
            return out
        amp += 1                                            # (an all-zero block has no bytes)
    raise AssertionError("no encoder output for %dx%d" % (w, h))


# ---- classifier ---------------------------------------------------------------------------------------------------------------------
class _Recorder(pyref.HTDecoder):
    """pyref's decoder, recording what it decides on the way: the MEL start's verdict and every u"""

    def __init__(self, w, h):
        super().__init__(w, h, TABLES)
        self.seen_u = []
        self.mel_ok = None                                   # None: decode() never got as far as the MEL start

    def _init_mel(self, data, lcup, scup):
        self.mel_ok = super()._init_mel(data, lcup, scup)
        return self.mel_ok

    def _uvlc(self, vlc, mode, initial):
        consumed, u = super()._uvlc(vlc, mode, initial)
        self.seen_u.extend(u)
        return consumed, u


def classify(stream, w, h, want_out=False):
    """Info of the stream on a w x h block; want_out: (Info, pyref's decode as int32 [h, w]).  One pyref decode per call, nothing kept:
    callers that ask about a stream twice (the lists' suffixes) hold on to the answer themselves"""
    stream = bytes(stream)
    n = len(stream)
    reject, seg, nff = "none", 0, 0
    if n < 2:
        reject = "len<2"
    else:
        scup = scup_of(stream)
        if scup < 2:
            reject = "scup<2"
        elif scup > n:
            reject = "scup>len"
        else:
            seg = n - scup
            nff = stream[:seg].count(0xFF)
    dec = _Recorder(w, h)
    out = dec.decode(stream)
    max_u = 0
    if reject == "none":
        assert dec.mel_ok is not None, "a stream with a valid SCUP field reaches the MEL start"
        if not dec.mel_ok:
            reject = "mel"
        else:
            max_u = max(dec.seen_u) if dec.seen_u else 1     # (a pair without a u-VLC has u = 1, ht.go:655)
    else:
        assert dec.mel_ok is None, "refused before the MEL start"
    if reject != "none":
        assert not any(out) and not dec.seen_u
    info = Info(reject, max_u, seg, nff)
    if want_out:
        return info, np.array(out, np.int64).astype(np.int32).reshape(h, w)
    return info


def bucket_of(max_u):
    return "<=31" if max_u <= 31 else ("=32" if max_u == 32 else ">=33")


BUCKETS = ("<=31", "=32", ">=33")


# ---- G: geometry ----------------------------------------------------------------------------------------------------------------------
G_SHAPES = [(64, 64), (61, 64), (65, 60), (64, 68), (1024, 4), (1028, 4), (8, 512), (4, 516), (256, 16), (128, 32), (128, 31), (129, 32),
            (57, 8), (62, 4), (63, 4), (5, 8), (7, 4), (3, 5), (13, 9), (33, 9), (1, 1), (2, 1), (1, 9)]


@functools.lru_cache(None)
def group_G():
    rng = np.random.default_rng(0x4701)
    out = []
    for w, h in G_SHAPES:
        for k in range(3):
            out.append(Case(w, h, random_stream(rng, w, h), "G random %d" % k, rand=True))
        out.append(Case(w, h, encoder_output(rng, w, h, 300), "G encoder"))
    return out


# ---- V: validation ----------------------------------------------------------------------------------------------------------------------
# MEL start: initMEL reads num = 4 - (pos & 3) bytes from pos = the MagSgn length and refuses the stream when a byte > 0x8F follows a 0xFF among
# them (ht.go:153-195).  With the 0xFF as byte k of the suffix and the byte > 0x8F behind it, that is: k + 2 <= num.  Written out per (k, pos mod 4):
_MEL_EXPECT = {(0, 0): "mel", (0, 1): "mel", (0, 2): "mel", (0, 3): "none",
               (1, 0): "mel", (1, 1): "mel", (1, 2): "none", (1, 3): "none",
               (2, 0): "mel", (2, 1): "none", (2, 2): "none", (2, 3): "none",
               (3, 0): "none", (3, 1): "none", (3, 2): "none", (3, 3): "none"}


@functools.lru_cache(None)
def group_V():
    rng = np.random.default_rng(0x5601)
    out = []
    for w, h in ((16, 16), (64, 64)):
        out.append(Case(w, h, b"", "V len 0", expect="len<2"))
        out.append(Case(w, h, b"\x5a", "V len 1", expect="len<2"))
        out.append(Case(w, h, with_scup(b"\x50\x00", 2), "V len 2, SCUP 2: empty VLC, empty MagSgn", expect="none"))
        out.append(Case(w, h, with_scup(b"\x12\x50\x00", 2), "V len 3, SCUP 2", expect="none"))
        out.append(Case(w, h, with_scup(b"\x12\x50\x00", 3), "V len 3, SCUP 3", expect="none"))
        out.append(Case(w, h, with_scup(b"\x12\x50\x00", 4), "V len 3, SCUP 4", expect="scup>len"))
        for n in (4095, 5000):
            body = _rand_no_ff(rng, n)                       # (no 0xFF anywhere: the MEL start is accepted wherever the suffix begins)
            # the field has 12 bits: with_scup keeps the low 12 of what it is given, and the expectation is that of the value it holds
            for scup in (0, 1, 2, 3, n - 1, n, n + 1, 4095):
                held = scup & 0xFFF
                exp = "scup<2" if held < 2 else ("scup>len" if held > n else "none")
                out.append(Case(w, h, with_scup(body, scup), "V len %d, SCUP %d (field holds %d)" % (n, scup, held), expect=exp))
        body = _rand_no_ff(rng, 100)
        out.append(Case(w, h, with_scup(body, 101), "V len 100, SCUP 101", expect="scup>len"))
        out.append(Case(w, h, with_scup(body, 4095), "V len 100, SCUP 4095", expect="scup>len"))
        base = 0 if w == 16 else 64
        for m in range(4):
            mag = _rand(rng, base + m)
            for k in range(4):
                for second, name in ((0x90 + int(rng.integers(0, 16)), "9x"), (0xFF, "FF"), (0x8F, "8F")):
                    suf = bytearray(_rand_no_ff(rng, 40))
                    for i in range(len(suf)):
                        if suf[i] > 0x8F and i <= 5:
                            suf[i] &= 0x7F                   # nothing else near the start can be refused or change the expectation
                    suf[k] = 0xFF
                    suf[k + 1] = second
                    exp = "none" if name == "8F" else _MEL_EXPECT[(k, (base + m) & 3)]
                    out.append(Case(w, h, splice(mag, with_scup(bytes(suf), 40)), "V MEL: FF %s at suffix byte %d, MagSgn %d bytes" % (name, k, base + m), expect=exp))
    return out


# ---- M: MagSgn routes -------------------------------------------------------------------------------------------------------------------
M_SHAPES = [(64, 64), (128, 32), (16, 16), (61, 64)]
M_PER_CELL = 6
M_LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257] + list(range(1020, 1029)) + [2047, 2048, 2049] + list(range(4236, 4245)) + [4300, 8000]
M_CONTENTS = ["random", "zeros", "ones", "FF7F", "7FFF", "ff_last", "ff_last_but_one", "ff63", "ff64", "ff65", "ff200"]
M_ALL_CONTENT_LENGTHS = [5, 257, 1025, 4240, 4241]
M_MAX_DRAWS = 4000


@functools.lru_cache(None)
def find_suffixes(w, h, per_cell=M_PER_CELL, max_draws=M_MAX_DRAWS):
    """({bucket: [suffix]}, draws): seeded random suffixes on a w x h block, classified, until every bucket holds per_cell (or max_draws are spent)"""
    rng = np.random.default_rng(0x4D00 + w * 1000 + h)
    pairs = ((h + 3) // 4) * ((((w + 3) // 4) + 1) // 2)
    top = min(6 * pairs + 16, 800)
    found = {b: [] for b in BUCKETS}
    draws = 0
    while draws < max_draws and any(len(found[b]) < per_cell for b in BUCKETS):
        draws += 1
        suf = random_suffix(rng, int(rng.integers(6, top)))
        info, dec = classify(suf, w, h, want_out=True)
        if info.reject != "none" or not dec.any():
            continue                                        # (refused, or nothing significant: says nothing about the MagSgn routes)
        cell = found[bucket_of(info.max_u)]
        if len(cell) < per_cell:
            cell.append(suf)
    return found, draws


def m_suffixes():
    """{(shape, bucket): [suffix] * M_PER_CELL}; the number of draws it took per shape in ["draws"]"""
    cells = {"draws": {}}
    for shape in M_SHAPES:
        found, cells["draws"][shape] = find_suffixes(*shape)
        for b in BUCKETS:
            cells[(shape, b)] = found[b]
    return cells


def magsgn_content(rng, kind, n):
    if kind == "random":
        return _rand(rng, n)
    if kind == "zeros":
        return bytes(n)
    if kind == "ones":
        return b"\xff" * n
    if kind == "FF7F":
        return (b"\xff\x7f" * (n // 2 + 1))[:n]
    if kind == "7FFF":
        return (b"\x7f\xff" * (n // 2 + 1))[:n]
    b = bytearray(_rand(rng, n))
    if kind == "ff_last":
        if n >= 1: b[-1] = 0xFF
        return bytes(b)
    if kind == "ff_last_but_one":
        if n >= 2: b[-2] = 0xFF
        return bytes(b)
    assert kind.startswith("ff")
    cnt = min(int(kind[2:]), n)                              # exactly cnt bytes of 0xFF (all of them when the segment is shorter)
    b = bytearray(_rand_no_ff(rng, n))
    for i in rng.choice(n, cnt, replace=False) if n else []:
        b[int(i)] = 0xFF
    return bytes(b)


@functools.lru_cache(None)
def group_M():
    """the cross product suffix x length x content, thinned: every length with random content and every content at M_ALL_CONTENT_LENGTHS, each such
    (length, content) in front of 18 of the 72 suffixes -- one per (shape, bucket) cell, by turns, and a second one in half of the cells"""
    cells = m_suffixes()
    rng = np.random.default_rng(0x4D02)
    combos = [(n, "random") for n in M_LENGTHS] + [(n, c) for n in M_ALL_CONTENT_LENGTHS for c in M_CONTENTS if c != "random"]
    out = []
    for ci, (n, kind) in enumerate(combos):
        for si, shape in enumerate(M_SHAPES):
            for bi, b in enumerate(BUCKETS):
                sufs = cells[(shape, b)]
                picks = [ci % M_PER_CELL] + ([(ci + 3) % M_PER_CELL] if (si * 3 + bi + ci) % 2 == 0 else [])
                for p in picks:
                    if p < len(sufs):
                        out.append(Case(shape[0], shape[1], splice(magsgn_content(rng, kind, n), sufs[p]),
                                        "M %s x %d, suffix %d of %s" % (kind, n, p, b), rand=True, bucket=b))
    return out


# ---- S: VLC routes ----------------------------------------------------------------------------------------------------------------------
S_LENGTHS = ([((64, 64), n) for n in (2, 3, 4, 5, 6)] + [((4, 4), n) for n in (2, 3, 4, 5, 6)] + [((4, 4), n) for n in range(14, 19)] +
             [((64, 64), n) for n in list(range(255, 263)) + list(range(511, 519)) + list(range(745, 761)) + [2000, 4095]] + [((4, 4), 2000), ((4, 4), 4095)])
S_CONTENTS = ["random", "zeros", "ones", "7F", "FF7F", "907F", "big_7F"]


def suffix_content(rng, kind, n):
    if kind == "random":
        b = _rand(rng, n)
    elif kind == "zeros":
        b = bytes(n)
    elif kind == "ones":
        b = b"\xff" * n
    elif kind == "7F":
        b = b"\x7f" * n
    elif kind == "FF7F":
        b = (b"\xff\x7f" * (n // 2 + 1))[:n]
    elif kind == "907F":
        b = (b"\x90\x7f" * (n // 2 + 1))[:n]
    else:                                                   # bytes > 0x8F on even positions, x7F (0x7F or 0xFF) on odd ones: the 7-bit rule at every second byte
        a = bytearray(n)
        for i in range(n):
            a[i] = int(rng.integers(0x90, 0x100)) if i % 2 == 0 else (0x7F | (int(rng.integers(0, 2)) << 7))
        b = bytes(a)
    return with_scup(b, n)


@functools.lru_cache(None)
def group_S():
    rng = np.random.default_rng(0x5301)
    mag = _rand(rng, 64)
    out = []
    for (w, h), n in S_LENGTHS:
        for kind in S_CONTENTS:
            out.append(Case(w, h, splice(mag, suffix_content(rng, kind, n)), "S %s suffix of %d" % (kind, n), rand=(kind == "random")))
    return out


# ---- E: damaged encoder output -----------------------------------------------------------------------------------------------------------
E_SHAPES = [(64, 64), (64, 61), (60, 64), (40, 17), (16, 9)]
E_AMPS = (3, 300, 40000)
E_VARIANTS = 40
E_KINDS = ["overwrite", "cut_head", "cut_tail", "cut_tail_scup", "scup_ones", "scup_zero", "flip_middle"]


def damage(rng, good, kind):
    b = bytearray(good)
    n = len(b)
    if kind == "overwrite":
        for _ in range(int(rng.integers(1, 9))):
            b[int(rng.integers(0, n))] = int(rng.integers(0, 256))
    elif kind == "cut_head":
        b = b[int(rng.integers(1, max(n - 1, 2))):]
    elif kind in ("cut_tail", "cut_tail_scup"):
        b = b[:n - int(rng.integers(1, max(n - 1, 2)))]
        if kind == "cut_tail_scup" and len(b) >= 2:
            b = bytearray(with_scup(b, int(rng.integers(2, min(len(b), 4095) + 1))))
    elif kind == "scup_ones":                               # the two kinds of test_plan_decode_coded_rows_only[corrupt] that touch SCUP ...
        b[-1] = 0xFF; b[-2] |= 0x0F
    elif kind == "scup_zero":
        b[-1] = 0; b[-2] &= 0xF0
    else:                                                   # ... and its third: eight bytes in the middle flipped
        for i in range(n // 2, min(n // 2 + 8, n)):
            b[i] ^= 0x5A
    return bytes(b)


@functools.lru_cache(None)
def group_E():
    rng = np.random.default_rng(0x4501)
    out = []
    for w, h in E_SHAPES:
        for amp in E_AMPS:
            good = encoder_output(rng, w, h, amp)
            for v in range(E_VARIANTS):
                kind = E_KINDS[v % len(E_KINDS)]
                out.append(Case(w, h, damage(rng, good, kind), "E amp %d %s" % (amp, kind)))
    return out


GROUPS = {"G": group_G, "V": group_V, "M": group_M, "S": group_S, "E": group_E}


# ---- one case per job of a plan (the plan and closed-loop tests; their supply is checked on the CPU) ------------------------------------------------
PLANS = [dict(W=328, H=211, cb=64, tile=(0, 0), nres=3), dict(W=200, H=150, cb=16, tile=(64, 64), nres=3)]
# sources by turns; "!": M streams with more than 64 bytes of 0xFF in the MagSgn segment or a segment beyond 4240 bytes
_TURNS = ["=32", ">=33!", "<=31", "=32!", ">=33", "S", "refused", "=32", ">=33!", "E", "=32!", ">=33", "G", "V", "<=31!"]


def is_large(w, h):
    return ((h + 3) // 4) * w > 1024 or ((h + 3) // 4) * ((((w + 3) // 4) + 1) // 2) > 128


@functools.lru_cache(None)
def pools():
    """{(w, h): {source: [case]}} of G, V (and its refused cases on their own), M (per bucket), S, E"""
    out = {}
    def add(c, src):
        out.setdefault((c.w, c.h), {}).setdefault(src, []).append(c)
    for g in ("G", "V", "S", "E"):
        for c in GROUPS[g]():
            add(c, g)
    for c in group_V():
        if c.expect != "none":
            add(c, "refused")
    for c in group_M():
        mag = split(c.data)[0]
        add(c, c.bucket + ("!" if mag.count(0xFF) > 64 or len(mag) > 4240 else ""))
    return out


def bodies_for(shapes, seed, keep=None):
    """one case per job, shapes[j] = (w, h): of the job's shape from the groups, by turns over their sources; a shape no group has gets streams
    made here the same ways (random with a valid SCUP field, damaged encoder output, refused by SCUP, a suffix of that shape with a known
    largest u behind a MagSgn segment).  keep[j]: leave job j alone (None in the result)"""
    rng = np.random.default_rng(seed)
    turn = {}
    out = []
    for j, (w, h) in enumerate(shapes):
        if keep is not None and keep[j]:
            out.append(None)
            continue
        pool = pools().get((w, h))
        k = turn.get((w, h), 0)
        if not pool:
            turn[(w, h)] = k + 1
            data = random_stream(rng, w, h)
            if k % 4 == 0:
                data = damage(rng, encoder_output(rng, w, h, 300), E_KINDS[(k // 4) % 7])
            elif k % 4 == 1:                                  # refused by its SCUP field
                data = with_scup(data, [0, 1, len(data) + 1, 4095 if len(data) < 4095 else 0][(k // 4) % 4])
            elif k % 4 == 2:
                found = find_suffixes(w, h, 2, 600)[0]
                sufs = found[BUCKETS[1 + (k // 4) % 2]] or found["<=31"]
                if sufs:
                    kind, n = [("random", 1025), ("ff64", 257), ("ones", 257), ("random", 4241), ("ff65", 1025), ("FF7F", 5)][(k // 4) % 6]
                    data = splice(magsgn_content(rng, kind, n), sufs[(k // 8) % len(sufs)])
            out.append(Case(w, h, data, "made for %dx%d" % (w, h)))
            continue
        while True:
            src = _TURNS[k % len(_TURNS)]
            k += 1
            if pool.get(src):
                break
        turn[(w, h)] = k
        out.append(pool[src][int(rng.integers(0, len(pool[src])))])
    return out


def kinds(cases):
    """blocks per kind, from the streams' properties: large / refused / the bucket of the largest u, and how many of the blocks with a u of 32 and
    more carry more than 64 bytes of 0xFF or a segment beyond 4240 bytes"""
    n = {k: 0 for k in ("large", "refused", "far") + BUCKETS}
    for c in cases:
        info = classify(c.data, c.w, c.h)
        if is_large(c.w, c.h):
            n["large"] += 1
        elif info.reject != "none":
            n["refused"] += 1
        else:
            n[bucket_of(info.max_u)] += 1
            if info.max_u >= 32 and (info.n_ff > 64 or info.seg_len > 4240):
                n["far"] += 1
    return n
