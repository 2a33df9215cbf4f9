"""HT block decode, what a verified follower costs (option ht_dec_dedup; csrc/ht.hip: ht_vlcprep_dedup_kernel's read-set compare, ht_walk_kernel<true>'s
slot order, a leader that leaves the lean path in ht_decode_lean_kernel<false, true>): the definitions the tests use, restated in Python, and the case lists.  CPU only.

  READ SET of a block of `n` bytes on a w x h code-block (scup = its 12-bit field, nvlc = min(scup - 2, (46 N + 7) // 8 + 8), N = its quad pairs):
      A = [0, min(n, n - scup + 4))      the MagSgn segment and the four bytes at the MEL start
      B = [n - 2 - nvlc, n)              the VLC bytes the prep's string takes, and the trailer
      when A reaches B: [0, n).  What lies between them -- the interior of the MEL run -- no decode path reads.
  WALK ORDER of a plan: the jobs that are their own leader (ht_dedup_cases.leaders) in ascending order, then the others, ascending; walk workgroup g
      takes slots 64 g .. 64 g + 63, and a workgroup whose first slot is at or behind the number of leaders holds followers only.

Nothing here looks at a kernel: positions come from the stream, and what a flip does to the result is asked of the C oracle alone (test_ht_follow_cases.py)."""
import functools
from typing import NamedTuple, Optional

import numpy as np

import ht_dedup_cases as dc
import ht_stream_cases as hc
import oracle as _orc

WALK_BLOCKS = 64


# ---- the walk order -----------------------------------------------------------------------------------------------------------------------
def walk_order(leaders):
    """(order, n_leaders): order[s] = the job of slot s"""
    lead = [j for j, L in enumerate(leaders) if L == j]
    return lead + [j for j, L in enumerate(leaders) if L != j], len(lead)


def follower_only_groups(order, n_leaders):
    """[(g, [jobs of its slots])] of the walk workgroups that hold static followers only"""
    out = []
    for g in range((len(order) + WALK_BLOCKS - 1) // WALK_BLOCKS):
        if g * WALK_BLOCKS >= n_leaders:
            out.append((g, order[g * WALK_BLOCKS:(g + 1) * WALK_BLOCKS]))
    return out


# one-component, one-tile HT plans by their count of non-follower jobs: FramePlan(W, H, 1, num_resolutions=nres, cb=cb); found by running the rule over
# frame sizes (test_ht_follow_cases.py asserts the counts and what each is for)
WALK_PLANS = {
    1: dict(W=15, H=15, nres=2, cb=(8, 8)),        # 4 jobs: one workgroup, its leader in lane 0
    63: dict(W=81, H=72, nres=5, cb=(8, 8)),       # 133 jobs: the leaders end in lane 62 of workgroup 0; workgroup 1 followers only; the last one partial (5 slots)
    64: dict(W=127, H=127, nres=2, cb=(8, 8)),     # 256 jobs: workgroup 0 exactly full of leaders, three workgroups of followers
    65: dict(W=113, H=72, nres=3, cb=(8, 8)),      # 168 jobs: one leader in workgroup 1 (a leader workgroup), the partial workgroup 2 followers only
    129: dict(W=60, H=121, nres=3, cb=(8, 4)),     # 256 jobs: two full leader workgroups and one leader in the third; the fourth followers only
}


def plan_rule(g):
    blocks = dc.block_list(g["W"], g["H"], g["nres"], g["cb"])
    return blocks, dc.leaders(blocks)


# ---- the read set -------------------------------------------------------------------------------------------------------------------------
def pairs_of(w, h):
    return ((h + 3) // 4) * (((w + 3) // 4 + 1) // 2)


def vlc_reach(scup, w, h):
    return min(scup - 2, (46 * pairs_of(w, h) + 7) // 8 + 8)


def read_set(data, w, h):
    """(a_end, b_start) of a block with a valid SCUP field: A = [0, a_end), B = [b_start, n); a_end == n when A reaches B"""
    n, scup = len(data), hc.scup_of(data)
    assert n >= 2 and 2 <= scup <= n
    a_end, b_start = min(n, n - scup + 4), n - 2 - vlc_reach(scup, w, h)
    return (n, b_start) if a_end >= b_start else (a_end, b_start)


POSITION_CLASSES = ("magsgn_last", "mel0", "mel1", "mel2", "mel3", "b_first", "vlc_deepest", "len-3", "trailer0", "trailer1")
INTERIOR_CLASSES = ("interior_first", "interior_last")


def positions(data, w, h):
    """{class: byte position, or None where the block has no such byte}"""
    n, scup = len(data), hc.scup_of(data)
    a_end, b_start = read_set(data, w, h)
    inside = a_end < b_start
    pos = dict(magsgn_last=n - scup - 1 if n > scup else None, b_first=b_start, trailer0=n - 2, trailer1=n - 1)
    pos["len-3"] = n - 3 if n >= 3 else None
    for i in range(4):
        pos["mel%d" % i] = n - scup + i if n - scup + i < n else None
    pos["interior_first"] = a_end if inside else None
    pos["interior_last"] = b_start - 1 if inside else None
    return pos


def flip(data, pos):
    b = bytearray(data)
    b[pos] ^= 0x55
    return bytes(b)


def decode(data, w, h):
    return _orc.ht_decode(np.frombuffer(bytes(data), np.uint8), w, h)


class Edge(NamedTuple):
    """a list's bodies: the leader and all followers carry `base`, except that `who` ("follower": the list's last one, "leader", "none") carries `other`"""
    label: str
    base: bytes
    other: Optional[bytes]
    who: str
    cls: str = ""            # the position class flipped ("" when the case is about a length or a form)


EDGE_SHAPE = (16, 16)        # the blocks these cases are made for: 8 pairs, a VLC reach of at most 54 bytes


def _mel_refused(rng, k, n=40, mag=b""):
    """test_gpu_ht_front.py's refusal recipe "mel": the MEL reader starts at the suffix's first byte and, where the MagSgn length is a multiple of four
    (0 there), looks at four bytes; 0xFF as byte k of an n-byte suffix and a byte above 0x8F behind it -- 0xD5 here, so that the flip (^ 0x55) of either
    byte lifts the refusal.  n = 40: A reaches B and the whole block is in the read set; n = 70: bytes 4 .. 13 of the suffix are interior"""
    w, h = EDGE_SHAPE
    assert len(mag) % 4 == 0 and 0xFF not in mag
    for _ in range(400):
        suf = bytearray(hc._rand_no_ff(rng, n))
        for i in range(6):
            if suf[i] > 0x8F:
                suf[i] &= 0x7F
        suf[k], suf[k + 1] = 0xFF, 0xD5
        s = hc.splice(mag, hc.with_scup(bytes(suf), n))
        m = len(mag)
        if not decode(s, w, h).any() and decode(flip(s, m + k), w, h).any() and decode(flip(s, m + k + 1), w, h).any():
            return s
    raise AssertionError("no refused suffix whose flips decode to something")


def _nonzero_suffix(rng, n):
    w, h = EDGE_SHAPE
    for _ in range(400):
        s = hc.random_suffix(rng, n)
        if decode(s, w, h).any():
            return s
    raise AssertionError("no suffix of %d bytes that decodes to something" % n)


@functools.lru_cache(None)
def edge_cases():
    """every case once with the differing body in a follower and once in the leader"""
    w, h = EDGE_SHAPE
    rng = np.random.default_rng(0xF011)
    enc = hc.encoder_output(rng, w, h, 300)
    assert len(enc) > hc.scup_of(enc) and positions(enc, w, h)["interior_first"] is not None
    _, enc_suffix = hc.split(enc)
    one = []                                                          # (label, base, other or None, class)
    # one byte flipped at each edge of the read set, and just outside it, of a block the encoder wrote
    for cls, pos in positions(enc, w, h).items():
        if not cls.startswith("mel"):
            one.append(("encoder block, %s" % cls, enc, flip(enc, pos), cls))
    for k in (0, 2):                                                  # the four MEL-start bytes: refused streams that one flip makes decodable
        s = _mel_refused(rng, k)
        for i in (k, k + 1):
            one.append(("refused MEL start, byte %d" % i, s, flip(s, i), "mel%d" % i))
    # the same in blocks that HAVE an interior (a suffix of 70 bytes: SCUP above 4 + 54 + 2), behind an empty and behind a four-byte MagSgn segment: a
    # compare that ended A at the MagSgn segment, without the four bytes init_mel_ok looks at, would call these followers verified
    for mag in (b"", hc._rand_no_ff(rng, 4)):
        for k in (0, 2):
            s = _mel_refused(rng, k, 70, mag)
            a_end, b_start = read_set(s, w, h)
            assert a_end == len(mag) + 4 and b_start == len(s) - 56 and a_end < b_start
            for i in (k, k + 1):
                one.append(("refused MEL start with an interior, MagSgn %d, byte %d" % (len(mag), i), s, flip(s, len(mag) + i), "mel%d" % i))
            one.append(("refused MEL start with an interior, MagSgn %d, first interior byte" % len(mag), s, flip(s, a_end), "interior_first"))
    # the deepest VLC byte the encoder's block really uses (B's first byte is below it: 8 pairs cannot take 46 bits each)
    deep = next(p for p in range(positions(enc, w, h)["b_first"], len(enc) - 2) if not np.array_equal(decode(enc, w, h), decode(flip(enc, p), w, h)))
    one.append(("encoder block, deepest VLC byte used (%d, B starts at %d)" % (deep, positions(enc, w, h)["b_first"]), enc, flip(enc, deep), "vlc_deepest"))
    # block lengths 4 .. 8: the whole block is suffix (SCUP == len), and SCUP == 2 (everything but the trailer is MagSgn)
    for n in range(4, 9):
        for scup in (n, 2):
            s = hc.with_scup(hc._rand_no_ff(rng, n), scup)
            one.append(("len %d, SCUP %d" % (n, scup), s, None, ""))
            one.append(("len %d, SCUP %d, byte 0" % (n, scup), s, flip(s, 0), ""))
    short = _nonzero_suffix(rng, 8)                                    # B starts at the suffix's first byte and every VLC byte is walked
    one.append(("suffix of 8 bytes, b_first", short, flip(short, positions(short, w, h)["b_first"]), "b_first"))
    # an empty MagSgn segment in front of the encoder's suffix
    one.append(("empty MagSgn", enc_suffix, None, ""))
    one.append(("empty MagSgn, len-3", enc_suffix, flip(enc_suffix, len(enc_suffix) - 3), "len-3"))
    # MagSgn lengths around the first compare batch (1 KB) and beyond the second
    for n in (1, 3, 1023, 1024, 1025, 2100):
        s = hc.splice(hc._rand(rng, n), enc_suffix)
        one.append(("MagSgn %d bytes" % n, s, None, ""))
        one.append(("MagSgn %d bytes, its last" % n, s, flip(s, n - 1), "magsgn_last"))
        if n >= 1023:
            one.append(("MagSgn %d bytes, byte 1020" % n, s, flip(s, 1020), ""))
    # suffixes short enough that A and B touch (SCUP 60: 4 + 54 + 2), overlap by one byte (59), leave a one-byte interior (61)
    for scup, what in ((60, "touch"), (59, "overlap"), (61, "one-byte interior")):
        s = hc.splice(hc._rand(rng, 10), _nonzero_suffix(rng, scup))
        a_end, b_start = read_set(s, w, h)
        assert (b_start - (len(s) - scup + 4)) == {"touch": 0, "overlap": -1, "one-byte interior": 1}[what]
        one.append(("A and B %s" % what, s, None, ""))
        for p in sorted({len(s) - scup + 3, len(s) - scup + 4, len(s) - 2 - 54}):
            inside = a_end <= p < b_start
            one.append(("A and B %s, byte %d" % (what, p), s, flip(s, p), "interior_first" if inside else ""))
    out = []
    for label, base, other, cls in one:
        if other is None:
            out.append(Edge(label, base, None, "none", cls))
        else:
            out.append(Edge(label + " (follower)", base, other, "follower", cls))
            out.append(Edge(label + " (leader)", base, other, "leader", cls))
    return out


# ---- a MagSgn segment that is READ past the first kilobyte -----------------------------------------------------------------------------------------
# A 16 x 16 block has 64 coded samples and reads about 60 MagSgn bytes whatever the segment's length; the reference's decoder reads 40 bytes of a
# 64 x 64 block its own encoder wrote with 24-bit samples (2.9 KB of MagSgn).  So a flip at byte 1 024 of those is inside the read set and changes
# nothing: the compare's batches behind the first would go untested.  tests/golden/ht_follow_suffix_64x64_reads_1493.bin is a 1 000-byte suffix for a
# 64 x 64 block (1 024 coded samples, the most the parallel path takes) whose code words make the decoder read 1 493 bytes of MagSgn: found with the C
# oracle alone, row by row, every byte of a row's VLC bytes tried at all 256 values for the farthest MagSgn byte that still changes the output (six
# passes per row; 350 s, so the result is kept, not the search).  Every byte below 1 493 decides a result here -- the second 1 KB batch and the piece
# pulled back to the segment's end.  Past 2 KB no stream was found (that search reached 90 bytes per row of 64 samples; 2 KB needs 128): the segment
# below is 2 500 bytes long so that the third batch runs, but its flips behind byte 1 493 are checked for equality with the oracle only.
# The plan: one list, a leader and three followers.
BIG_SHAPE = (64, 64)
BIG_PLAN = dict(W=128, H=128, nres=2, cb=(64, 64))
BIG_READS = 1493
BIG_CLASSES = ("batch1_last", "batch2_first", "batch2", "read_last", "cut_last")     # every one of them changes the oracle's output


@functools.lru_cache(None)
def big_edge_cases():
    import os
    w, h = BIG_SHAPE
    rng = np.random.default_rng(0xF021)
    suffix = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ht_follow_suffix_64x64_reads_1493.bin"), "rb").read()
    assert len(suffix) == 1000 and hc.scup_of(suffix) == 1000
    mag = hc._rand_no_ff(rng, 2500)
    enc = hc.splice(mag, suffix)
    a_end, b_start = read_set(enc, w, h)
    assert a_end == len(mag) + 4 and a_end < b_start
    one = [("64 x 64, MagSgn 2500 bytes", enc, None, "")]
    for cls, p in (("batch1_last", 1023), ("batch2_first", 1024), ("batch2", 1030), ("batch2", 1400), ("read_last", BIG_READS - 1), ("", BIG_READS + 8),
                   ("", 2047), ("", 2048), ("", 2060), ("", len(mag) - 1), ("interior_first", a_end), ("interior_last", b_start - 1)):
        one.append(("64 x 64, MagSgn 2500 bytes, byte %d" % p, enc, flip(enc, p), cls))
    for n in (1023, 1024, 1025, 1300):                               # the same block with its MagSgn segment cut to n bytes: the last of them is read
        s = hc.splice(mag[:n], suffix)
        one.append(("64 x 64, MagSgn cut to %d bytes" % n, s, None, ""))
        one.append(("64 x 64, MagSgn cut to %d bytes, its last" % n, s, flip(s, n - 1), "cut_last"))
    out = []
    for label, base, other, cls in one:
        if other is None:
            out.append(Edge(label, base, None, "none", cls))
        else:
            out.append(Edge(label + " (follower)", base, other, "follower", cls))
            out.append(Edge(label + " (leader)", base, other, "leader", cls))
    return out


@functools.lru_cache(None)
def big_u_suffixes(w, h):
    """{"=32": suffix, ">=33": suffix} on a w x h block (ht_stream_cases' seeded search, one per bucket)"""
    found, _ = hc.find_suffixes(w, h, 1, 3000)
    assert found["=32"] and found[">=33"], "no suffix with u of 32 and above on %dx%d" % (w, h)
    return {b: found[b][0] for b in ("=32", ">=33")}
