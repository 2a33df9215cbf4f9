"""HT block decode, byte-identical blocks once (context option ht_dec_dedup): the definition of the plan's candidate table, restated in Python,
and the small geometries the tests use.

The reference addresses every block window from the top left of its tile-component (encoder.go:763-795) and sizes the three bands of a
resolution alike, so block (cbx, cby) of every band and resolution that has one reads the same window.  The HT coder ignores the band: such
jobs carry the same bytes.  The plan names candidates from static facts alone; the decoder compares the bytes in every call.

  leader(j) = the lowest job with the same (tile-component, x0, y0, w, h)
  j FOLLOWS its leader L != j iff   w == w_L and h == h_L                                  (same key: always)
                                    and w in (8, 16, 32, 64)                                (the lean kernel's widths)
                                    and ceil(h / 4) * w <= 1024 and ceil(h / 4) * ceil(ceil(w / 4) / 2) <= 128    (the parallel path)
                                    and dec_off(j) % 4 == 0 and dec_off(L) % 4 == 0         (16-byte aligned decoded blocks)
                                    and L has fewer than 7 followers so far (jobs in ascending order)
  otherwise j is its own leader (a job beyond the cap is NOT chained to another leader).
"""
import collections

MAX_FOLLOWERS = 7
FAST_MAX_SAMPLES, WALK_MAX_PAIRS = 1024, 128
LEAN_WIDTHS = (8, 16, 32, 64)

# single-tile, one-component plans (FramePlan(W, H, 1, num_resolutions=nres, cb=cb, coder=CODER_HT)); at most about 128 x 128 samples
GEOMETRIES = {
    "136x136_cb16": dict(W=136, H=136, nres=5, cb=(16, 16)),     # window (0, 0): 9 jobs -- a list at the cap and one job beyond it; 118 jobs: two walk workgroups
    "132x132_cb32": dict(W=132, H=132, nres=4, cb=(32, 32)),     # narrow-block stores, 32 wide
    "264x72_cb64x16": dict(W=264, H=72, nres=4, cb=(64, 16)),    # the 64-wide row stores (64 x 64 blocks twice over need a 256 x 256 frame)
}


def block_list(W, H, nres, cb, ncomp=1):
    """the jobs of a one-tile open-loop plan in job order (encoder.go:616-673): dicts plane, res, band, x0, y0, w, h"""
    out = []
    for c in range(ncomp):
        for r in range(nres):
            scale = 1 << (nres - 1 - r)
            bw, bh = -(-W // scale), -(-H // scale)
            if r > 0:
                bw, bh = (bw + 1) // 2, (bh + 1) // 2
            for band in ([0] if r == 0 else [1, 2, 3]):
                for y0 in range(0, bh, cb[1]):
                    for x0 in range(0, bw, cb[0]):
                        out.append(dict(plane=c, res=r, band=band, x0=x0, y0=y0, w=min(cb[0], bw - x0), h=min(cb[1], bh - y0)))
    return out


def decoded_offsets(blocks):
    offs, pos = [], 0
    for b in blocks:
        offs.append(pos)
        pos += (b["w"] * b["h"] + 3) & ~3
    return offs


def on_parallel_path(w, h):
    R, P = (h + 3) // 4, ((w + 3) // 4 + 1) // 2
    return R * w <= FAST_MAX_SAMPLES and R * P <= WALK_MAX_PAIRS


Rule = collections.namedtuple("Rule", "leaders followers refused")     # leaders[j]; {leader: [followers]}; {j: why} for candidates that stay alone


def leaders(blocks, dec_offs=None):
    dec_offs = decoded_offsets(blocks) if dec_offs is None else dec_offs
    first, lead, fol, refused = {}, [], collections.defaultdict(list), {}
    for j, b in enumerate(blocks):
        key = (b["plane"], b["x0"], b["y0"], b["w"], b["h"])
        L = first.setdefault(key, j)
        lead.append(j)
        if L == j:
            continue
        if b["w"] not in LEAN_WIDTHS:
            refused[j] = "width"
        elif not on_parallel_path(b["w"], b["h"]):
            refused[j] = "serial"
        elif int(dec_offs[j]) % 4 or int(dec_offs[L]) % 4:
            refused[j] = "alignment"
        elif len(fol[L]) >= MAX_FOLLOWERS:
            refused[j] = "cap"
        else:
            fol[L].append(j)
            lead[j] = L
    return Rule(lead, {k: v for k, v in fol.items() if v}, refused)
