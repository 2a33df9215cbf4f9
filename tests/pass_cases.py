"""The yardstick of pass-level rate control (the *_passes / *_pfloors calls: MQ blocks cut at coding-pass ends, not only at bit-plane ends),
importable without a GPU: tests/test_pass_cases.py checks it on the CPU, tests/test_gpu_pass_cuts.py holds the device against it bit for bit.

Pass index.  A block of nb planes (nb = min(numBPS, 31)) has the cut points q = 0 ... 3 nb - 2; q = 0 keeps nothing; q >= 1 keeps
p = (q + 2) // 3 whole planes from the top and s = (q + 2) % 3 further passes of plane b = nb - p - 1 (s = 1: its SigProp pass, s = 2: SigProp
and MagRef).  This is the packet header's pass count (rate_cases.passes_of(p) = 3 p - 2 is s = 0); the top plane has no cut inside it, its
SigProp and MagRef passes are empty.

sp mask.  One bit per sample: "turned significant in a SigProp pass (not in Cleanup)".  Per plane b from the top: the samples with
|v| >= 2^(b+1) are significant, the candidates are those whose top bit is b; in raster order (rows, then columns) a candidate with a
significant 8-neighbour IN THE STATE AT THAT MOMENT (the samples turned earlier in this pass included) turns significant with sp = 1; the
other candidates turn significant in Cleanup.

coarse_pass(v, nb, q, sp).  The sample's floor k is nb - p for s = 0; for s > 0 it is b where the sample's pass of plane b has run (top bit
== b and sp set; or top bit > b and s = 2), else b + 1.  The value is coarse_cases.coarse(v, k) sample by sample.

Tables, stride 96 per block:
  R[q]  uint32, bytes of the unchanged codeword whose decode has every pass up to q right; R[0] = 0, R[3 nb - 2] = len, non-decreasing,
        entries above 3 nb - 2 repeat len.
  D[q]  uint64 (wrapping), sum (|v| - |coarse_pass(v, nb, q, sp)|)^2; 0 at and above 3 nb - 2.
They tie to the plane tables: R[3 p - 2] == rate32[p], D[3 p - 2] == dist32[p].

Allocation: rate_cases.hull / allocate and quality_cases.allocate_quality unchanged, with the point count max(3 nb - 2, 0) in nb's place.

Reader: from a block header p = (np + 2) // 3, s = (np + 2) % 3, floor = max(31 - zbp - p, 0), numbps = p + floor, and the passes left
undecoded pfloor = 3 floor - s if floor > 0 else 0.  A block decodes down to f = max(3 skip_planes, pfloor): whole planes down to
ceil(f / 3), then the first 3 ceil(f / 3) - f passes of the next plane."""
import numpy as np

from coarse_cases import coarse

STRIDE = 96
MASK64 = (1 << 64) - 1


def points(nb):
    """the last pass index of a block of nb planes (the point count the allocation runs on)"""
    return max(3 * min(int(nb), 31) - 2, 0)


def split(q):
    """q >= 1 -> (p, s)"""
    return (q + 2) // 3, (q + 2) % 3


def top_bits(v):
    """int array: the index of the top set bit of |v|, -1 for 0"""
    a = np.abs(np.asarray(v).astype(np.int64))
    t = np.full(a.shape, -1, np.int64)
    for b in range(32):
        t[a >> b != 0] = b
    return t


def sp_mask(v, nb):
    """bool [h, w] by the row-mask model: per row, a candidate turns in SigProp if a neighbour in the rows above / below (the row above as
    updated by this pass) or its left-hand neighbour (as updated) or its right-hand neighbour (old state) is significant"""
    v = np.asarray(v)
    h, w = v.shape
    t = top_bits(v)
    sp = np.zeros((h, w), bool)
    for b in range(nb - 1, -1, -1):
        sig = t > b                                           # before this plane
        cand = t == b
        if not sig.any():
            continue                                          # the top plane: SigProp has nothing to go on
        cur = sig.copy()
        for y in range(h):
            up = cur[y - 1] if y > 0 else np.zeros(w, bool)
            dn = sig[y + 1] if y + 1 < h else np.zeros(w, bool)
            vert = up | dn
            around = vert.copy()
            around[1:] |= vert[:-1]
            around[:-1] |= vert[1:]
            around[:-1] |= sig[y, 1:]                         # E: not yet visited
            row = cur[y]
            for x in range(w):
                if cand[y, x] and (around[x] or (x > 0 and row[x - 1])):
                    row[x] = True
                    sp[y, x] = True
    return sp


def sp_mask_direct(v, nb):
    """the same by a plain loop over the samples and their eight neighbours"""
    v = np.asarray(v)
    h, w = v.shape
    a = np.abs(v.astype(np.int64))
    sp = np.zeros((h, w), bool)
    for b in range(nb - 1, -1, -1):
        sig = [[bool(a[y, x] >> (b + 1)) for x in range(w)] for y in range(h)]
        for y in range(h):
            for x in range(w):
                if sig[y][x] or not (a[y, x] >> b) & 1:
                    continue
                nbr = False
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = y + dy, x + dx
                        if (dy or dx) and 0 <= yy < h and 0 <= xx < w and sig[yy][xx]:
                            nbr = True
                if nbr:
                    sig[y][x] = True
                    sp[y, x] = True
    return sp


def sp_words(sp):
    """bool [h, w] (w, h <= 64) -> uint64 [64]: row y's mask, bit x; rows >= h zero (the device's spmask layout)"""
    h, w = sp.shape
    out = np.zeros(64, np.uint64)
    for y in range(h):
        out[y] = np.uint64(sum(1 << x for x in range(w) if sp[y, x]))
    return out


def floors_pass(v, nb, q, sp):
    """int array: every sample's floor k at cut q"""
    v = np.asarray(v)
    if q == 0:
        return np.full(v.shape, nb, np.int64)
    p, s = split(q)
    if s == 0:
        return np.full(v.shape, nb - p, np.int64)
    b = nb - p - 1
    t = top_bits(v)
    run = (t == b) & np.asarray(sp, bool)
    if s == 2:
        run |= t > b
    return np.where(run, b, b + 1).astype(np.int64)


def coarse_pass(v, nb, q, sp):
    """int32 array: what a decoder that stops after pass q leaves of v"""
    v = np.asarray(v)
    k = floors_pass(v, nb, q, sp)
    out = np.zeros(v.shape, np.int32)
    for kk in np.unique(k).tolist():
        out = np.where(k == kk, coarse(v, int(kk)), out)
    return out.astype(np.int32)


def distortion_passes(v, nb, sp):
    """D[0 ... 3 nb - 2] as Python ints (mod 2^64); [0] for nb = 0"""
    a = np.abs(np.asarray(v).astype(np.int64))
    out = []
    for q in range(points(nb) + 1):
        d = (a - np.abs(coarse_pass(v, nb, q, sp).astype(np.int64))).astype(np.uint64)
        with np.errstate(over="ignore"):
            out.append(int((d * d).sum(dtype=np.uint64)))
    return out


def prefix_ok_pass(oracle, data, R_q, nb, band, v, q, sp):
    """the prefix property of R[q]: the decode of data[:R_q] has every pass up to q right -- it agrees with v in |.| >> k, and in sign where
    that is non-zero, with the per-sample k of coarse_pass"""
    h, w = v.shape
    k = floors_pass(v, nb, q, sp)
    g = oracle.t1_decode(np.ascontiguousarray(data[:R_q], dtype=np.uint8), nb, band, w, h).reshape(h, w).astype(np.int64)
    a, b = np.abs(g) >> k, np.abs(v.astype(np.int64)) >> k
    return bool(np.array_equal(a, b) and np.array_equal(np.sign(g)[a != 0], np.sign(v)[a != 0]))


def check_tables(R, D, nb, length):
    """the definition's invariants of one block's tables (arrays of STRIDE entries)"""
    last = points(nb)
    R = [int(x) for x in R]
    D = [int(x) for x in D]
    assert len(R) == STRIDE and len(D) == STRIDE
    assert R[0] == 0 and R[last] == length
    assert all(R[i] <= R[i + 1] for i in range(last))
    assert all(x == length for x in R[last:])
    assert not any(D[last:])


# ---- headers --------------------------------------------------------------------------------------------------------------------------------
def pfloor_from_header(zero_bit_planes, num_passes, mb=31):
    """(pfloor, numbps) a pass-aware reader takes from a closed-loop packet header"""
    p, s = (num_passes + 2) // 3, (num_passes + 2) % 3
    floor = max(mb - zero_bit_planes - p, 0)
    return (3 * floor - s if floor > 0 else 0), p + floor


def pfloor_of(nb, q):
    """the passes left undecoded of a block of nb planes cut at q"""
    return points(nb) - q


def decode_plan(f):
    """f passes left undecoded -> (whole planes run down to this floor, passes of the next plane)"""
    k = (f + 2) // 3
    return k, 3 * k - f


def q_of(nb, f):
    """the cut a decoder stopping f passes short of a block of nb planes stands at (never below 0)"""
    return max(points(nb) - f, 0)


def allocate_quality(Rs, Ds, pts, ws, T):
    """quality_cases.allocate_quality on pass tables: its hull arrays are rate_cases.STRIDE wide, a pass hull can have up to 92 points"""
    import quality_cases as qc
    import rate_cases as rc
    old = rc.STRIDE
    rc.STRIDE = STRIDE
    try:
        return qc.allocate_quality(Rs, Ds, pts, ws, T)
    finally:
        rc.STRIDE = old


# ---- packets --------------------------------------------------------------------------------------------------------------------------------
def compose_kept_passes(t2ref, tiles, datas, nbs, Rs, qs, sop, eph, tile_first=0):
    """layer_cases.compose_kept with the two fields of a pass cut: body data[:R[q]], num_passes = q; zero_bit_planes = 31 - nb stays, and a block
    without bytes is in no layer.  tiles: per tile its packets, a packet = the list of its block numbers"""
    import layer_cases as lc
    out = bytearray()
    for t, packets in enumerate(tiles):
        enc = t2ref.PacketEncoder(len_bits=5)
        for pk in packets:
            blocks = []
            for j in pk:
                ln = int(Rs[j][qs[j]]) if qs[j] > 0 else 0
                blocks.append(t2ref.CodeBlock(bytes(bytearray(datas[j][:ln])), 1 if ln == 0 else 0, max(31 - int(nbs[j]), 0), int(qs[j]) if ln else 0))
            enc.encode_packet(t2ref.Precinct([blocks]), 0, sop, eph)
        out += lc.tile_head(tile_first + t, 14 + len(enc.out)) + bytes(enc.out)
    return bytes(out)


# ---- blocks ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (5, 7), (8, 8), (16, 16), (33, 64), (64, 3), (64, 64))      # (w, h)
CONTENTS = ("noise", "sparse", "zero", "deep", "gradient")


def block(w, h, content, seed=0):
    """int32 [h, w]"""
    rng = np.random.default_rng(9000 + 131 * w + 17 * h + seed)
    if content == "noise":
        return rng.integers(-255, 256, (h, w)).astype(np.int32)
    if content == "sparse":                                                   # about 1 % non-zero (at least one sample): most passes are empty
        x = rng.integers(-255, 256, (h, w))
        x[rng.random((h, w)) >= 0.01] = 0
        x.reshape(-1)[int(rng.integers(0, w * h))] = 200
        return x.astype(np.int32)
    if content == "zero":
        return np.zeros((h, w), np.int32)
    if content == "deep":                                                     # 31 planes
        x = rng.integers(-3, 4, (h, w)).astype(np.int64)
        x.reshape(-1)[(w * h) // 2] = (1 << 31) - 1
        return x.astype(np.int32)
    if content == "gradient":
        yy, xx = np.mgrid[0:h, 0:w]
        return (3 * xx - 2 * yy + (xx * yy) // 7 - 40).astype(np.int32)
    raise ValueError(content)


def numbps_of(v):
    m = int(np.abs(np.asarray(v).astype(np.int64)).max()) if np.asarray(v).size else 0
    return m.bit_length()
