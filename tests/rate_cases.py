"""The yardstick of the rate-limited MQ encode (j2k_plan_encode_blocks_planes, j2k_plan_rate_allocate), importable without a GPU:
tests/test_rate_cases.py checks it on the CPU, tests/test_gpu_rate_encode.py holds the device against it bit for bit.

Block j has nb = numBPS (<= 31) bit planes; p = 0 ... nb is the number of planes kept, k = nb - p its floor.

  R[p]  uint32, bytes of the block's codeword that decode the first p planes; R[0] = 0, R[nb] = len(data), non-decreasing.  How the encoder
        derives it is its own business; what it must satisfy is the PREFIX PROPERTY, prefix_ok() below.
  D[p]  uint64, sum (|v| - |coarse(v, k)|)^2 in wrapping arithmetic, coarse = coarse_cases.coarse; D[nb] = 0.
  w     float64 weight of the block's (component, resolution, band), finite and >= 0.

Hull: the upper-left convex hull of (R[p], D[p]) from p = 0, built incrementally: a point that does not lower D is never a hull point; a
point that lowers D for no more bytes is steeper than anything (slope +inf) and so replaces its predecessor (the start itself, if it gets
that far); otherwise the slope from hull point a to p is (w * float64(D[a] - D[p])) / float64(R[p] - R[a]) -- one multiply, one divide -- and
points are popped while the new slope is not smaller than the incoming slope of the last one.  Slopes along a hull fall strictly.

Choice: p(lam) = the last hull point whose incoming slope is >= lam, or the start.  If the full lengths fit the budget nothing is cut.
Otherwise lam* is the non-negative float64 with the smallest bit pattern whose choices fit, found by 64 bisection steps over the bit patterns
0 ... 2^63 - 1 (those above +inf are NaNs: no slope is >= a NaN, every block is at its start, 0 bytes).  The budget counts code-block body
bytes only."""
import struct

import numpy as np

from coarse_cases import coarse

STRIDE = 32            # table entries per block on the device
MASK64 = (1 << 64) - 1


# ---- tables -------------------------------------------------------------------------------------------------------------------------------
def distortion(v, nb):
    """D[0 ... nb] as Python ints (mod 2^64) of an int32 block v with numBPS = nb"""
    a = np.abs(np.asarray(v).astype(np.int64))
    out = []
    for p in range(nb + 1):
        d = (a - np.abs(coarse(v, nb - p).astype(np.int64))).astype(np.uint64)          # negative differences wrap; their squares do not care
        with np.errstate(over="ignore"):
            out.append(int((d * d).sum(dtype=np.uint64)))
    return out


def distortion_direct(v, nb):
    """the same by a plain loop over the samples (tests/test_rate_cases.py)"""
    out = []
    for p in range(nb + 1):
        k, s = nb - p, 0
        for x in np.asarray(v).reshape(-1).tolist():
            m = abs(x)
            hi = m >> k << k
            rec = hi | (1 << (k - 1)) if (hi and k >= 1) else hi
            s += (m - rec) ** 2
        out.append(s & MASK64)
    return out


def prefix_ok(oracle, data, R_p, nb, band, v, p):
    """the prefix property of R[p]: the decode of data[:R_p] has the first p planes right"""
    h, w = v.shape
    k = nb - p
    g = oracle.t1_decode(np.ascontiguousarray(data[:R_p], dtype=np.uint8), nb, band, w, h).reshape(h, w).astype(np.int64)
    a, b = np.abs(g) >> k, np.abs(v.astype(np.int64)) >> k
    return bool(np.array_equal(a, b) and np.array_equal(np.sign(g)[a != 0], np.sign(v)[a != 0]))


def floors_from_header(zero_bit_planes, num_passes, mb=31):
    """(floor, numbps) a decoder reads from a closed-loop packet header: a block of nb planes cut to p of them is written with zero_bit_planes
    = mb - nb and num_passes = 3 p - 2 (0 for p = 0)"""
    p = (num_passes + 2) // 3
    floor = max(mb - zero_bit_planes - p, 0)
    return floor, p + floor


def passes_of(p):
    return 3 * p - 2 if p > 0 else 0


# ---- hull and choice ----------------------------------------------------------------------------------------------------------------------
def hull(R, D, nb, w):
    """([plane of every hull point], [incoming slope of each; None for the start])"""
    w = float(w)
    pts, sl = [0], [None]
    for p in range(1, nb + 1):
        while True:
            a = pts[-1]
            if not D[p] < D[a]:
                break
            free = R[p] <= R[a]
            s = float("inf") if free else (w * float(D[a] - D[p])) / float(R[p] - R[a])
            if len(pts) > 1:
                if s >= sl[-1]:
                    pts.pop(); sl.pop()
                    continue
                pts.append(p); sl.append(s)
            elif free:
                pts[0] = p
            else:
                pts.append(p); sl.append(s)
            break
    return pts, sl


def pick(h, lam):
    pts, sl = h
    i = 0
    while i + 1 < len(pts) and sl[i + 1] >= lam:
        i += 1
    return pts[i]


def bits_to_float(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def allocate(Rs, Ds, nbs, ws, budget):
    """tables of every block -> ([planes kept of every block], body bytes of the choice)"""
    n = len(Rs)
    total = sum(int(Rs[j][nbs[j]]) for j in range(n))
    if total <= budget:
        return [int(nb) for nb in nbs], total
    hulls = [hull([int(x) for x in Rs[j]], [int(x) for x in Ds[j]], int(nbs[j]), ws[j]) for j in range(n)]

    def choice(bits):
        lam = bits_to_float(bits)
        ps = [pick(h, lam) for h in hulls]
        return ps, sum(int(Rs[j][ps[j]]) for j in range(n))

    lo, hi = 0, (1 << 63) - 1
    for _ in range(64):
        mid = lo + (hi - lo) // 2
        if lo < hi:
            if choice(mid)[1] <= budget:
                hi = mid
            else:
                lo = mid + 1
    return choice(hi)


def weighted_distortion(Ds, ws, ps):
    return sum(float(ws[j]) * float(Ds[j][ps[j]]) for j in range(len(ps)))


# ---- weights ------------------------------------------------------------------------------------------------------------------------------
def _synth_response(lossless, high):
    """one level of the 1-D inverse lifting without its integer rounding (pyref.inverse53 / inverse97), impulse in the middle of a long line"""
    n = 64
    d = [0.0] * n
    d[33 if high else 32] = 1.0                                     # interleaved: even = low, odd = high

    def lift(first, c):
        for i in range(1 if first else 2, n - 1, 2):
            d[i] -= c * (d[i - 1] + d[i + 1])
    if lossless:
        lift(0, 0.25); lift(1, -0.5)
    else:
        for i in range(n):
            d[i] *= 0.812893066115961 if i & 1 else 1.230174104914001
        lift(0, 0.443506852043971); lift(1, 0.882911075530934); lift(0, -0.052980118572961); lift(1, -1.586134342059924)
    nz = [i for i, v in enumerate(d) if v != 0.0]
    return np.array(d[nz[0]:nz[-1] + 1])


def default_weights(ncomp, nres, lossless, mallat=True):
    """float64 [ncomp, nres, 4]: the synthesis energy gain of every band of a Mallat plan (1 on other plans), component weight 1"""
    out = np.ones((ncomp, nres, 4))
    if not mallat:
        return out
    L = nres - 1
    g0, g1 = _synth_response(lossless, False), _synth_response(lossless, True)
    EL, EH = [1.0] * (L + 1), [1.0] * (L + 1)
    fl, fh = g0, g1
    for d in range(1, L + 1):
        if d > 1:
            up = lambda f: np.convolve(np.stack([f, np.zeros_like(f)], 1).reshape(-1)[:-1], g0)
            fl, fh = up(fl), up(fh)
        EL[d], EH[d] = float((fl ** 2).sum()), float((fh ** 2).sum())
    for r in range(nres):
        d = L if r == 0 else L - r + 1
        out[:, r, 0] = EL[d] * EL[d]
        out[:, r, 1] = out[:, r, 2] = EH[d] * EL[d]
        out[:, r, 3] = EH[d] * EH[d]
    return out


def band_rect(w, h, levels, res, band):
    """(x0, y0, bw, bh) of band `band` (0 LL, 1 HL, 2 LH, 3 HH) of resolution `res` in a Mallat plane of `levels` levels"""
    wl, hl = w, h
    for _ in range(levels if res == 0 else levels - res):
        wl, hl = (wl + 1) // 2, (hl + 1) // 2
    if res == 0:
        return 0, 0, wl, hl
    wn, hn = (wl + 1) // 2, (hl + 1) // 2
    return {1: (wn, 0, wl - wn, hn), 2: (0, hn, wn, hl - hn), 3: (wn, hn, wl - wn, hl - hn)}[band]


def impulse_energy(oracle, w, h, levels, res, band, lossless, amp=1 << 24):
    """energy gain of band (res, band): an impulse in the middle of the band through the Mallat inverse (mallat_cases.inverse_tile's level loop),
    sum of squares of the result over amp^2"""
    import mallat_cases as mc
    x0, y0, bw, bh = band_rect(w, h, levels, res, band)
    p = np.zeros((h, w), np.int32 if lossless else np.float64)
    p[y0 + bh // 2, x0 + bw // 2] = amp
    d = mc.dims(w, h, levels)
    for l in range(levels - 1, -1, -1):
        wl, hl = d[l]
        rect = np.ascontiguousarray(p[:hl, :wl])
        p[:hl, :wl] = (oracle.inv53_2d if lossless else oracle.inv97_2d)(rect, wl, hl)
    return float((p.astype(np.float64) ** 2).sum()) / float(amp) ** 2
