"""The yardstick of the quality-targeted MQ encode (min_psnr= / max_distortion= / layer_psnr= / layer_distortion= of encode_frame_pixels and
encode_pixels_host, rate_allocate_quality, the j2k_*_quality calls), importable without a GPU: tests/test_quality_cases.py checks it on the CPU,
tests/test_gpu_quality_encode.py holds the device against it bit for bit.  It is the dual of tests/rate_cases.py and builds on its hull, pick
and bits_to_float: the tables R, D, the weights w, the hulls and the rule "p(lam) = the last hull point whose incoming slope is >= lam" are
unchanged; the search runs on the distortion sum instead of the byte sum.

Weighted distortion of a choice p, in a FIXED order (the terms are float64, so the order is part of the definition).  Block j's term is
t_j = w_j * float64(D_j[p_j]), one multiply.  S(p) is the sum the device's one workgroup of 1024 threads takes:

  1. thread i adds t_i, t_(i + 1024), ... in that order, starting from 0.0;
  2. within each group of 64 threads six butterfly steps v = v + v[lane ^ o], o = 32, 16, ..., 1 (addition commutes, so afterwards every lane
     of a group holds the same value);
  3. the 16 group values are added in order, starting from 0.0.

Rounded addition is monotone in each argument and every t_j falls along its hull, so S does not rise as lam falls: the bisection below is
well defined.

Search: allocate_quality(Rs, Ds, nbs, ws, T) for a finite T >= 0 returns the choice p(lam*), lam* the float64 with the LARGEST bit pattern in
0 ... 2^63 - 1 whose choice has S <= T (the patterns above +inf are NaNs: no slope is >= a NaN, every block is at its start point).  64 steps:
mid = lo + (hi - lo + 1) / 2, lo = mid if S(mid) <= T else hi = mid - 1.  Pattern 0 always fits: lam = +0.0 takes every hull to its last
point, where D = D[nb] = 0 -- there is no infeasible target.  T = 0 keeps every plane of every block of positive weight (a block of weight 0
has slope 0 and is dropped); a T at or above the start-point sum gives the start points, 0 bytes on the device's tables.

Layers: targets T_0 >= T_1 >= ... >= T_(L-1), 1 <= L <= 32; layer l is allocate_quality for T_l; kept [L][n] then goes through
layer_cases' normalisation and packet format unchanged.

dB: T = N * peak^2 * q^2 / 10^(dB / 10) with N = W * H * ncomp, peak = 2^precision - 1, q = the plan's quality on a plan that quantises
(its coefficients are the transform times quality) and 1 on a lossless plan.  The band weights are synthesis energy gains, so S estimates the
squared error of the colour-TRANSFORMED components, not of RGB, and ignores the rounding of the 5-3: an estimate, not a bound."""
import numpy as np

import rate_cases as rc

WG = 1024              # threads of the allocation's workgroup
MAX_LAYERS = 32
_LANES = np.arange(64)


# ---- the sum --------------------------------------------------------------------------------------------------------------------------------
def wg_sum_f64(terms):
    """float64 terms t_0 ... t_(n-1) -> S, in the order above"""
    t = np.asarray(terms, dtype=np.float64)
    acc = np.zeros(WG, np.float64)
    for k in range(0, len(t), WG):                      # step 1: every thread its own terms, in order
        c = t[k:k + WG]
        acc[:len(c)] = acc[:len(c)] + c
    v = acc.reshape(WG // 64, 64)
    for o in (32, 16, 8, 4, 2, 1):                      # step 2
        v = v + v[:, _LANES ^ o]
    s = 0.0
    for g in range(WG // 64):                           # step 3
        s = s + float(v[g, 0])
    return s


def wg_sum_f64_plain(terms):
    """the same without numpy, lane by lane (tests/test_quality_cases.py)"""
    acc = [0.0] * WG
    for j, x in enumerate(terms):
        acc[j % WG] = acc[j % WG] + float(x)
    for o in (32, 16, 8, 4, 2, 1):
        acc = [acc[i] + acc[(i & ~63) | ((i & 63) ^ o)] for i in range(WG)]
    s = 0.0
    for g in range(WG // 64):
        s = s + acc[g * 64]
    return s


def term(w, D):
    return float(w) * float(int(D))                     # uint64 -> float64 (round to nearest even), one multiply


def weighted_distortion(Ds, ws, ps):
    """S of the choice ps"""
    return wg_sum_f64([term(ws[j], Ds[j][ps[j]]) for j in range(len(ps))])


# ---- the search -----------------------------------------------------------------------------------------------------------------------------
class Hulls:
    """the hulls of every block (rate_cases.hull) as arrays: slopes [n, 32] (-inf behind a hull's end and at its start), the planes, bytes and
    terms of the hull points.  Slopes along a hull fall strictly, so rate_cases.pick = the number of slopes >= lam."""

    def __init__(self, Rs, Ds, nbs, ws):
        n = len(Rs)
        self.n = n
        self.hulls = [rc.hull([int(x) for x in Rs[j]], [int(x) for x in Ds[j]], int(nbs[j]), ws[j]) for j in range(n)]
        self.sl = np.full((n, rc.STRIDE), -np.inf)
        self.pt = np.zeros((n, rc.STRIDE), np.int64)
        self.by = np.zeros((n, rc.STRIDE), np.int64)
        self.tm = np.zeros((n, rc.STRIDE), np.float64)
        for j, (pts, sl) in enumerate(self.hulls):
            assert all(a > b for a, b in zip(sl[1:], sl[2:])), "slopes along a hull fall strictly"
            for i, p in enumerate(pts):
                if i:
                    self.sl[j, i] = sl[i]
                self.pt[j, i], self.by[j, i], self.tm[j, i] = p, int(Rs[j][p]), term(ws[j], Ds[j][p])
        self.rows = np.arange(n)

    def choice(self, bits):
        """(kept, body bytes, S) at the lambda of that bit pattern"""
        lam = rc.bits_to_float(bits)
        with np.errstate(invalid="ignore"):
            i = (self.sl >= lam).sum(axis=1) if self.n else np.zeros(0, np.int64)
        return [int(p) for p in self.pt[self.rows, i]], int(self.by[self.rows, i].sum()), wg_sum_f64(self.tm[self.rows, i])

    def choice_plain(self, bits, Rs, Ds, ws):
        """the same by rate_cases.pick, block by block"""
        lam = rc.bits_to_float(bits)
        ps = [rc.pick(h, lam) for h in self.hulls]
        return ps, sum(int(Rs[j][ps[j]]) for j in range(self.n)), wg_sum_f64_plain([term(ws[j], Ds[j][ps[j]]) for j in range(self.n)])

    def search(self, T, choice=None):
        T = float(T)
        assert T >= 0.0 and T != float("inf"), "a target is finite and >= 0"
        choice = choice or self.choice
        lo, hi = 0, (1 << 63) - 1
        for _ in range(64):
            mid = lo + (hi - lo + 1) // 2
            if choice(mid)[2] <= T:
                lo = mid
            else:
                hi = mid - 1
        return choice(lo)


def allocate_quality(Rs, Ds, nbs, ws, T):
    """tables of every block, a target T -> ([planes kept of every block], body bytes of the choice, its S)"""
    return Hulls(Rs, Ds, nbs, ws).search(T)


def allocate_quality_plain(Rs, Ds, nbs, ws, T):
    """the same with rate_cases.pick and the lane-by-lane sum at every step (slow: small tables only)"""
    H = Hulls(Rs, Ds, nbs, ws)
    return H.search(T, lambda bits: H.choice_plain(bits, Rs, Ds, ws))


def allocate_quality_layers(Rs, Ds, nbs, ws, targets):
    """layer l = allocate_quality(..., targets[l]) -> (kept [L][n], chosen [L], achieved [L]).  Targets fall (or stay); "the largest lambda
    that fits" then makes the cuts monotone in l, asserted here."""
    targets = [float(t) for t in targets]
    assert 1 <= len(targets) <= MAX_LAYERS and all(a >= b for a, b in zip(targets, targets[1:]))
    H = Hulls(Rs, Ds, nbs, ws)
    kept, chosen, achieved = [], [], []
    for T in targets:
        ps, b, s = H.search(T)
        if kept:
            assert all(p >= q for p, q in zip(ps, kept[-1])), "cuts fell with a smaller target"
        kept.append(ps); chosen.append(b); achieved.append(s)
    return kept, chosen, achieved


def float_bits(x):
    return int(np.float64(x).view(np.uint64))


# ---- dB <-> distortion ----------------------------------------------------------------------------------------------------------------------
def psnr_distortion(W, H, ncomp, precision, lossless, quality, db):
    peak = float((1 << int(precision)) - 1)
    q = 1.0 if lossless else float(quality)
    return float(W) * float(H) * float(ncomp) * peak * peak * q * q / 10.0 ** (float(db) / 10.0)


def psnr(sse, nsamples, peak):
    """10 log10(peak^2 n / sse) of an integer sum of squared errors; inf for 0"""
    return float("inf") if sse == 0 else 10.0 * float(np.log10(float(peak) ** 2 * float(nsamples) / float(sse)))


# ---- tables without a device ----------------------------------------------------------------------------------------------------------------
def random_tables(seed, n, zero_weights=True, big=False):
    """(Rs, Ds, nbs, ws): n blocks with rising R, falling D (D[nb] = 0), 0 ... 12 planes; some weights 0; big: D near 2^63, where uint64 ->
    float64 rounds"""
    rng = np.random.default_rng(seed)
    Rs, Ds, nbs, ws = [], [], [], []
    for _ in range(n):
        nb = int(rng.integers(0, 13))
        R = np.zeros(rc.STRIDE, np.uint32)
        D = np.zeros(rc.STRIDE, np.uint64)
        if nb:
            R[1:nb + 1] = np.cumsum(rng.integers(0, 40, nb))
            top = (1 << 63) - int(rng.integers(0, 1 << 20)) if big else int(rng.integers(1, 1 << 24))
            cuts = np.sort(rng.integers(0, top, nb - 1).astype(np.uint64))[::-1] if nb > 1 else np.zeros(0, np.uint64)
            D[0] = top
            D[1:nb] = cuts
        Rs.append(R); Ds.append(D); nbs.append(nb)
        ws.append(0.0 if zero_weights and rng.integers(0, 9) == 0 else float(rng.choice([1.0, 0.7071067811865476, 2.25, 1.9657, 0.5316])))
    return Rs, Ds, nbs, ws


# the table sets of the duality check: (seed, blocks) -- fewer than 64, not a multiple of 64, more than 1024
TABLE_SETS = ((1, 10), (2, 63), (3, 144), (4, 700), (5, 1152), (6, 1203))
