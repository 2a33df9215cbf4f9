"""Named, seeded cases for the lossy 9-7 path (csrc/dwt97.hip, dwt97_l0wg.inc, dwt97_l0wg_inv.inc): the shapes at which its kernel forms change
behaviour and the contents that make a mistake visible where it happens.  Importable without a GPU: tests/test_lossy97_cases.py checks the
lists on the CPU, tests/test_gpu_lossy97_oracle.py runs them against the oracle on the device.

Shapes come from the code's own constants.  The context defaults (waves per workgroup of the three workgroup forms, pair-rows per band of the
marching kernels) are read from csrc/j2k_plan.h; the strip advance of the marching kernels is (64 - halo) * cpl columns (make_jobs,
j2k_planbuild.cpp) with cpl = 2 (halo 2) for planes narrower than 192 columns and for RGB triples, cpl = 4 (halo 1) otherwise; a workgroup
of NW waves owns NR = NW - 3 pair-rows.

Contents: `noise` is what the older tests use; `impulse`, `step`, `const`, `checker` put an edge on a known row / column (symmetric
extension, strip seam, band seam, tile edge); `outrange` leaves int32 in a few rows and keeps the others inside it; the float64 families
reach the ends of the format (`subnormal`, `huge`, `overflow`)."""
import collections
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_H = os.path.join(ROOT, "go-jpeg2000_amd", "csrc", "j2k_plan.h")

# the values the options accept besides the default (j2k_ctx.cpp: l0_wg97, l0_wg97_inv, plane_wg97); 0 = the general marching kernels
FWD_WAVES = (0, 6, 8, 10, 12, 14, 16)
INV_WAVES = (0, 6, 8, 10, 12)
PLANE_WAVES = (0, 8)
QUALITIES = (1, 2, 3, 75, 100, 101, 4097, 8191)
PRECISIONS = (8, 12, 16)
NRES = (1, 2, 3, 6)          # levels 5 (encoder.go:249-252: none given), 1 (no float64 prefix), 2 (one prefix), 5 (a deep prefix)
INT_FRAME_FAMILIES = ("noise", "impulse", "step", "const", "checker", "outrange")
COEFF_FAMILIES = ("noise", "impulse", "outrange")
FLOAT_FAMILIES = ("noise", "subnormal", "huge", "overflow")
OUTRANGE_MIN_H = 10          # below this every output row is within filter reach of the rows that leave int32
TWO31 = 2147483648.0


@functools.lru_cache(None)
def defaults():
    """{l0_wg97, l0_wg97_inv, plane_wg97, band_prows_97}: the context defaults, from the struct that holds them"""
    with open(PLAN_H) as f:
        text = f.read()
    out = {}
    for name in ("l0_wg97", "l0_wg97_inv", "plane_wg97", "band_prows_97"):
        m = re.search(r"\bint\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, "no default for %s in %s" % (name, PLAN_H)
        out[name] = int(m.group(1))
    return out


def levels_of(nres):
    return nres - 1 if nres - 1 > 0 else 5          # encoder.go:249-252


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
STRIP_SEAMS = (124, 128, 248, 252, 256, 504, 508)   # (64 - 2) * 2 and its multiples, (64 - 1) * 4 and its multiple, the strips' own widths
WG_WIDTHS = (16, 24, 248, 504, 512)


def march_widths():
    return sorted({s + d for s in STRIP_SEAMS for d in (-1, 0, 1, 2)})


def march_heights(band=None):
    band = band or defaults()["band_prows_97"]
    return [1, 2, 3] + [2 * band * k + d for k in (1, 2) for d in (-1, 0, 1)]


@functools.lru_cache(None)
def march_shapes():
    """every seam width with a height, every seam height with three widths at least: planes of 800 x 33 at the most"""
    ws, hs = march_widths(), march_heights()
    out = [(w, hs[i % len(hs)]) for i, w in enumerate(ws)]
    out += [(ws[(5 * i + 2) % len(ws)], h) for i, h in enumerate(hs)]
    return tuple(dict.fromkeys(out))


def wg_heights(nw):
    nr = nw - 3
    halves = (1, 2, nr - 1, nr, nr + 1, 2 * nr, 2 * nr + 1)
    return sorted({h for q in halves for h in (2 * q - 1, 2 * q) if h >= 1})


@functools.lru_cache(None)
def wg_shapes(nw):
    """heights with halfH on, one below and one past the band of NR = nw - 3 pair-rows (both parities), each with two of the widths"""
    out = []
    for i, h in enumerate(wg_heights(nw)):
        out += [(WG_WIDTHS[i % 5], h), (WG_WIDTHS[(i + 2) % 5], h)]
    return tuple(out)


def tiled_frames(nw):
    """(W, H, tile): tiles of 256 with a ragged last tile column and a ragged last tile row.  One plane outside the workgroup form's
    admission rule (wg_admitted) puts the whole plan on the marching kernels, so the last column of 8 goes to them alone (nw 0); a
    workgroup width gets last columns of 16 -- the narrowest plane the form takes -- and 24"""
    nr = (nw or defaults()["l0_wg97_inv"]) - 3
    return ((528 if nw else 520, 2 * nr + 3, (256, 128)), (536, 4 * nr + 5, (256, 4 * nr + 2)))


def wg_admitted(W, H, tile):
    """the level-0 workgroup forms' admission rule (j2k_planbuild.cpp, ok97), restated: every tile plane 16 ... 512 columns, a multiple of
    8, two rows at least, the frame's width a multiple of 4.  A frame that fails it runs the marching kernels whatever the knob says."""
    return W % 4 == 0 and all(16 <= w <= 512 and w % 8 == 0 and h >= 2 for _, _, w, h in tiles_of(W, H, tile))


def seam_cols(w):
    c = {0, w - 1}
    for s in (124, 248, 372, 496, 252, 504, 128, 256, 384):
        c |= {s - 1, s}
    return sorted(x for x in c if 0 <= x < w)


def seam_rows(h, nrs=()):
    bands = {defaults()["band_prows_97"]} | {n for n in nrs if n > 0}
    r = {0, h - 1}
    for b in bands:
        for k in (1, 2, 3):
            r |= {2 * b * k - 1, 2 * b * k}
    return sorted(y for y in r if 0 <= y < h)


def impulse_points(w, h, nrs=()):
    """the corners, one sample on every strip seam column and band seam row, one in the last column and one in the last row"""
    pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w - 1), (h - 1, w // 2)]
    pts += [((7 * i + 3) % h, c) for i, c in enumerate(seam_cols(w))]
    pts += [(r, (11 * i + 5) % w) for i, r in enumerate(seam_rows(h, nrs))]
    return list(dict.fromkeys(pts))


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


# ---- int32 frames -----------------------------------------------------------------------------------------------------------------------
def int_frame(family, w, h, ncomp, prec, seed=0, nrs=()):
    """an int32 frame [ncomp, h, w] of unsigned `prec`-bit samples (`outrange`: with rows that are not)"""
    rng = _rng(seed, w, h, ncomp, prec, INT_FRAME_FAMILIES.index(family))
    top, mid = (1 << prec) - 1, 1 << (prec - 1)
    yy, xx = np.mgrid[0:h, 0:w]
    if family == "noise":
        f = rng.integers(0, top + 1, size=(ncomp, h, w))
    elif family == "const":
        f = np.full((ncomp, h, w), top)
    elif family == "checker":
        f = np.stack([((xx + yy + c) & 1) * top for c in range(ncomp)])
    elif family == "step":                      # a half-plane at full scale: along x, along y, both
        f = np.zeros((ncomp, h, w), np.int64)
        for c in range(ncomp):
            if c % 3 != 1: f[c][:, w // 2:] = top
            if c % 3 != 0: f[c][h // 2:, :] = top - f[c][h // 2:, :]
    elif family == "impulse":                   # mid-grey (zero after the DC shift) with single full-scale samples
        f = np.full((ncomp, h, w), mid)
        for i, (y, x) in enumerate(impulse_points(w, h, nrs)):
            f[i % ncomp, y, x] = top if i & 1 else 0
    elif family == "outrange":
        f = rng.integers(0, top + 1, size=(ncomp, h, w)).astype(np.int64)
        r0 = 1 if h > 1 else 0
        f[:, r0, :] = rng.integers(-2 ** 31, 2 ** 31, size=(ncomp, w))
        lit = [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31 + 1, 2 ** 30, -2 ** 30, 65536, -1]
        f[ncomp // 2, r0, : min(w, 8)] = lit[: min(w, 8)]
        if ncomp >= 3 and w >= 16:
            # after the DC shift r = 2^31 - 1, g = b = -2^31: Cr = 0.5 r - 0.41869 g - 0.08131 b = 2^31 - 0.5, and Cr + 0.5 is 2^31 itself
            f[0, r0, 8:12] = 2 ** 31 - 1 + mid - 2 ** 32
            f[1:3, r0, 8:12] = -2 ** 31 + mid
            f[:, r0, 12:16] = 2 ** 31 - 1 + mid - 2 ** 32          # r = g = b = 2^31 - 1: Y + 0.5 stays just inside
    else:
        raise ValueError(family)
    return np.asarray(f).astype(np.int64).astype(np.int32)


# Frames on which the quotient's correction matters.  The level-0 workgroup kernel divides by the step as q0 = v * RN(1 / step) plus two
# correcting fma (dwt97_l0wg.inc); q0 alone is the quotient's neighbour on a fraction of a percent of the values and changes the
# INTEGER only where the quotient lies within an ulp of k + 0.5 -- about one coefficient in 10^7 at |q| ~ 2^30, never among the
# thousands a noise frame of the declared precision has.  These seeds were searched for on the CPU (3000 frames per Quality); each
# frame has one such coefficient, which tests/test_lossy97_cases.py re-derives from the oracle's own float64 results.
MARKSTEIN_SHAPE = (512, 21, 16, 2)              # W, H, precision, resolutions (one level: every coefficient takes the level-0 quantiser)
MARKSTEIN_FRAMES = ((75, 1347), (75, 1363), (100, 634))         # (Quality, seed)


def markstein_frame(quality, seed):
    """int32 noise of 24 bits (outside the declared precision, inside what the plan takes): quotients near 2^30, inside int32"""
    W, H, _, _ = MARKSTEIN_SHAPE
    return np.random.default_rng([seed, quality, 4242]).integers(-(1 << 23), 1 << 23, size=(3, H, W)).astype(np.int32)


# ---- int32 coefficient planes (the inverse's input: the level's dense matrix, low half first) ----------------------------------------------
def coeff_plane(family, w, h, seed=0, nrs=()):
    rng = _rng(seed, w, h, 77, COEFF_FAMILIES.index(family))
    if family == "noise":
        f = rng.integers(-(1 << 12), 1 << 12, size=(h, w))
    elif family == "impulse":
        f = np.zeros((h, w), np.int64)
        for i, (y, x) in enumerate(impulse_points(w, h, nrs)):
            f[y, x] = (1 << 14) * (1 if i & 1 else -1)
    elif family == "outrange":
        # the first high-pass row of level 0 spans int32 (it reaches the output rows 0 ... 4); everything else stays small
        f = rng.integers(-(1 << 12), 1 << 12, size=(h, w)).astype(np.int64)
        r0 = (h + 1) // 2 if h > 1 else 0
        f[r0, :] = rng.integers(-2 ** 31, 2 ** 31, size=w)
        f[r0, rng.random(w) < 0.5] >>= 3
        lit = [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, 2 ** 30]
        f[r0, : min(w, 6)] = lit[: min(w, 6)]
    else:
        raise ValueError(family)
    return np.asarray(f).astype(np.int64).astype(np.int32)


# ---- float64 planes for the unit calls ----------------------------------------------------------------------------------------------------
def float_plane(family, w, h, seed=0):
    """flat float64 [w * h]; no NaN in any of them"""
    rng = _rng(seed, w, h, 99, FLOAT_FAMILIES.index(family))
    n = w * h
    if family == "noise":
        return rng.uniform(-500, 500, n)
    if family == "subnormal":                   # 2^-1074 ... 2^-1022, either sign, two fifths of the samples +0.0 or -0.0
        x = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-1074, -1022, n)) * rng.choice([-1.0, 1.0], n)
        x = np.clip(x, -2.0 ** -1022, 2.0 ** -1022)
        z = rng.random(n)
        x[z < 0.2] = 0.0
        x[(z >= 0.2) & (z < 0.4)] = -0.0
        return x
    if family == "huge":
        return rng.uniform(-1.0, 1.0, n) * 2.0 ** 1019
    if family == "overflow":
        x = rng.uniform(-500, 500, n).reshape(h, w)
        big = 1.5e308
        if n < 8:
            x[0, 0] = big
            x[-1, -1] = -big if n == 2 else big       # (three samples: the two neighbours of the middle one must not cancel)
        else:
            pts = [(0, min(1, w - 1), big),                       # the neighbour of the first column / row: the mirrored edge term
                   (h - 1, max(w - 2, 0), -big),
                   (h // 2, w // 2, big), (h // 2, min(w // 2 + 2, w - 1), big),          # two of one sign around one sample: the sum is inf
                   (h // 3, w // 3, big), (h // 3, min(w // 3 + 2, w - 1), -big)]         # opposite signs: inf - inf further on
            if h > 4:
                pts += [(min(1, h - 1), w // 4, -big), (h - 2, (3 * w) // 4, big)]
            for y, xx, v in pts:
                x[y, xx] = v
        return x.reshape(-1)
    raise ValueError(family)


def same_floats(a, b):
    """bit patterns of the non-NaN values and NaN-ness elementwise (NaN payloads are not something the reference pins)"""
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    b = np.ascontiguousarray(b, np.float64).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


# ---- the reference's conversions, restated to COUNT what the oracle only does ------------------------------------------------------------
def go_int32(v):
    """Go's int32(float64) on amd64 and which elements took its out-of-range result (oracle/j2k_oracle.c go_int32)"""
    v = np.asarray(v, np.float64)
    ok = (v < TWO31) & (v > -TWO31 - 1.0)
    with np.errstate(invalid="ignore"):
        out = np.where(ok, np.trunc(np.where(ok, v, 0.0)), -TWO31).astype(np.int64).astype(np.int32)
    return out, ~ok


def round_half_away(v):
    v = np.asarray(v, np.float64)
    return go_int32(np.where(v >= 0, v + 0.5, v - 0.5))


def forward_counts(oracle, frame, prec, nres, quality):
    """encoder.preprocess on one tile, step by step on the oracle's float64 functions: (coefficients [C, h, w], out-of-range conversions per
    coefficient row [h] -- a pixel's ICT conversions count on its own row --, conversions whose rounded sum is 2^31 exactly)"""
    C, h, w = frame.shape
    s = np.stack([oracle.dc_shift_fwd(frame[c].reshape(-1), prec).reshape(h, w) for c in range(C)])
    rows = np.zeros(h, np.int64)
    exact = 0
    if C >= 3:
        y = oracle.ict_fwd(*[s[c].astype(np.float64).reshape(-1) for c in range(3)])
        for c in range(3):
            v = y[c].reshape(h, w)
            t, bad = round_half_away(v)
            exact += int(np.count_nonzero(np.where(v >= 0, v + 0.5, v - 0.5) == TWO31))
            rows += bad.sum(axis=1)
            s[c] = t
    step = 1.0 / float(quality if quality > 0 else 100)
    out = []
    for c in range(C):
        f = oracle.decompose97(s[c].astype(np.float64), w, h, levels_of(nres))
        q = np.where(f >= 0, f / step + 0.5, f / step - 0.5)
        t, bad = go_int32(q)
        exact += int(np.count_nonzero(q == TWO31))
        rows += bad.sum(axis=1)
        out.append(t)
    return np.stack(out), rows, exact


def inverse_counts(oracle, coefs, prec, nres):
    """the decode side of one tile (tcd.ApplyInverseDWT, InverseICT, DC shift) the same way: (frame [C, h, w], out-of-range conversions per
    output row [h])"""
    C, h, w = coefs.shape
    rows = np.zeros(h, np.int64)
    t = []
    for c in range(C):
        f = oracle.reconstruct97(coefs[c].astype(np.float64), w, h, levels_of(nres))
        v, bad = go_int32(f + 0.5)
        rows += bad.sum(axis=1)
        t.append(v)
    if C >= 3:
        rgb = oracle.ict_inv(*[t[c].astype(np.float64).reshape(-1) for c in range(3)])
        for c in range(3):
            v, bad = go_int32(rgb[c].reshape(h, w) + 0.5)
            rows += bad.sum(axis=1)
            t[c] = v
    out = np.stack([oracle.dc_shift_inv(p.reshape(-1), prec).reshape(h, w) for p in t])
    return out, rows


def expect_inverse(oracle, coefs, prec, nres, is_signed=False):
    """the composition tests/test_gpu_dwt97.py::test_plan_forward_lossy uses for the decode side of one tile"""
    C, h, w = coefs.shape
    inv = [oracle.tcd_inverse_dwt(coefs[c], w, h, levels_of(nres), 0) for c in range(C)]
    return np.stack(oracle.postprocess(inv, prec, False, is_signed=is_signed))


# ---- pyref's 1-D transforms on whole rows / columns at a time ----------------------------------------------------------------------------------
def pyref_2d(pyref, x, w, h, inverse):
    """pyref.forward97 / inverse97 -- the literal Python restatement of dwt.go:161-262 -- applied as dwt.go:432-473 applies them, with every
    row (then every column) as one list element: the same IEEE operations per sample as the scalar call, in numpy lanes"""
    a = np.array(x, np.float64).reshape(h, w)

    def along(m, n, fn):            # transform along axis 0 of m [n, lanes]
        d = [m[i].copy() for i in range(n)]
        fn(d, n)
        return np.stack(d) if n else m

    with np.errstate(all="ignore"):
        if not inverse:
            a = along(a.T.copy(), w, pyref.forward97).T.copy()     # rows first (dwt.go:436-441)
            a = along(a, h, pyref.forward97)
        else:
            a = along(a, h, pyref.inverse97)                       # columns first (dwt.go:458-465)
            a = along(a.T.copy(), w, pyref.inverse97).T.copy()
    return a


def pyref_multilevel(pyref, x, w, h, levels, inverse):
    """dwt.go:551-573 around pyref_2d: level l works on the prefix of the slice"""
    d = np.array(x, np.float64).reshape(-1)
    dims = []
    for _ in range(levels):
        dims.append((w, h)); w = (w + 1) // 2; h = (h + 1) // 2
    for lw, lh in (reversed(dims) if inverse else dims):
        d[:lw * lh] = pyref_2d(pyref, d[:lw * lh], lw, lh, inverse).reshape(-1)
    return d


# ---- the case lists both test files walk -------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "nw W H tile prec nres quality families")):
    """nw = waves per workgroup of the form under test (0: the marching kernels)"""
    __slots__ = ()

    @property
    def id(self):
        return "nw%d-%dx%d-t%dx%d-p%d-r%d-q%d" % (self.nw, self.W, self.H, self.tile[0], self.tile[1], self.prec, self.nres, self.quality)


def _rgb_shapes(nw, default_nw):
    """what a context with `nw` waves runs: its own band seams; the marching kernels (nw 0) get the strip seams and the default form's
    shapes.  A plane of one row is not admitted to the workgroup form: it runs once, under nw 0."""
    if nw:
        return [(w, h) for w, h in wg_shapes(nw) if h >= 2]
    return list(march_shapes()) + list(wg_shapes(default_nw))[::2]


@functools.lru_cache(None)
def inverse_cases():
    """level 0 of the inverse, RGB + ICT, for every J2K_L0_WG97_INV: precisions and resolution counts go round with the shapes (every pair of
    them at every width of the form), `outrange` wherever a row can stay inside int32"""
    out = []
    for nw in INV_WAVES:
        for i, (w, h) in enumerate(_rgb_shapes(nw, defaults()["l0_wg97_inv"])):
            fam = tuple(f for f in COEFF_FAMILIES if f != "outrange" or h >= OUTRANGE_MIN_H)
            out.append(Case(nw, w, h, (0, 0), PRECISIONS[i % 3], NRES[i % 4], 75, fam))
        for i, (W, H, tile) in enumerate(tiled_frames(nw)):
            out.append(Case(nw, W, H, tile, PRECISIONS[(i + nw // 2) % 3], NRES[(i + 1 + nw // 2) % 4], 75, COEFF_FAMILIES))
    return tuple(out)


@functools.lru_cache(None)
def forward_cases():
    """level 0 of the forward path, RGB + ICT, for every J2K_L0_WG97: the qualities go round with the shapes (each at three shapes of a form
    at least); `outrange` for two of the widths and the marching kernel, the edge patterns for the default form and the marching kernel"""
    d = defaults()["l0_wg97"]
    out = []
    for nw in FWD_WAVES:
        for i, (w, h) in enumerate(_rgb_shapes(nw, d)):
            fam = ["noise", "step"]
            if nw in (0, d, 12) and h >= OUTRANGE_MIN_H: fam.append("outrange")
            if nw in (0, d): fam += ["impulse", "const", "checker"]
            out.append(Case(nw, w, h, (0, 0), PRECISIONS[(i // 2) % 3], NRES[(i + 1) % 4], QUALITIES[i % 8], tuple(fam)))
        for i, (W, H, tile) in enumerate(tiled_frames(nw)):
            out.append(Case(nw, W, H, tile, PRECISIONS[i % 3], NRES[(i + 3) % 4], QUALITIES[(3 + i + nw // 2) % 8], ("noise", "step")))
    return tuple(out)


def tiles_of(W, H, tile):
    """(x0, y0, w, h) of every tile, in the plan's order"""
    tw, th = tile[0] or W, tile[1] or H
    return [(x0, y0, min(tw, W - x0), min(th, H - y0)) for y0 in range(0, H, th) for x0 in range(0, W, tw)]


# single components and deeper levels (J2K_PLANE_WG97): (W, H, ncomp, tile, nres, prec, quality).  The workgroup form takes a level when
# EVERY plane of it is 16 ... 512 columns wide, a multiple of 8, and two rows high at least (j2k_planbuild.cpp)
PLANE_FRAMES = (
    (512, 33, 1, (0, 0), 4, 12, 50), (24, 17, 1, (0, 0), 3, 8, 75), (248, 10, 1, (0, 0), 2, 16, 8191), (520, 21, 1, (256, 16), 3, 8, 1),
    (256, 11, 4, (128, 0), 3, 16, 101), (64, 2, 1, (0, 0), 2, 8, 3), (504, 9, 4, (0, 0), 6, 12, 2),
    # RGB frames whose level-1 planes straddle the rule: 12 columns (too narrow), 16 (the narrowest), 20 (not a multiple of 8), 24, 512 (the
    # widest), 516 (too wide); tiles of 256 next to a last tile of 24 columns (level 1: 128 beside 12) and of 32 (128 beside 16)
    (24, 19, 3, (0, 0), 3, 12, 75), (32, 19, 3, (0, 0), 3, 12, 75), (40, 19, 3, (0, 0), 4, 8, 100), (48, 18, 3, (0, 0), 6, 16, 4097),
    (1024, 12, 3, (0, 0), 3, 12, 75), (1032, 12, 3, (0, 0), 3, 12, 75), (280, 21, 3, (256, 0), 4, 12, 75), (288, 21, 3, (256, 0), 4, 8, 1),
)


@functools.lru_cache(None)
def float_shapes():
    return tuple(dict.fromkeys(list(march_shapes()) + list(wg_shapes(defaults()["plane_wg97"]))))


LENGTHS_1D = (1, 2, 3) + tuple(range(125, 130)) + tuple(range(253, 258))
