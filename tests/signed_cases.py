"""The yardstick for signed components (j2k_params.is_signed, FramePlan(is_signed=True)), importable without a GPU: tests/test_signed_cases.py
checks it on the CPU, tests/test_gpu_signed.py holds the device against it bit for bit.

What the flag does: the plan builder makes PlanSpec::dc_shift_inv = is_signed ? 0 : dc_shift of it (csrc/j2k_planbuild.cpp, decoder.go:344-348:
the inverse DC level shift is skipped for signed components); the forward path always shifts.  So

  forward            the unsigned plan's expectation (lossless53_cases.expect_forward, oracle.preprocess), and for the frame calls the same bytes
  inverse, int32     the existing definitions with oracle.postprocess(..., is_signed=True): lossless53_cases.expect_inverse, lossy97_cases.expect_inverse,
                     dequantize_cases.expect_dequantized, mallat_cases.inverse_frame (reduce= included) -- each took an is_signed=False keyword for this
  inverse, pixels    oracle.create_image of those planes: decoder.createImage ignores `signed` and clamps negatives to 0
  closed loop        the per-tile decode of closed_loop_ref.oracle_frame's streams (mallat_cases.decoded_tiles, coarse_cases.coarse for skip_planes,
                     area_cases.crop for area=) through the same inverse

Nothing here is computed by the device, and no threshold of a kernel form is restated: the 5-3 cases are picked from the generators of
lossless53_cases by their forms() labels, the 9-7 cases from lossy97_cases.inverse_cases() by their workgroup width.

Not reachable with the flag: a 9-7 plan without the quantiser (Q_NONE) -- those are the one-component host unit calls, whose spec has no DC shift in
either direction.  `quantiser off` is therefore Quality 1 here (step 1.0: the quantiser only rounds), `on` is Quality 75."""
import collections
import functools

import numpy as np

import area_cases as ac
import coarse_cases as cc
import dequantize_cases as dq
import lossless53_cases as ll
import lossy97_cases as l9
import mallat_cases as mc

PIXEL_PRECISIONS = (8, 12, 16)        # what decoder.createImage is asked for in the pixel tests (12: scaled into an image.RGBA64)
SIGNEDRANGE_MIN_SHARE = 0.30
COEFF_FAMILIES_53 = ll.COEFF_FAMILIES                  # noise, fullrange, impulse
COEFF_FAMILIES_97 = l9.COEFF_FAMILIES                  # noise, impulse, outrange (the 9-7 module's own span of int32)


def half(prec):
    return 1 << (prec - 1)


def wrap_sub(frame, prec):
    """frame - 2^(prec - 1) in wrapping int32"""
    f = np.ascontiguousarray(frame, np.int32).view(np.uint32) - np.uint32(half(prec))
    return f.view(np.int32)


# ---- expectations ---------------------------------------------------------------------------------------------------------------------------
expect_forward53 = ll.expect_forward


def expect_inverse53(oracle, coefs, prec, nres, is_signed=True):
    return ll.expect_inverse(oracle, coefs, prec, nres, is_signed=is_signed)


def expect_inverse97(oracle, coefs, prec, nres, quality, dequantize, is_signed=True):
    """dequantize off: tcd.ApplyInverseDWT as written (lossy97_cases.expect_inverse); on: dwt.Dequantize in front (dequantize_cases)"""
    if dequantize:
        return dq.expect_dequantized(oracle, coefs, prec, nres, quality, True, is_signed=is_signed)
    return l9.expect_inverse(oracle, coefs, prec, nres, is_signed=is_signed)


def pixels(oracle, frame, prec):
    """decoder.createImage of an int32 frame [C, h, w]: negatives clamp to 0 whatever `signed` says"""
    return oracle.create_image([frame[c] for c in range(frame.shape[0])], prec)


def clamp_shares(frame, prec):
    """(share of the samples createImage clamps to 0, share strictly between 0 and maxVal)"""
    f = np.asarray(frame, np.int64)
    top = (1 << prec) - 1
    return float(np.mean(f < 0)), float(np.mean((f > 0) & (f < top)))


# ---- signedrange: the transform of a frame uniform over 0 ... 2^prec - 1 ----------------------------------------------------------------------
def uniform_frame(w, h, C, prec, seed=0):
    rng = np.random.default_rng([abs(int(seed)), w, h, C, prec, 9053])
    return rng.integers(0, 1 << prec, size=(C, h, w)).astype(np.int32)


@functools.lru_cache(None)
def _signedrange(w, h, C, prec, nres, seed, lossless, quality, mallat):
    import oracle
    frame = uniform_frame(w, h, C, prec, seed)
    if mallat:
        co = mc.forward_tile(oracle, frame, prec, nres, lossless, quality)
    elif lossless:
        co = ll.expect_forward(oracle, frame, prec, nres)
    else:
        co = np.stack(oracle.preprocess([np.ascontiguousarray(frame[c]) for c in range(C)], w, h, prec, False, nres, quality))
    co = np.ascontiguousarray(co, np.int32)
    co.setflags(write=False)
    frame.setflags(write=False)
    return co, frame


def signedrange_set(w, h, C, prec, nres, seed=0, lossless=True, quality=0, mallat=False):
    """(coefficients [C, h, w], the frame they are the oracle's forward transform of).  Lossless: the signed reconstruction is that frame minus
    2^(prec - 1), so about half of the samples clamp to 0 and half land strictly inside the range (tests/test_signed_cases.py asserts the shares)"""
    return _signedrange(w, h, C, prec, nres, seed, bool(lossless), int(quality), bool(mallat))


# ---- 5-3 cases: by form label -----------------------------------------------------------------------------------------------------------------
GENERATORS_53 = (ll.marching_plane_cases, ll.marching_rgb_cases, ll.plane_wg_cases, ll.tail_deep_cases)


def inverse_labels(case):
    """the form labels of j2k_plan_inverse on the case's int32 frame (level 0, the deeper levels, the tail / deep launch)"""
    return {f for f, _d, _io in case.forms("inv")}


def _area(c):
    return c.W * c.H


@functools.lru_cache(None)
def generator_labels_53():
    """{label: smallest-area case} over the generators above"""
    best = {}
    for gen in GENERATORS_53:
        for c in gen():
            for lab in inverse_labels(c):
                if lab not in best or _area(c) < _area(best[lab]):
                    best[lab] = c
    return best


@functools.lru_cache(None)
def cases_53():
    """for every inverse form label the smallest-area case; the smallest four-component case (a triple plus a single plane); a case for each
    of the precisions 8 / 12 / 16 / 31 the labels did not bring"""
    best = generator_labels_53()
    out = [best[lab] for lab in sorted(best)]
    pool = [c for gen in GENERATORS_53 for c in gen()]
    out.append(min((c for c in pool if c.C == 4), key=_area))
    for prec in ll.PRECISIONS:
        if not any(c.prec == prec for c in out):
            out.append(min((c for c in pool if c.prec == prec), key=_area))
    return tuple(dict.fromkeys(out))


# ---- 9-7 cases: by workgroup width ------------------------------------------------------------------------------------------------------------
class Case97(collections.namedtuple("Case97", "nw W H tile prec nres quality dequantize families")):
    __slots__ = ()

    @property
    def id(self):
        return "nw%d-%dx%d-t%dx%d-p%d-r%d-q%d-dq%d" % (self.nw, self.W, self.H, self.tile[0], self.tile[1], self.prec, self.nres, self.quality, int(self.dequantize))


def label_97(c):
    """the level-0 inverse a context with J2K_L0_WG97_INV = nw runs on the case: the workgroup form of that width where the geometry is admitted
    (lossy97_cases.wg_admitted), else the general kernel"""
    return "inv97_wg<nw%d>" % c.nw if c.nw and l9.wg_admitted(c.W, c.H, c.tile) else "inv97_march"


@functools.lru_cache(None)
def generator_labels_97():
    best = {}
    for c in l9.inverse_cases():
        lab = label_97(c)
        if lab not in best or _area(c) < _area(best[lab]):
            best[lab] = c
    return best


QUANT_VARIANTS = ((75, False), (75, True), (1, False))      # (Quality, dequantise): quantiser on, on + dequantised, off (step 1.0)


@functools.lru_cache(None)
def cases_97():
    out = []
    best = generator_labels_97()
    for i, lab in enumerate(sorted(best)):
        c = best[lab]
        for k, (q, deq) in enumerate(QUANT_VARIANTS):
            out.append(Case97(c.nw, c.W, c.H, c.tile, l9.PRECISIONS[(i + k) % 3], c.nres, q, deq, c.families))
    return tuple(out)


# ---- Mallat cases: partial tiles on both axes, every reduce ----------------------------------------------------------------------------------------
# (W, H, components, precision, tile, resolutions, lossless, Quality, dequantise)
MALLAT = (
    (130, 70, 3, 8, (64, 64), 3, True, 0, False),
    (130, 70, 1, 16, (64, 64), 3, True, 0, False),
    (130, 70, 3, 12, (64, 64), 3, False, 75, True),
    (130, 70, 3, 8, (64, 64), 3, False, 75, False),
)


def mallat_id(m):
    return "%dx%dx%d-p%d-%s-dq%d" % (m[0], m[1], m[2], m[3], "53" if m[6] else "97q%d" % m[7], int(m[8]))


def mallat_tiles(m, family, seed=0):
    """coefficient tiles [C, h, w] of one family in the plan's order (`signedrange`: the oracle's forward transform per tile)"""
    W, H, Cn, prec, tile, nres, lossless, quality, _ = m
    out = []
    for t, (x0, y0, w, h) in enumerate(mc.tiles_of(W, H, tile)):
        if family == "signedrange":
            out.append(np.array(signedrange_set(w, h, Cn, prec, nres, seed + t, lossless, quality, True)[0]))
        elif lossless:
            out.append(np.stack([ll.coeff_plane(family, w, h, seed + 5 * t + c) for c in range(Cn)]))
        else:
            out.append(np.stack([l9.coeff_plane(family, w, h, seed + 7 * t + c, (l9.defaults()["band_prows_97"],)) for c in range(Cn)]))
    return out


def mallat_frame(oracle, m, tiles, reduce=0, is_signed=True, **kw):
    W, H, _Cn, prec, tile, nres, lossless, quality, deq = m
    return mc.inverse_frame(oracle, tiles, W, H, tile, prec, nres, lossless, quality, deq, reduce, is_signed=is_signed, **kw)


# ---- packed pixels: the cases whose UNSIGNED inverse writes the pixels in a level-0 kernel ---------------------------------------------------------
def pixel_inverse_routes(case):
    """the (label, format) routes of the unsigned plan's inverse_pixels that write packed pixels themselves"""
    return {(f, io) for f, _d, io in case.forms("inv") if io in ll.PIX_NAMES}


@functools.lru_cache(None)
def pixel_cases():
    """from lossless53_cases.packed_cases() and rgba8_cases(): the smallest-area case behind every pixel-writing inverse route of an unsigned plan
    (RGBA8 workgroup, plane workgroup for Gray8 / Gray16 / a byte or 16 bits of NRGBA / RGBA64 triples, the pixel-writing marching kernels,
    the merged launch) and behind each of the six source formats; a signed plan must stage every one of them"""
    best = {}
    for c in ll.packed_cases() + ll.rgba8_cases():
        for key in list(pixel_inverse_routes(c)) + [("format", c.fmt)]:
            if key not in best or _area(c) < _area(best[key]):
                best[key] = c
    return tuple(dict.fromkeys(best[k] for k in sorted(best, key=str)))


def pixel_routes_covered():
    return sorted({r for c in pixel_cases() for r in pixel_inverse_routes(c)})


@functools.lru_cache(None)
def pixel_cases_97():
    """(W, H, tile, resolutions): RGB at 8 bit, Quality 75, where the default workgroup form of the 9-7 inverse writes RGBA8 pixels on an unsigned
    plan -- the smallest and the widest shape of lossy97_cases.wg_shapes at the default width, and its tiled frame"""
    nw = l9.defaults()["l0_wg97_inv"]
    shapes = [(w, h) for w, h in l9.wg_shapes(nw) if h >= 2 and w % 8 == 0]
    small = min(shapes, key=lambda s: s[0] * s[1])
    wide = max(shapes, key=lambda s: (s[0], s[1]))
    W, H, tile = l9.tiled_frames(nw)[0]
    return ((small[0], small[1], (0, 0), 2), (wide[0], wide[1], (0, 0), 3), (W, H, tile, 3))


# ---- the closed loop ---------------------------------------------------------------------------------------------------------------------------
def decoded_tiles(oracle, want, Cn, nres, cb, coder, skip_planes=0):
    """what the block decoder gives back per tile of closed_loop_ref.oracle_frame's streams, stopped after bit plane skip_planes (MQ)"""
    tiles = mc.decoded_tiles(oracle, want, Cn, nres, cb, coder)
    return cc.coarse_tiles(tiles, skip_planes) if skip_planes else tiles


def closed_loop_frame(oracle, tiles, W, H, tile, prec, nres, lossless=True, quality=0, dequantize=False, mallat=False, reduce=0, frame_rows=0,
                      only=None, fill=0, is_signed=True):
    """decoded coefficient tiles -> the int32 frame [C, H_r, W_r] of a closed-loop decode; only: the tile numbers written (a shard)"""
    if mallat:
        return mc.inverse_frame(oracle, tiles, W, H, tile, prec, nres, lossless, quality, dequantize, reduce, frame_rows, only, fill, is_signed=is_signed)
    assert reduce == 0
    out = np.full((tiles[0].shape[0], H, W), fill, np.int32)
    for t, (x0, y0, w, h) in enumerate(mc.tiles_of(W, H, tile, frame_rows)):
        if only is not None and t not in only:
            continue
        if lossless:
            out[:, y0:y0 + h, x0:x0 + w] = expect_inverse53(oracle, tiles[t], prec, nres, is_signed)
        else:
            out[:, y0:y0 + h, x0:x0 + w] = expect_inverse97(oracle, tiles[t], prec, nres, quality, dequantize, is_signed)
    return out


def crop(full_pix, area, reduce, bpp):
    return ac.crop(full_pix, area, reduce, bpp)


# the frame calls: 200 x 72 in 64 x 64 tiles (partial tiles on both axes), 3 resolutions
FRAME_W, FRAME_H, FRAME_TILE, FRAME_NRES = 200, 72, (64, 64), 3
# name -> (components, precision, pixel format, bytes per pixel, SOP / EPH, code-block size, FramePlan keywords)
FRAME_PLANS = {
    "mq_rgba8": (3, 8, 2, 4, True, 32, dict(lossless=True, coder=0, closed_loop=True)),
    "ht_gray8": (1, 8, 0, 1, False, 16, dict(lossless=True, coder=1, closed_loop=True)),
    "mallat_mq_gray16": (1, 16, 1, 2, True, 32, dict(lossless=True, coder=0, mallat=True)),
    "lossy_dq_rgba8": (3, 8, 2, 4, True, 32, dict(lossless=False, quality=75, coder=0, closed_loop=True, dequantize=True)),
}
FRAME_AREA = (50, 40, 140, 70)          # straddles the corner of tiles 0, 1, 4, 5 at (64, 64)
FRAME_SHARDS = ((0, 3), (3, 5))         # tile_first, tile_count: the eight tiles in two parts, the cut inside the first tile row
