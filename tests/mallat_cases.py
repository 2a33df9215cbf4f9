"""The yardstick for Mallat plans (j2k_params.closed_loop = J2K_CLOSED_LOOP_MALLAT, FramePlan(mallat=True)) and their reduced-resolution decode,
importable without a GPU: tests/test_mallat_ref.py checks it on the CPU, tests/test_gpu_mallat.py holds the device against it bit for bit.

The expectation is composed from the oracle's existing entry points only.  One tile-component is a dense w x h plane; w_0 = w, w_{l+1} =
ceil(w_l / 2), the same for h; level l is the reference's single-level 2-D transform on a contiguous copy of the RECTANGLE [0, w_l) x [0, h_l),
written back into the rectangle:

  forward, lossless   dc_shift_fwd -> rct_fwd (C >= 3) -> per level fwd53_2d
  forward, lossy      dc_shift_fwd -> ict_fwd on float64 -> round half away to int32 (encoder.go:236-244) -> float64 -> per level fwd97_2d
                      -> go_int32(v / step +- 0.5), the sign of v, step = 1.0 / float(Quality) (encoder.go:265-276)
  inverse to reduce r (x step when dequantising) -> inv53_2d / inv97_2d on the rectangles of levels L-1 ... r -> crop [0, w_r) x [0, h_r)
                      -> go_int32(f + 0.5) for 9-7 -> postprocess; the tile at (x0 >> r, y0 >> r) of the ceil(W / 2^r) x ceil(H / 2^r) frame
  streams             encode_tile_blocks(coeff, windows=1) and the packet loop of closed_loop_ref.oracle_frame: only the coefficients differ

`level=` of forward_tile swaps the per-level step for the oracle's own multi-level call (decompose53 / decompose97, the prefix layout): that must
give oracle.preprocess bit for bit, which proves that the glue around the levels is the oracle's."""
import numpy as np

import closed_loop_ref as ref
import lossless53_cases as ll
import lossy97_cases as lc


def levels_of(nres):
    return ll.levels_of(nres)


def dims(w, h, levels):
    """[(w_0, h_0), ..., (w_L, h_L)]"""
    out = [(w, h)]
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def step_of(quality):
    return 1.0 / float(quality if quality > 0 else 100)


def _levels_fwd(oracle, plane, w, h, levels, lossless, prefix):
    if prefix:      # the reference's multi-level call: level l + 1 on the first w_{l+1} h_{l+1} LINEAR elements
        return (oracle.decompose53 if lossless else oracle.decompose97)(plane, w, h, levels)
    p = np.array(plane, dtype=np.int32 if lossless else np.float64).reshape(h, w)
    for wl, hl in dims(w, h, levels)[:levels]:
        rect = np.ascontiguousarray(p[:hl, :wl])
        p[:hl, :wl] = (oracle.fwd53_2d if lossless else oracle.fwd97_2d)(rect, wl, hl)
    return p


def forward_tile(oracle, crop, prec, nres, lossless=True, quality=0, prefix=False):
    """one tile int32 [C, h, w] -> coefficients int32 [C, h, w]"""
    C, h, w = crop.shape
    L = levels_of(nres)
    s = [oracle.dc_shift_fwd(np.ascontiguousarray(crop[c]).reshape(-1), prec).reshape(h, w) for c in range(C)]
    if lossless:
        if C >= 3:
            s[:3] = [p.reshape(h, w) for p in oracle.rct_fwd(*[s[c].reshape(-1) for c in range(3)])]
        return np.stack([_levels_fwd(oracle, s[c], w, h, L, True, prefix) for c in range(C)]).astype(np.int32)
    if C >= 3:
        y = oracle.ict_fwd(*[s[c].astype(np.float64).reshape(-1) for c in range(3)])
        s[:3] = [lc.round_half_away(y[c].reshape(h, w))[0] for c in range(3)]
    step = step_of(quality)
    out = []
    for c in range(C):
        f = _levels_fwd(oracle, s[c].astype(np.float64), w, h, L, False, prefix)
        with np.errstate(all="ignore"):
            q = np.where(f >= 0, f / step + 0.5, f / step - 0.5)
        out.append(lc.go_int32(q)[0])
    return np.stack(out)


def inverse_tile(oracle, coefs, prec, nres, lossless=True, quality=0, dequantize=False, reduce=0, is_signed=False):
    """one tile's coefficients int32 [C, h, w] -> int32 [C, h_r, w_r]"""
    C, h, w = coefs.shape
    L = levels_of(nres)
    d = dims(w, h, L)
    assert 0 <= reduce <= L
    wr, hr = d[reduce]
    planes = []
    for c in range(C):
        if lossless:
            p = np.array(coefs[c], dtype=np.int32)
        else:
            p = coefs[c].astype(np.float64)
            if dequantize:
                p = p * step_of(quality)                                # dwt.go:517
        for l in range(L - 1, reduce - 1, -1):
            wl, hl = d[l]
            rect = np.ascontiguousarray(p[:hl, :wl])
            p[:hl, :wl] = (oracle.inv53_2d if lossless else oracle.inv97_2d)(rect, wl, hl)
        p = np.ascontiguousarray(p[:hr, :wr])
        planes.append(p if lossless else lc.go_int32(p + 0.5)[0])       # tcd.go:433-435
    return np.stack(oracle.postprocess(planes, prec, lossless, mct=C >= 3, is_signed=is_signed))


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
def tiles_of(W, H, tile, frame_rows=0):
    """(x0, y0, w, h) of every tile in the plan's order; frame_rows: a batch, the grid starts again at every frame"""
    fh = frame_rows or H
    out = []
    for f in range(H // fh):
        out += [(x0, f * fh + y0, w, h) for x0, y0, w, h in ll.tiles_of(W, fh, tile)]
    return out


def shr(v, r):
    return (v + (1 << r) - 1) >> r


def admissible(W, H, tile, nres, frame_rows=0):
    """the `reduce` values the geometry allows: 0 ... L, a tiled dimension's tile size and a batch's frame_rows multiples of 2^reduce"""
    fh = frame_rows or H
    tw, th = tile[0] or W, tile[1] or fh
    out = []
    for r in range(levels_of(nres) + 1):
        m = (1 << r) - 1
        if (tw < W and tw & m) or (th < fh and th & m) or (fh < H and fh & m):
            continue
        out.append(r)
    return out


def reduced_rects(W, H, tile, r, frame_rows=0):
    """(x, y, w, h) of every tile in the reduced frame"""
    return [(x0 >> r, y0 >> r, shr(w, r), shr(h, r)) for x0, y0, w, h in tiles_of(W, H, tile, frame_rows)]


def forward_frame(oracle, frm, tile, prec, nres, lossless=True, quality=0, frame_rows=0, prefix=False):
    """int32 [C, H, W] -> list of coefficient tiles int32 [C, h, w] in the plan's order"""
    _, H, W = frm.shape
    return [forward_tile(oracle, np.ascontiguousarray(frm[:, y0:y0 + h, x0:x0 + w]).astype(np.int32), prec, nres, lossless, quality, prefix)
            for x0, y0, w, h in tiles_of(W, H, tile, frame_rows)]


def inverse_frame(oracle, tiles, W, H, tile, prec, nres, lossless=True, quality=0, dequantize=False, reduce=0, frame_rows=0, only=None, fill=0,
                  is_signed=False):
    """coefficient tiles -> the reduced frame int32 [C, H_r, W_r]; only: the tile numbers written (a shard), the rest holds `fill`"""
    C = tiles[0].shape[0]
    out = np.full((C, shr(H, reduce), shr(W, reduce)), fill, np.int32)
    for t, (x, y, w, h) in enumerate(reduced_rects(W, H, tile, reduce, frame_rows)):
        if only is not None and t not in only:
            continue
        got = inverse_tile(oracle, tiles[t], prec, nres, lossless, quality, dequantize, reduce, is_signed)
        assert got.shape == (C, h, w)
        out[:, y:y + h, x:x + w] = got
    return out


def flat_coeff(plan_planes, tiles, n):
    """the plan's flat coefficient buffer (FramePlan.planes(): tile, comp, x0, y0, w, h, offset) from coefficient tiles"""
    buf = np.zeros(n, np.int32)
    for t, c, _x0, _y0, w, h, off in (tuple(int(v) for v in r) for r in plan_planes):
        buf[off:off + w * h] = tiles[t][c].reshape(-1)
    return buf


def pixels(oracle, frame, prec):
    """decoder.createImage of an int32 frame [C, h, w]: it clamps, and reduced frames do leave 0 ... 2^prec - 1"""
    return oracle.create_image([frame[c] for c in range(frame.shape[0])], prec)


# ---- streams: closed_loop_ref.oracle_frame with the Mallat coefficients in place of encoder.preprocess ------------------------------------
class MallatOracle:
    """the oracle with `preprocess` replaced by forward_tile: everything oracle_frame does after the transform stays its own"""

    def __init__(self, oracle):
        self._o = oracle

    def __getattr__(self, name):
        return getattr(self._o, name)

    def preprocess(self, planes, w, h, precision, lossless, num_resolutions, quality=0):
        crop = np.stack([np.asarray(p, np.int32).reshape(h, w) for p in planes])
        return [p for p in forward_tile(self._o, crop, precision, num_resolutions, bool(lossless), quality)]


def oracle_frame(frm, W, H, tw, th, nres, cb, coder, sop, eph, orc, t2ref, **kw):
    return ref.oracle_frame(frm, W, H, tw or W, th or H, nres, cb, coder, sop, eph, MallatOracle(orc), t2ref, **kw)


def decoded_tiles(orc, want, Cn, nres, cb, coder):
    """what the block decoder gives back per tile, int32 [C, h, w]: the MQ coder's coefficients; for HT the oracle's own decode (one row in four)"""
    return [np.stack(orc.decode_tile_blocks(want[t]["bytes"], want[t]["lens"], want[t]["numbps"], Cn, want[t]["w"], want[t]["h"], nres, cb, cb, coder, 1))
            for t in sorted(want)]


def stream_bytes(orc, tiles, nres, cb, coder):
    """bytes the block coder makes of coefficient tiles (closed-loop windows)"""
    return sum(len(orc.encode_tile_blocks([p for p in t], t.shape[2], t.shape[1], nres, cb, cb, coder, windows=1)[0]) for t in tiles)


def box_mean(frm, r):
    """the 2^r x 2^r box mean of int [C, H, W], edge-replicated: float64 [C, ceil(H / 2^r), ceil(W / 2^r)]"""
    C, H, W = frm.shape
    k = 1 << r
    Hp, Wp = shr(H, r) * k, shr(W, r) * k
    f = np.pad(frm.astype(np.float64), ((0, 0), (0, Hp - H), (0, Wp - W)), mode="edge")
    return f.reshape(C, Hp // k, k, Wp // k, k).mean(axis=(2, 4))


# ---- the cases of the issue -------------------------------------------------------------------------------------------------------------------
# lossless: (W, H, components, precision, tile, resolutions)
LOSSLESS = (
    (130, 70, 3, 8, (0, 0), 4),        # CPL 2 strip seam at column 126; 7 bands; odd 65 x 35 level 1 with the LL / H boundary inside a lane; RCT triple
    (260, 44, 3, 8, (128, 32), 4),     # tile grid; edge tiles 4 columns wide and 12 rows high; admissible reduce up to 3
    (5, 3, 1, 8, (0, 0), 4),           # levels 3 x 2, 2 x 1, 1 x 1: h < 2 / w < 2 levels pass LL through
    (256, 12, 4, 8, (0, 0), 3),        # CPL 4, seam at 252, the vector path (w_0 % 4 == 0), the fourth component as its own plane
    (520, 10, 1, 16, (0, 0), 2),       # CPL 8, seam at 504, second strip 16 columns wide
    (258, 10, 1, 8, (0, 0), 3),        # w_0 % 4 != 0: the scalar fallback
    (200, 150, 3, 8, (64, 64), 6),     # five levels in a 64 x 64 tile, edge tiles 8 x 22
)
# lossy: (W, H, components, precision, tile, resolutions, Quality)
LOSSY = (
    (130, 70, 3, 8, (0, 0), 4, 75),
    (96, 70, 1, 16, (0, 0), 6, 50),
    (200, 150, 4, 8, (64, 64), 4, 2),
)
PICTURES = ((130, 70, (0, 0), 4), (260, 44, (128, 32), 4), (200, 150, (64, 64), 6))     # closed_loop_ref.frame(W, H, 3, 16)
PICTURE_BOUND = 32
PIX_FORMAT = {(1, 8): 0, (1, 16): 1, (3, 8): 2, (3, 16): 3, (4, 8): 4, (4, 16): 5}      # J2K_PIX_GRAY8 ... (components, precision)


def case_id(c):
    return "%dx%dx%d-p%d-t%dx%d-r%d" % (c[0], c[1], c[2], c[3], c[4][0], c[4][1], c[5]) + ("-q%d" % c[6] if len(c) > 6 else "")


def level_seams(w, h, nres):
    """columns w_{l+1} and rows h_{l+1} of every level of a w x h tile: where LL ends"""
    d = dims(w, h, levels_of(nres))[1:]
    return sorted({x for x, _ in d if x < w}), sorted({y for _, y in d if y < h})


def seam_map(W, H, tile, nres):
    """lossless53_cases.int_frame's `seam`: per tile origin the strip seams of the general kernels (lossless53_cases.STRIP_BASES) and its band
    rows, plus column w_{l+1} / row h_{l+1} of every level"""
    band = 2 * ll.defaults()["band_prows"]
    out = {}
    for x0, y0, w, h in ll.tiles_of(W, H, tile):
        cols, rows = level_seams(w, h, nres)
        cols = set(cols) | {b + d for b in ll.STRIP_BASES for d in (-1, 0) if 0 <= b + d < w}
        rows = set(rows) | {r + d for r in range(band, h, band) for d in (-1, 0)}
        out[(x0, y0)] = (tuple(sorted(cols)), tuple(sorted(rows)))
    return out


def lossless_frame(case, family, seed=0):
    W, H, Cn, prec, tile, nres = case
    return ll.int_frame(family, W, H, Cn, prec, seed, tile, seam_map(W, H, tile, nres))


# the two frames whose Mallat tile-parts are pinned by digest (tests/golden/closed_loop_mallat_v1.json)
GOLDEN_CASES = [
    dict(name="mallat_mq_130x70", W=130, H=70, tile=(0, 0), cb=64, nres=4, coder=0, sop=False, eph=False, seed=301, noise=16),
    dict(name="mallat_ht_260x44_tiled_sop_eph", W=260, H=44, tile=(128, 32), cb=64, nres=4, coder=1, sop=True, eph=True, seed=302, noise=16),
]
GOLDEN_FILE = "closed_loop_mallat_v1.json"


def golden_stream(case, orc, t2ref):
    frm = ref.frame(case["W"], case["H"], case["seed"], noise=case["noise"])
    want = oracle_frame(frm, case["W"], case["H"], case["tile"][0], case["tile"][1], case["nres"], case["cb"], case["coder"], case["sop"], case["eph"], orc, t2ref)
    return frm, want, b"".join(want[t]["part"] for t in sorted(want))
