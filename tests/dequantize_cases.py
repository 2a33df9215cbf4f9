"""The yardstick for j2k_plan_set_dequantize and the unit calls j2k_quantize / j2k_dequantize, importable without a GPU:
tests/test_dequantize_ref.py checks it on the CPU, tests/test_gpu_dequantize.py holds the device against it bit for bit.

The expectation is lossy97_cases.inverse_counts with dwt.Dequantize (dwt.go:514-520) in front, built from the oracle's own entry points per
tile and component:

    coef.astype(float64) * step  ->  oracle.reconstruct97(., levels_of(nres))  ->  go_int32(f + 0.5)  ->  oracle.postprocess(planes, prec, False)

with step = 1.0 / float(Quality) (Quality <= 0: 100) -- the double the encoder divides by (encoder.go:265-269).  Multiplying, never dividing by
Quality: the two are not the same bits."""
import numpy as np

import closed_loop_ref as ref
import lossy97_cases as lc

TWO31 = lc.TWO31


def step_of(quality):
    return 1.0 / float(quality if quality > 0 else 100)


def expect_dequantized(oracle, coefs, prec, nres, quality, multiply=True, is_signed=False):
    """the decode side of one tile with the coefficients dequantised first: coefs int32 [C, h, w] -> frame int32 [C, h, w].
    multiply=False leaves the product out: tcd.ApplyInverseDWT as written (== lossy97_cases.expect_inverse)"""
    C, h, w = coefs.shape
    step = step_of(quality)
    planes = []
    for c in range(C):
        f = coefs[c].astype(np.float64)
        if multiply:
            f = f * step                                               # dwt.go:517
        f = oracle.reconstruct97(f, w, h, lc.levels_of(nres))
        planes.append(lc.go_int32(f + 0.5)[0])                         # tcd.go:433-435
    return np.stack(oracle.postprocess(planes, prec, False, is_signed=is_signed))


def expect_frame(oracle, coef_of_tile, Cn, W, H, tile, prec, nres, quality, multiply=True):
    """a whole frame: coef_of_tile(t, x0, y0, w, h) -> int32 [Cn, h, w] for every tile in the plan's order"""
    out = np.zeros((Cn, H, W), np.int32)
    for t, (x0, y0, w, h) in enumerate(lc.tiles_of(W, H, tile)):
        out[:, y0:y0 + h, x0:x0 + w] = expect_dequantized(oracle, coef_of_tile(t, x0, y0, w, h), prec, nres, quality, multiply)
    return out


# ---- the nine frames of the issue's table: (W, H, components, bits, tile, resolutions, Quality) -------------------------------------------------
# tile (32, 0): 32 columns x the full height; (0, 0): untiled
FRAMES = (
    (200, 150, 3, 8, (64, 64), 4, 75),
    (200, 150, 3, 8, (64, 64), 4, 2),
    (200, 150, 3, 8, (64, 64), 4, 1),
    (200, 150, 1, 8, (64, 64), 4, 75),
    (200, 150, 4, 8, (64, 64), 4, 75),
    (96, 70, 3, 12, (64, 64), 6, 75),
    (96, 70, 3, 16, (32, 0), 3, 75),
    (96, 70, 1, 16, (0, 0), 6, 50),
    (96, 70, 4, 16, (64, 64), 6, 2),
)
MAX_ERR = 16                 # about twice what the reference arithmetic gives on these frames (5 ... 9): a property of the oracle
MIN_ERR_PLAIN = 60           # without the product, Quality >= 2
FRAME_SEED = 1000


def frame_id(f):
    return "%dx%dx%d-p%d-t%dx%d-r%d-q%d" % (f[0], f[1], f[2], f[3], f[4][0], f[4][1], f[5], f[6])


def source_frame(f, i=0):
    W, H, Cn, prec = f[:4]
    return ref.frame_n(W, H, Cn, prec, FRAME_SEED + i)


def quantised_tiles(oracle, frm, W, H, tile, prec, nres, quality):
    """encoder.preprocess (ICT + 9-7 + the encoder's quantiser) per tile: a list of int32 [Cn, h, w] in the plan's order"""
    out = []
    for x0, y0, w, h in lc.tiles_of(W, H, tile):
        sub = [np.ascontiguousarray(frm[c, y0:y0 + h, x0:x0 + w]).astype(np.int32) for c in range(frm.shape[0])]
        out.append(np.stack(oracle.preprocess(sub, w, h, prec, False, nres, quality)))
    return out


def reconstruct(oracle, frm, f, multiply=True):
    """source frame -> quantised coefficients -> the decode side, by the oracle alone"""
    W, H, Cn, prec, tile, nres, q = f
    tiles = quantised_tiles(oracle, frm, W, H, tile, prec, nres, q)
    return expect_frame(oracle, lambda t, *_: tiles[t], Cn, W, H, tile, prec, nres, q, multiply)


def psnr(a, b, prec):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(((1 << prec) - 1) ** 2 / mse)


# ---- dwt.Quantize / dwt.Dequantize restated (dwt.go:500-520) --------------------------------------------------------------------------------------
UNIT_LENGTHS = (0, 1, 63, 64, 65, 4099)
UNIT_STEPS = (1.0 / 75.0, 1.0, 0.3, 1e-300)


def quantize_ref(data, step_size):
    """invStep = 1.0 / stepSize; v >= 0 (-0.0 included): int32(math.Floor(v*invStep + 0.5)), else int32(math.Ceil(v*invStep - 0.5)); NaN
    compares false and takes the Ceil branch; int32() is Go's (out of range and NaN: 0x80000000)"""
    v = np.asarray(data, np.float64)
    with np.errstate(all="ignore"):
        inv = np.float64(1.0) / np.float64(step_size)
        q = v * inv
        r = np.where(v >= 0, np.floor(q + 0.5), np.ceil(q - 0.5))
    return lc.go_int32(r)[0]


def dequantize_ref(data, step_size):
    with np.errstate(all="ignore"):
        return np.asarray(data, np.int32).astype(np.float64) * np.float64(step_size)


def quantize_input(n, step_size, seed=0):
    """float64 [n]: noise that quantises inside int32, then -- as far as n allows -- +-0.0, ties at +-x.5, the neighbours of +-2^31, +-inf, NaN"""
    rng = np.random.default_rng([seed, n, 5])
    step = np.float64(step_size)
    with np.errstate(all="ignore"):
        x = rng.uniform(-1e6, 1e6, n) * step
        k = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 1e6 + 0.5, -(1e6 + 0.5)]) * step
        e = np.array([TWO31 - 1.0, TWO31 - 0.5, TWO31 - 0.5000001, TWO31, -TWO31, -TWO31 - 0.5, -TWO31 - 0.4999999, -TWO31 - 1.0, -TWO31 - 2.0]) * step
    lit = np.concatenate([[0.0, -0.0], k, e, [np.inf, -np.inf, np.nan, 5e-324, -5e-324]])
    m = min(n, lit.size)
    if n >= 2 * lit.size:                      # behind a stretch of noise, so that they do not all sit in the first wavefront
        x[n - m:] = lit[:m]
    else:
        x[:m] = lit[:m]
    return x


def dequantize_input(n, seed=0):
    rng = np.random.default_rng([seed, n, 6])
    x = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int64)
    lit = [-2 ** 31, 2 ** 31 - 1, 0, -1, 1, 75, -75]
    m = min(n, len(lit))
    x[:m] = lit[:m]
    return x.astype(np.int32)
