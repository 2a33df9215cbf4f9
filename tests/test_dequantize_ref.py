"""CPU: the yardstick of tests/dequantize_cases.py checked on its own, by the oracle alone -- before tests/test_gpu_dequantize.py holds the
device against it."""
import numpy as np
import pytest

import dequantize_cases as dq
import lossy97_cases as lc


def _coefs(C, w, h, family="noise", seed=0):
    return np.stack([lc.coeff_plane(family, w, h, seed + c) for c in range(C)])


@pytest.mark.parametrize("C,w,h,prec,nres", [(3, 24, 10, 8, 3), (1, 37, 21, 12, 6), (4, 16, 9, 16, 2), (3, 130, 17, 8, 1)])
def test_without_the_product_it_is_the_plain_expectation(oracle, C, w, h, prec, nres):
    for family in lc.COEFF_FAMILIES:
        if family == "outrange" and h < lc.OUTRANGE_MIN_H:
            continue
        coefs = _coefs(C, w, h, family, 3)
        assert np.array_equal(dq.expect_dequantized(oracle, coefs, prec, nres, 75, multiply=False), lc.expect_inverse(oracle, coefs, prec, nres)), family
        # ... which is lossy97_cases.inverse_counts, the composition the expectation restates, rows that leave int32 included
        out, _ = lc.inverse_counts(oracle, coefs, prec, nres)
        assert np.array_equal(dq.expect_dequantized(oracle, coefs, prec, nres, 75, multiply=False), out), family


@pytest.mark.parametrize("C,w,h,prec,nres", [(3, 24, 10, 8, 3), (1, 37, 21, 12, 6)])
def test_quality_one_is_the_same_bits_and_quality_75_is_not(oracle, C, w, h, prec, nres):
    coefs = _coefs(C, w, h, "noise", 5)
    plain = lc.expect_inverse(oracle, coefs, prec, nres)
    assert dq.step_of(1) == 1.0 and dq.step_of(0) == 1.0 / 100.0 and dq.step_of(-3) == 0.01
    assert np.array_equal(dq.expect_dequantized(oracle, coefs, prec, nres, 1), plain)
    assert not np.array_equal(dq.expect_dequantized(oracle, coefs, prec, nres, 75), plain)
    # multiplying by 1.0 / 75 is not dividing by 75: the products differ in the last place for some of these integers
    v = coefs[0].astype(np.float64)
    assert np.count_nonzero(v * dq.step_of(75) != v / 75.0) > 0


@pytest.mark.parametrize("i", range(len(dq.FRAMES)), ids=[dq.frame_id(f) for f in dq.FRAMES])
def test_the_nine_frames_reconstruct(oracle, i):
    """source -> encoder.preprocess at Quality -> the decode side with the product, per tile, by the oracle alone.  Max abs error / PSNR
    dequantised, and max abs error of the plain decode clamped to the sample range as decoder.createImage clamps it (recomputed on the CPU,
    dequantize_cases.source_frame: closed_loop_ref.frame_n, seeds 1000 ... 1008):

        200x150  3 x  8 bit  tiles 64x64   4 res  Q 75    5   41.5 dB    127
        200x150  3 x  8 bit  tiles 64x64   4 res  Q  2    7   41.5 dB     66
        200x150  3 x  8 bit  tiles 64x64   4 res  Q  1    9   40.9 dB      9   (identical bits)
        200x150  1 x  8 bit  tiles 64x64   4 res  Q 75    1   51.1 dB    126
        200x150  4 x  8 bit  tiles 64x64   4 res  Q 75    5   42.6 dB    127
         96x70   3 x 12 bit  tiles 64x64   6 res  Q 75    5   65.6 dB   2021
         96x70   3 x 16 bit  tiles 32xH    3 res  Q 75    6   89.4 dB  32328
         96x70   1 x 16 bit  untiled       6 res  Q 50    1   99.3 dB  32101
         96x70   4 x 16 bit  tiles 64x64   6 res  Q  2    7   90.4 dB  16383

    The bound of 16 is about twice the largest of these: the residual is the reference's ICT constants and roundings."""
    f = dq.FRAMES[i]
    prec, q = f[3], f[6]
    frm = dq.source_frame(f, i)
    top = (1 << prec) - 1
    got = dq.reconstruct(oracle, frm, f, True)
    plain = np.clip(dq.reconstruct(oracle, frm, f, False).astype(np.int64), 0, top)
    err = int(np.abs(got.astype(np.int64) - frm).max())
    err_plain = int(np.abs(plain - frm).max())
    print("%s: max abs err %d, PSNR %.1f dB; plain, clamped: %d" % (dq.frame_id(f), err, dq.psnr(got, frm, prec), err_plain))
    assert err <= dq.MAX_ERR
    if q >= 2:
        assert err_plain >= dq.MIN_ERR_PLAIN
    else:
        assert np.array_equal(got, dq.reconstruct(oracle, frm, f, False))


def _go_int32_scalar(v):
    import math
    if math.isnan(v) or not (-2147483649.0 < v < 2147483648.0):
        return -2 ** 31
    return int(math.trunc(v))


@pytest.mark.parametrize("step", dq.UNIT_STEPS)
def test_quantize_and_dequantize_restated(step):
    """the numpy restatements against dwt.go:500-520 read one value at a time with math.floor / math.ceil"""
    import math
    for n in dq.UNIT_LENGTHS:
        x = dq.quantize_input(n, step, 1)
        assert x.shape == (n,)
        got = dq.quantize_ref(x, step)
        assert got.dtype == np.int32 and got.shape == (n,)
        inv = 1.0 / step
        for k in list(range(min(n, 40))) + list(range(max(n - 40, 0), n)):
            v = float(x[k])
            r = v * inv + 0.5 if v >= 0 else v * inv - 0.5
            if math.isnan(r) or math.isinf(r):
                want = -2 ** 31
            else:
                want = _go_int32_scalar(float(math.floor(r)) if v >= 0 else float(math.ceil(r)))
            assert int(got[k]) == want, (n, k, v)
        y = dq.dequantize_input(n, 2)
        d = dq.dequantize_ref(y, step)
        assert d.dtype == np.float64 and all(float(d[k]) == float(int(y[k])) * step for k in range(min(n, 64)))
    big = dq.quantize_input(4099, step, 1)
    assert np.isnan(big).any() and np.isinf(big).any() and (np.signbit(big) & (big == 0)).any()
    # ties: +-x.5 round away from zero, -0.0 takes the Floor branch
    if step == 1.0:
        assert list(dq.quantize_ref(np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.0, 2147483647.4, 2147483647.5, -2147483648.5, -2147483649.5, np.nan, np.inf, -np.inf]), 1.0)) == \
            [1, -1, 2, -2, 3, -3, 0, 2147483647, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31]
    y = dq.dequantize_input(4099, 2)
    assert y[0] == -2 ** 31 and y[1] == 2 ** 31 - 1
