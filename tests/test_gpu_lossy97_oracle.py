"""GPU: every kernel form of the lossy 9-7 path against the C oracle, bit for bit (np.array_equal: the bar tests/test_gpu_dwt97.py states), on
the cases of tests/lossy97_cases.py -- coefficients the forward path never produced, every workgroup width, every Quality class, the shapes
at the strip / band / tile seams, contents that show a boundary mistake on its own row or column and the ends of int32 and float64.
tests/test_lossy97_cases.py checks the same lists on the CPU first.

Which test reaches which launcher branch (csrc/dwt97.hip, launch_dwt97_fwd / launch_dwt97_inv):

  launch_dwt97_fwd
    wg_waves 6 ... 16, quantiser ENCODER  (dwt97_fwd_rgb_wg_kernel<NW, Q_ENCODER, ., 0>, Markstein division)   test_forward_level0[nw6 ... nw16],
                                                                                                               test_forward_markstein_frames
    pix_stride > 0                        (<8, Q_ENCODER, ., 3>: packed RGBA8 pixels)                          test_forward_rgba8_pixels
    wg_waves, quantiser TCD / NONE        (<NW, Q_TCD / Q_NONE, ., 0>)             not reachable: the table needs the colour transform on an int32 frame
                                                                                   (S.mct); the plans of another quantiser are one-component host calls
    pwaves 8, float64 in, ENCODER         (<8, Q_ENCODER, 7, 1>: deeper levels)    test_forward_level0 (nres 3, 6, 1), test_planes_forward_inverse[wg8]
    pwaves 8, float64 in, TCD             (<8, Q_TCD, 7, 1>)                       test_tcd_apply_dwt[wg8] (levels 3: level 1 and 2)
    pwaves 8, float64 in, NONE            (<8, Q_NONE, 7, 1>)                      test_float_unit_calls[wg8]
    pwaves 8, int32 in, ENCODER           (<8, Q_ENCODER, 7, 2>: one component)    test_planes_forward_inverse[wg8] (gray, the fourth component)
    pwaves 8, int32 in, TCD               (<8, Q_TCD, 7, 2>)                       test_tcd_apply_dwt[wg8] (level 0)
    pwaves 8, int32 in, NONE              (<8, Q_NONE, 7, 2>)                      not reachable: an int32 frame without a quantiser is the 5-3 path
    dwt97_fwd_kernel<2, 3>                (RGB triple, marching)                   test_forward_level0[nw0] (strip seams of 124 columns)
    dwt97_fwd_kernel<4, 1>                (one plane of 192 columns and more)      test_float_unit_calls[wg0], test_tcd_apply_dwt[wg0], test_planes_forward_inverse[wg0]
    dwt97_fwd_kernel<2, 1>                (one plane below 192 columns)            the same three, and test_float_1d

  launch_dwt97_inv
    wg_waves 6 ... 12                     (dwt97_inv_rgb_wg_kernel<NW, ., false>, the wave-level redo)         test_inverse_level0[nw6 ... nw12]
    pix_stride > 0                        (<8, ., true>: packed RGBA8 pixels)                                  test_inverse_rgba8_pixels
    pwaves 8, int32 coefficients -> f64   (dwt97_inv_plane_wg_kernel<8, 6, false, false>: deeper levels)       test_inverse_level0 (nres 3, 6, 1), test_planes_forward_inverse[wg8]
    pwaves 8, int32 -> int32 frame        (<8, 6, false, true>: one component, tcd level 0)                    test_planes_forward_inverse[wg8], test_tcd_apply_dwt[wg8]
    pwaves 8, float64 -> float64          (<8, 6, true, false>)                                                test_float_unit_calls[wg8]
    pwaves 8, float64 -> int32            (<8, 6, true, true>)                     not reachable: float64 coefficients come with a float64 frame
    dwt97_inv_kernel<2, 3>, <4, 1>, <2, 1>                                         as the forward marching kernels, with test_inverse_level0[nw0]

Found by `overflow` (float64 unit calls only) and fixed with it: the kernels formed a mirrored edge term as c * (x + x) where the reference
has (2 * c) * x (dwt.go:171-197, 230-260).  The two are the same bits until x + x overflows: for |x| > DBL_MAX / 2 beside a mirrored edge the
reference stays finite and the kernels gave +-inf -- test_float_unit_calls[wg0-overflow] differed from the oracle on most of its shapes.  The
marching kernels and the float64 instantiations of the workgroup forms now take the reference's form at every mirrored position (lift97 in
csrc/dwt97.hip); samples that come from int32 cannot reach such values, and the int32 level-0 workgroup kernels are unchanged."""
import ctypes as C
import os

import numpy as np
import pytest

import lossy97_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx_for():
    """a context per knob setting, made once for the module (the knobs are read when a context is created)"""
    from j2kgfx import Context
    cache = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in cache:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update({k: str(v) for k, v in env.items()})
            try:
                cache[key] = Context(0)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return cache[key]

    yield get
    for c in cache.values():
        c.close()


def _nrs(case):
    return (case.nw - 3, lc.defaults()["band_prows_97"])


def _coefficient_sets(plan, case, family):
    """(flat coefficient buffer of the plan, {(tile, comp): plane}) of one family"""
    rows = plan.planes()
    buf = np.zeros(int(plan.info.coeff_elems), np.int32)
    per = {}
    for t, c, x0, y0, w, h, off in (tuple(int(v) for v in r) for r in rows):
        p = lc.coeff_plane(family, w, h, 3 * (x0 + y0) + c, _nrs(case))
        per[(t, c)] = p
        buf[off:off + w * h] = p.reshape(-1)
    return buf, per


def _expected_frame(oracle, plan, per, ncomp, prec, nres, W, H):
    rows = plan.planes()
    out = np.zeros((ncomp, H, W), np.int32)
    for t in np.unique(rows[:, 0]):
        x0, y0, w, h = (int(v) for v in rows[rows[:, 0] == t][0, 2:6])
        out[:, y0:y0 + h, x0:x0 + w] = lc.expect_inverse(oracle, np.stack([per[(int(t), c)] for c in range(ncomp)]), prec, nres)
    return out


def _check_forward(oracle, plan, frame, hc, ncomp, prec, nres, quality, what):
    rows = plan.planes()
    for t in np.unique(rows[:, 0]):
        sel = rows[rows[:, 0] == t]
        x0, y0, w, h = (int(v) for v in sel[0, 2:6])
        want = oracle.preprocess([np.ascontiguousarray(frame[c, y0:y0 + h, x0:x0 + w]) for c in range(ncomp)], w, h, prec, False, nres, quality)
        for row in sel:
            c, off = int(row[1]), int(row[6])
            assert np.array_equal(hc[off:off + w * h].reshape(h, w), want[c]), (what, "tile", int(t), "component", c)


@pytest.mark.parametrize("case", lc.inverse_cases(), ids=lambda c: c.id)
def test_inverse_level0(oracle, ctx_for, case):
    """ARBITRARY int32 coefficients -> frame, RGB + ICT: tcd.ApplyInverseDWT's int32(v + 0.5), InverseICT's, the DC shift -- the general kernel
    and every width of the workgroup form against the oracle's composition, `outrange` through Go's out-of-range conversion (the redo)"""
    import torch
    from j2kgfx.codec import FramePlan
    plan = FramePlan(case.W, case.H, 3, ctx=ctx_for(J2K_L0_WG97_INV=case.nw), precision=case.prec, lossless=False, quality=case.quality,
                     num_resolutions=case.nres, cb=(64, 64), tile=case.tile, coder=0)
    try:
        for family in case.families:
            buf, per = _coefficient_sets(plan, case, family)
            back = plan.inverse(torch.from_numpy(buf).to(plan.device))
            plan.ctx.sync()
            want = _expected_frame(oracle, plan, per, 3, case.prec, case.nres, case.W, case.H)
            assert np.array_equal(back.cpu().numpy(), want), family
    finally:
        plan.close()


@pytest.mark.parametrize("W,H,tile", [(512, 11, (0, 0)), (24, 10, (0, 0)), (280, 13, (256, 128)), (536, 25, (256, 22)), (248, 21, (0, 0)), (16, 2, (0, 0))])
@pytest.mark.parametrize("nres", [2, 6])
def test_inverse_rgba8_pixels(oracle, W, H, tile, nres):
    """the same coefficient sets straight to packed RGBA8 pixels (dwt97_inv_rgb_wg_kernel, PIX): decoder.createImage's clamp of the frame the
    oracle's composition gives"""
    import torch
    from j2kgfx.codec import FramePlan
    nw = lc.defaults()["l0_wg97_inv"]
    case = lc.Case(nw, W, H, tile, 8, nres, 75, lc.COEFF_FAMILIES)
    plan = FramePlan(W, H, 3, precision=8, lossless=False, quality=75, num_resolutions=nres, cb=(64, 64), tile=tile, coder=0)
    try:
        for family in lc.COEFF_FAMILIES:
            buf, per = _coefficient_sets(plan, case, family)
            out = torch.full((H, W * 4), 0x5A, dtype=torch.uint8, device=plan.device)
            assert plan.pixels_fused(2, out, inverse=True)                 # the kernel writes the pixels itself
            plan.inverse_pixels(torch.from_numpy(buf).to(plan.device), out)
            plan.ctx.sync()
            want = _expected_frame(oracle, plan, per, 3, 8, nres, W, H)
            assert np.array_equal(out.cpu().numpy(), oracle.create_image([p for p in want], 8)), family
    finally:
        plan.close()


@pytest.mark.parametrize("case", lc.forward_cases(), ids=lambda c: c.id)
def test_forward_level0(oracle, ctx_for, case):
    """frame -> quantised coefficients, RGB + ICT (encoder.preprocess): the general kernel and every width of the workgroup form against
    oracle.preprocess -- the Markstein division against the oracle's true one at every Quality class, cvt_go on `outrange`"""
    import torch
    from j2kgfx.codec import FramePlan
    plan = FramePlan(case.W, case.H, 3, ctx=ctx_for(J2K_L0_WG97=case.nw), precision=case.prec, lossless=False, quality=case.quality,
                     num_resolutions=case.nres, cb=(64, 64), tile=case.tile, coder=0)
    try:
        for family in case.families:
            frame = lc.int_frame(family, case.W, case.H, 3, case.prec, 1, _nrs(case))
            coeff = plan.forward(torch.from_numpy(frame).to(plan.device))
            plan.ctx.sync()
            _check_forward(oracle, plan, frame, coeff.cpu().numpy(), 3, case.prec, case.nres, case.quality, family)
    finally:
        plan.close()


@pytest.mark.parametrize("quality,seed", lc.MARKSTEIN_FRAMES)
@pytest.mark.parametrize("nw", [n for n in lc.FWD_WAVES if n], ids=lambda v: "nw%d" % v)
def test_forward_markstein_frames(oracle, ctx_for, nw, quality, seed):
    """the frames of lc.MARKSTEIN_FRAMES: one coefficient each on which the division's two correcting fma decide the integer"""
    import torch
    from j2kgfx.codec import FramePlan
    W, H, prec, nres = lc.MARKSTEIN_SHAPE
    plan = FramePlan(W, H, 3, ctx=ctx_for(J2K_L0_WG97=nw), precision=prec, lossless=False, quality=quality, num_resolutions=nres, cb=(64, 64),
                     tile=(0, 0), coder=0)
    try:
        frame = lc.markstein_frame(quality, seed)
        coeff = plan.forward(torch.from_numpy(frame).to(plan.device))
        plan.ctx.sync()
        _check_forward(oracle, plan, frame, coeff.cpu().numpy(), 3, prec, nres, quality, "markstein")
    finally:
        plan.close()


@pytest.mark.parametrize("quality", lc.QUALITIES)
def test_forward_rgba8_pixels(oracle, quality):
    """packed RGBA8 pixels -> quantised coefficients (dwt97_fwd_rgb_wg_kernel, SRC 3) at every Quality class: oracle.preprocess of
    extractImageData's planes; a ragged last tile column, halfH one past two bands"""
    import torch
    from j2kgfx.codec import FramePlan
    nr = lc.defaults()["l0_wg97"] - 3
    W, H, tile = 536, 4 * nr + 1, (256, 0)
    plan = FramePlan(W, H, 3, precision=8, lossless=False, quality=quality, num_resolutions=3, cb=(64, 64), tile=tile, coder=0)
    try:
        for family in ("noise", "step", "checker"):
            frame = lc.int_frame(family, W, H, 4, 8, quality)
            pix = np.ascontiguousarray(frame.transpose(1, 2, 0).astype(np.uint8).reshape(H, W * 4))
            dpix = torch.from_numpy(pix).to(plan.device)
            assert plan.pixels_fused(2, dpix)
            coeff = plan.forward_pixels(2, dpix)
            plan.ctx.sync()
            planes = np.stack(oracle.extract_image_data(pix, 2, W, H, 8))
            assert np.array_equal(planes, frame[:3])
            _check_forward(oracle, plan, planes, coeff.cpu().numpy(), 3, 8, 3, quality, family)
    finally:
        plan.close()


@pytest.mark.parametrize("W,H,Cn,tile,nres,prec,quality", lc.PLANE_FRAMES)
@pytest.mark.parametrize("wg", lc.PLANE_WAVES, ids=lambda v: "wg%d" % v)
def test_planes_forward_inverse(oracle, ctx_for, wg, W, H, Cn, tile, nres, prec, quality):
    """single components at level 0 (gray frames, the fourth component) and the deeper levels of every frame, marching kernels and workgroup
    form: coefficients == oracle.preprocess, and ARBITRARY coefficients (small, and with a row that leaves int32) back to the frame the
    oracle's composition gives.  RGB frames whose level-1 planes lie on both sides of the workgroup form's admission rule."""
    import torch
    from j2kgfx.codec import FramePlan
    plan = FramePlan(W, H, Cn, ctx=ctx_for(J2K_PLANE_WG97=wg), precision=prec, lossless=False, quality=quality, num_resolutions=nres, cb=(64, 64),
                     tile=tile, coder=0)
    case = lc.Case(lc.defaults()["plane_wg97"], W, H, tile, prec, nres, quality, ())
    try:
        for family in ("noise", "impulse", "step", "outrange"):
            frame = lc.int_frame(family, W, H, Cn, prec, 2, _nrs(case))
            coeff = plan.forward(torch.from_numpy(frame).to(plan.device))
            plan.ctx.sync()
            _check_forward(oracle, plan, frame, coeff.cpu().numpy(), Cn, prec, nres, quality, family)
        for family in lc.COEFF_FAMILIES:
            buf, per = _coefficient_sets(plan, case, family)
            back = plan.inverse(torch.from_numpy(buf).to(plan.device))
            plan.ctx.sync()
            assert np.array_equal(back.cpu().numpy(), _expected_frame(oracle, plan, per, Cn, prec, nres, W, H)), family
    finally:
        plan.close()


def _unit(fn, x, *a, ctx):
    y = np.array(x, np.float64)
    fn(y, *a, ctx=ctx)
    return y


@pytest.mark.parametrize("family", lc.FLOAT_FAMILIES)
@pytest.mark.parametrize("wg", lc.PLANE_WAVES, ids=lambda v: "wg%d" % v)
def test_float_unit_calls(oracle, ctx_for, wg, family):
    """dwt.Forward2D97 / Inverse2D97 / DecomposeMultiLevel97 / ReconstructMultiLevel97 (levels 1 and 3) on every marching-kernel and workgroup
    shape: bit patterns and NaN-ness equal to the oracle's -- subnormals, +-0.0, values near the top of the format, +-inf and inf - inf.
    The reference's round-trip tolerances (dwt_test.go) hold for `noise`."""
    from j2kgfx import dwt
    ctx = ctx_for(J2K_PLANE_WG97=wg)
    bad = []
    with np.errstate(all="ignore"):
        for w, h in lc.float_shapes():
            if wg and not (16 <= w <= 512 and w % 8 == 0 and h >= 2):
                continue                                        # the marching kernels in either context: run once, under wg0
            x = lc.float_plane(family, w, h)
            y = _unit(dwt.Forward2D97, x, w, h, ctx=ctx)
            ok = [lc.same_floats(y, oracle.fwd97_2d(x, w, h)),
                  lc.same_floats(_unit(dwt.Inverse2D97, x, w, h, ctx=ctx), oracle.inv97_2d(x, w, h)),
                  lc.same_floats(_unit(dwt.DecomposeMultiLevel97, x, w, h, 1, ctx=ctx), oracle.decompose97(x, w, h, 1)),
                  lc.same_floats(_unit(dwt.ReconstructMultiLevel97, x, w, h, 1, ctx=ctx), oracle.reconstruct97(x, w, h, 1)),
                  lc.same_floats(_unit(dwt.DecomposeMultiLevel97, x, w, h, 3, ctx=ctx), oracle.decompose97(x, w, h, 3)),
                  lc.same_floats(_unit(dwt.ReconstructMultiLevel97, x, w, h, 3, ctx=ctx), oracle.reconstruct97(x, w, h, 3))]
            if not all(ok):
                bad.append((w, h, ok))
            if family == "noise":
                z = _unit(dwt.Inverse2D97, y, w, h, ctx=ctx)
                assert np.max(np.abs(z - x)) < 1e-9
                d3 = _unit(dwt.DecomposeMultiLevel97, x, w, h, 3, ctx=ctx)
                assert np.max(np.abs(_unit(dwt.ReconstructMultiLevel97, d3, w, h, 3, ctx=ctx) - x)) < 1e-8
    assert not bad, "(w, h, [Forward2D97, Inverse2D97, Decompose 1, Reconstruct 1, Decompose 3, Reconstruct 3] equal to the oracle): %s" % bad


@pytest.mark.parametrize("family", lc.FLOAT_FAMILIES)
def test_float_1d(oracle, family):
    """dwt.Forward97 / Inverse97 at the strip seams of the marching kernel"""
    from j2kgfx import dwt
    bad = []
    with np.errstate(all="ignore"):
        for n in lc.LENGTHS_1D:
            x = lc.float_plane(family, n, 1)
            y = x.copy(); dwt.Forward97(y, n)
            z = x.copy(); dwt.Inverse97(z, n)
            if not (lc.same_floats(y, oracle.fwd97_1d(x)) and lc.same_floats(z, oracle.inv97_1d(x))):
                bad.append(n)
            if family == "noise":
                r = y.copy(); dwt.Inverse97(r, n)
                assert np.max(np.abs(r - x)) < 1e-10
    assert not bad, bad


@pytest.mark.parametrize("family", ["noise", "outrange"])
@pytest.mark.parametrize("wg", lc.PLANE_WAVES, ids=lambda v: "wg%d" % v)
def test_tcd_apply_dwt(oracle, ctx_for, wg, family):
    """tcd.TileEncoder.ApplyForwardDWT / TileDecoder.ApplyInverseDWT, 9-7 branch (tcd.go:520-532, 428-435), at the seam shapes: `noise`, and
    `outrange` planes on which int32(v +- 0.5) leaves int32 in both directions"""
    ctx = ctx_for(J2K_PLANE_WG97=wg)
    bad = []
    for i, (w, h) in enumerate(lc.float_shapes()):
        if wg and not (16 <= w <= 512 and w % 8 == 0 and h >= 2):
            continue
        levels = (1, 3)[i % 2]
        x = lc.int_frame(family, w, h, 1, 12, 3)[0] if family == "noise" else lc.coeff_plane("outrange", w, h, 4)
        if family == "noise":
            x = x - 2048
        y = np.ascontiguousarray(x.reshape(-1), np.int32).copy()
        ctx.check(ctx.L.j2k_tcd_apply_forward_dwt(ctx.h, y.ctypes.data_as(C.c_void_p), w, h, levels, 0))
        z = np.ascontiguousarray(x.reshape(-1), np.int32).copy()
        ctx.check(ctx.L.j2k_tcd_apply_inverse_dwt(ctx.h, z.ctypes.data_as(C.c_void_p), w, h, levels, 0))
        if not (np.array_equal(y.reshape(h, w), oracle.tcd_forward_dwt(x, w, h, levels, 0))
                and np.array_equal(z.reshape(h, w), oracle.tcd_inverse_dwt(x, w, h, levels, 0))):
            bad.append((w, h, levels))
    assert not bad, bad
