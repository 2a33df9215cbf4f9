"""GPU: every kernel form of the lossless 5-3 path against the C oracle, bit for bit (integer lifting is exact: np.array_equal, no tolerance),
on the cases of tests/lossless53_cases.py -- the strip / band / link / tile seams of every job table, every context option of the 5-3 path,
contents that show a boundary mistake on its own row or column, all of int32, and for the inverse coefficient sets that no forward
transform produced (`pixelrange`: reconstructions that leave 0 ... 2^prec - 1, so the pixel writers' saturation is compared with
decoder.createImage).  tests/test_lossless53_cases.py checks the same lists on the CPU first.  No comparison here is device against device.

Which test reaches which launcher branch.  The labels are those of lossless53_cases.forms(); tests/test_lossless53_cases.py counts three
cases at least behind each (label, direction, int32 frame | unit call | packed format).  Ids are the first of each route.

  launch_dwt53_fwd / launch_dwt53_inv (csrc/dwt53.hip), the same branches in both directions unless a line says otherwise
    J2K_DISPATCH, !L.vec   dwt53_*_kernel<2, 1, false>             test_marching_planes[march1-1x2c1-t0x0-p8-r1-deep0-plane_wg0], test_host_unit_calls[wg0-*]
                           <2, 3, false>                           test_marching_rgb[march3-1x3c3-t0x0-p8-r3-deep0]
    vec, one plane         <2, 1, true> / <4, 1, true> / <8, 1, true>   test_marching_planes[march1-2x9c1-... / march1-192x9c1-... / march1-384x9c1-...], test_host_unit_calls[wg0-*]
    vec, RGB triple        <2, 3, true> / <4, 3, true> / <8, 3, true>   test_marching_rgb[march3-8x23c3-... / march3-192x25c3-... / march3-384x6c3-...]
    fwd_go / inv_go, pix_stride > 0   <8, 1, true, ., PIX> (Gray16)      test_packed_formats[packed-512x11c1-t0x0-p16-r1-gray16+0-plane_wg0]
                           <8, 3, true, ., PIX> (RGBA8)            test_rgba8_level0[rgba8-528x3c3-t512x0-p8-r2-rgba8+16-l0_wg0] (forward), [...-l0_wg_inv0] (inverse),
                                                                   test_packed_formats[packed-520x13c4-t0x0-p8-r0-nrgba8+32-pix_fuse1] (a plane above 512 columns)
    fwd_go PF = true       not reachable: no option sets j2k_ctx.fwd_pf (j2k_ctx.cpp ctx_options)
    pix_stride > 0 on another instantiation (hipErrorInvalidValue)   not reachable: pix_fusable admits a table only at cpl 8, vec
    L.pwaves > 0, int32    dwt53_*_plane_wg_kernel<4 | 8, 1, 0, false | true, 8>    test_plane_workgroup[pwg-16x11c1-...-plane_wg8, pwg-520x3c1-...-plane_wg4], test_host_unit_calls[wg4-*, wg8-*]
                           <4 | 8, 3, 0, false (5) | true (4 / 3)> (J2K_PLANE_WG3=1)  test_plane_workgroup[pwg-16x3c3-t0x0-p31-r6-deep0-plane_wg4-plane_wg31, pwg-520x16c3-...-plane_wg8-plane_wg31]
    L.pwaves, pixels       <4, 1, 1> Gray16 / <4, 1, 2> Gray8 / <4, 1, 3> a byte of NRGBA / <4, 1, 4> 16 bits of NRGBA64, single and multi
                                                                   test_packed_formats[packed-24x5c1-...-gray16+16-pix_fuse1, packed-16x4c1-...-gray8+0-pix_fuse1,
                                                                   packed-512x8c4-...-nrgba8+16-pix_fuse1, packed-528x5c4-...-nrgba64+16-pix_fuse1; multi: packed-520x...]
                           <4, 3, 4> RGBA64 triples                test_packed_formats[packed-504x7c3-t0x0-p16-r4-rgba64+0-pix_fuse1, packed-520x3c3-...-rgba64+32-pix_fuse1]
                           <8, 1, 1> Gray16 at eight waves         test_packed_formats[packed-24x13c1-t0x0-p16-r2-gray16+0-plane_wg8, packed-520x12c1-t0x0-p16-r6-gray16+0-plane_wg8]
    L.wg_waves (inverse)   dwt53_inv_rgba8_wg_kernel<4 | 8, 5 | 6 | 7>  test_rgba8_level0[rgba8-512x2c3-t0x0-p8-r1-rgba8+0, ...-l0_inv_wpe6, ...-l0_inv_wpe7, ...-l0_wg_invw0,
                                                                   ...-l0_inv_wpe6-l0_wg_invw8, ...-l0_inv_wpe7-l0_wg_invw8]
  fwd_wg_go
    dwt53_fwd_rgba8_wg_kernel<4 | 8, store 0 | 1 | 2 | 4, 6>       test_rgba8_level0[...-l0_wg4, ...-l0_store0, (default), ...-l0_store2, ...-l0_store4]
    dwt53_fwd_rgba8_wg2_kernel<8 | 10 | 16, 0 | 1, 5> + the rest   test_rgba8_level0[rgba8-528x13c3-...-l0_fuse8, rgba8-504x21c3-...-l0_fuse10, rgba8-536x45c3-...-l0_fuse16, rgba8-760x13c3-...-l0_fuse8-l0_store0]
    dwt53_fwd_ycc_wg_kernel                                        tests/test_gpu_image_sources_edges.py owns it
  launch_dwt53_tail_fwd / _inv                                     `tail` in every test (test_marching_planes[march1-1x2c1-...] is the first); J2K_DEEP=0 in test_tail_and_deep
  launch_dwt53_deep_fwd    deep, deep + mid, flat jobs             test_tail_and_deep[deep-264x40c3-...-deep_mid0-deep_mid_inv0-..., deep-512x66c1-...-deep_mid1-deep_mid_inv0-...]
  launch_dwt53_deep_inv    J2K_DEEP_MID_INV 0 / 1 (compact layout and not) / 2   test_tail_and_deep[deep-512x66c1-...-deep_mid1-deep_mid_inv0-..., deep-512x66c3-...-deep_mid_inv1-...,
                                                                   deep-528x40c3-t512x0-p12-r5-deep_mid1-deep_mid_inv1-... (a 16-column tile: odd h2), deep-512x66c1-...-deep_mid_inv2-...]
                           twelve planes at the default J2K_DEEP_MIN_PLANES   test_rgba8_level0[rgba8-1024x29c3-t512x15-p8-r4-rgba8+16]
  launch_dwt53_mega_fwd / _inv   job order 1 / 2, bands of 15 pair-rows, deep / mid / flat jobs   test_rgba8_level0[rgba8-1008x3c3-...-deep_min_planes1-mega1, rgba8-512x3c3-...-deep_min_planes1-mega2]
  not reachable by any option: j2k_ctx.xcd_map, cpl0, force_novec (no entry in ctx_options(); the scalar kernels are reached by geometry), the level-l0
    flat chunk of 65 pair-rows (the deep launch admits 256 rows: 64 at the most)

Each test can fail.  One deliberate arithmetic change per kernel form (never an address) in a scratch copy, built once, this file run once (the 784 cases it had
before six Gray16 cases at eight waves joined):
  marching forward, the link's finishing row takes d of its own band twice (dwt53.hip)      216 cases red, first test_marching_planes[march1-3x19c1-t0x0-p16-r3-deep0-plane_wg0]
  marching inverse, the last odd row predicts from a row below that does not exist          364, test_marching_planes[march1-1x2c1-t0x0-p8-r1-deep0-plane_wg0]
  plane workgroup forward, the strip seam's left high-pass value (MULTI)                     57, test_plane_workgroup[pwg-520x3c1-t0x0-p16-r2-deep0-plane_wg4]
  plane workgroup inverse, the mirrored neighbour of the last odd row + 1                   171, test_marching_rgb[march3-511x23c3-t0x0-p8-r6-deep0] (its deeper levels)
  RGBA8 workgroup forward, rounding constant 1 of the vertical update                       267, test_rgba8_level0[rgba8-512x2c3-t0x0-p8-r1-rgba8+0]
  RGBA8 workgroup inverse, red clamped to 254                                               251, test_rgba8_level0[rgba8-512x2c3-t0x0-p8-r1-rgba8+0]
  fused levels 0 + 1, rounding constant 1 of the level-1 vertical update                     34, test_rgba8_level0[rgba8-528x13c3-t512x0-p8-r3-rgba8+16-l0_fuse8]
  LDS tail (lds_inv_level), the mirrored neighbour of the last odd row + 1                  222, test_marching_planes[march1-6x9c1-t0x0-p12-r0-deep0-plane_wg0]
  deep forward, the streamed level's last odd row predicts from e + 1                        67, test_tail_and_deep[deep-264x40c3-t0x0-p12-r6-deep_mid0-deep_mid_inv0-deep_min_planes1]
  deep inverse, the same on the way back                                                     67, test_tail_and_deep[deep-264x40c3-t0x0-p12-r6-deep_mid0-deep_mid_inv0-deep_min_planes1]
  merged launch's level-0 bands (NW 16 only), rounding constant 1                            26, test_rgba8_level0[rgba8-1008x15c3-t504x0-p8-r5-rgba8+32-deep_min_planes1-mega1]
and the saturation of the other pixel writers, which `pixelrange` and `fullrange` coefficients reach (run on all 790 cases):
  plane workgroup writer, 8 bit clamped to 254 / 16 bit clamped from 1                      15 / 36, test_packed_formats[packed-16x4c1-t0x0-p8-r1-gray8+0-pix_fuse1] / [packed-24x5c1-t0x0-p16-r2-gray16+16-pix_fuse1]
  pixel-writing marching kernel, RGBA8 blue clamped to 254 / Gray16 odd samples from 1      36 / 4, test_rgba8_level0[rgba8-528x3c3-t512x0-p8-r2-rgba8+16-l0_wg0] / test_packed_formats[packed-512x11c1-t0x0-p16-r1-gray16+0-plane_wg0]
No change went unnoticed, so no case had to be added for one.  The unchanged library passes all 790 cases: the file found no kernel bug."""
import os

import numpy as np
import pytest

import lossless53_cases as lc

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


def _plan(case, ctx_for):
    from j2kgfx.codec import FramePlan
    return FramePlan(case.W, case.H, case.C, ctx=ctx_for(**dict(case.env)), precision=case.prec, lossless=True, num_resolutions=case.nres,
                     cb=(64, 64), tile=case.tile, coder=1)


def _tiles(plan):
    """[(tile, x0, y0, w, h, {component: coefficient offset})]"""
    rows = plan.planes()
    out = []
    for t in np.unique(rows[:, 0]):
        sel = rows[rows[:, 0] == t]
        x0, y0, w, h = (int(v) for v in sel[0, 2:6])
        out.append((int(t), x0, y0, w, h, {int(r[1]): int(r[6]) for r in sel}))
    return out


def _check_forward(oracle, plan, frame, hc, case, what):
    """the device's coefficients == encoder.preprocess of every tile's crop, per tile and component"""
    for t, x0, y0, w, h, offs in _tiles(plan):
        want = lc.expect_forward(oracle, frame[:, y0:y0 + h, x0:x0 + w], case.prec, case.nres)
        for c, off in offs.items():
            assert np.array_equal(hc[off:off + w * h].reshape(h, w), want[c]), (case.id, what, "tile", t, "component", c)


def _coefficient_sets(oracle, plan, case, family, seam):
    """(the plan's flat coefficient buffer filled with one family, the frame the oracle's decode side makes of it)"""
    buf = np.zeros(int(plan.info.coeff_elems), np.int32)
    want = np.zeros((case.C, case.H, case.W), np.int32)
    for t, x0, y0, w, h, offs in _tiles(plan):
        if family == "pixelrange":
            co = lc.pixelrange_set(w, h, case.C, case.prec, case.nres, x0 + y0)
        else:
            cols, rows = seam.get((x0, y0), ((), ()))
            co = np.stack([lc.coeff_plane(family, w, h, 3 * (x0 + y0) + c, cols, rows) for c in range(case.C)])
        for c, off in offs.items():
            buf[off:off + w * h] = co[c].reshape(-1)
        want[:, y0:y0 + h, x0:x0 + w] = lc.expect_inverse(oracle, co, case.prec, case.nres)
    return buf, want


def _frame_case(oracle, ctx_for, case, families=lc.FRAME_FAMILIES, cfamilies=lc.COEFF_FAMILIES):
    """j2k_plan_forward / j2k_plan_inverse on int32 frames: every family against encoder.preprocess, every coefficient family against the
    oracle's decode side"""
    import torch
    plan = _plan(case, ctx_for)
    seam = lc.seams(case.route)
    try:
        for family in families:
            frame = lc.int_frame(family, case.W, case.H, case.C, case.prec, 1, case.tile, seam)
            coeff = plan.forward(torch.from_numpy(frame).to(plan.device))
            plan.ctx.sync()
            _check_forward(oracle, plan, frame, coeff.cpu().numpy(), case, family)
        for family in cfamilies:
            buf, want = _coefficient_sets(oracle, plan, case, family, seam)
            back = plan.inverse(torch.from_numpy(buf).to(plan.device))
            plan.ctx.sync()
            assert np.array_equal(back.cpu().numpy(), want), (case.id, "inverse", family)
    finally:
        plan.close()


@pytest.mark.parametrize("case", lc.marching_plane_cases(), ids=lambda c: c.id)
def test_marching_planes(oracle, ctx_for, case):
    """one component on the marching kernels (J2K_PLANE_WG=0, J2K_DEEP=0): dwt53_fwd_kernel / dwt53_inv_kernel<2 | 4 | 8, 1, vec | scalar> at the
    strip advances of 126 / 252 / 504 columns, the pick_cpl thresholds, the band and link seams; the LDS tail below them"""
    _frame_case(oracle, ctx_for, case)


@pytest.mark.parametrize("case", lc.marching_rgb_cases(), ids=lambda c: c.id)
def test_marching_rgb(oracle, ctx_for, case):
    """RGB triples with the RCT and the DC shift in the level-0 kernel (<cpl, 3, vec | scalar>), precisions 8 / 12 / 16 / 31; four components:
    the single-plane table beside the triples'"""
    _frame_case(oracle, ctx_for, case)


@pytest.mark.parametrize("case", lc.plane_wg_cases(), ids=lambda c: c.id)
def test_plane_workgroup(oracle, ctx_for, case):
    """dwt53_fwd_plane_wg_kernel / dwt53_inv_plane_wg_kernel<4 | 8, 1 | 3, 0, single | multi> around their bands of NW - 1 pair-rows"""
    big = case.W * case.H > 100000
    _frame_case(oracle, ctx_for, case, ("noise", "fullrange", "impulse") if big else lc.FRAME_FAMILIES, ("noise", "fullrange") if big else lc.COEFF_FAMILIES)


@pytest.mark.parametrize("case", lc.tail_deep_cases(), ids=lambda c: c.id)
def test_tail_and_deep(oracle, ctx_for, case):
    """the LDS tail (J2K_DEEP=0) and the deep launch (deep / mid / flat jobs; J2K_DEEP_MID 0 / 1, J2K_DEEP_MID_INV 0 / 1 / 2), one and three
    components: each forward and each inverse on arbitrary coefficients"""
    _frame_case(oracle, ctx_for, case, ("noise", "fullrange", "impulse", "step"), lc.COEFF_FAMILIES)


def _pixel_case(oracle, ctx_for, case, families, cfamilies, rgba8_entry):
    """packed pixels in: the device's coefficients == encoder.preprocess of encoder.extractImageData's planes.  Arbitrary coefficients out:
    the device's pixels == decoder.createImage of the oracle's decode side; the bytes after every row keep their sentinel."""
    import torch
    plan = _plan(case, ctx_for)
    R = case.route
    seam = lc.seams(R)
    fmt, W, H = case.fmt, case.W, case.H
    bpp_out = (1 if case.C == 1 else 4) * (2 if case.prec > 8 else 1)
    try:
        probe = torch.zeros((H, case.stride), dtype=torch.uint8, device=plan.device)
        # the restated admission rule is what labels the case: the library's own answer must agree with it
        assert plan.pixels_fused(fmt, probe) == (lc.pix_fusable(R, lc.PIX_BPS[fmt], 1 if case.C == 1 else 4, case.stride, False, case.prec) is not None), case.id
        oprobe = torch.zeros((H, case.out_stride), dtype=torch.uint8, device=plan.device)
        assert plan.pixels_fused(fmt, oprobe, inverse=True) == (lc.pix_fusable(R, lc.PIX_BPS[fmt], 1 if case.C == 1 else 4, case.out_stride, True, case.prec) is not None), case.id
        for family in families:
            frame = lc.int_frame(family, W, H, 4, case.prec, 2, case.tile, seam)
            pix = lc.pack_pixels(fmt, frame, case.stride)
            dpix = torch.from_numpy(pix).to(plan.device)
            coeff = plan.forward_rgba8(dpix) if rgba8_entry else plan.forward_pixels(fmt, dpix)
            plan.ctx.sync()
            planes = np.stack(oracle.extract_image_data(pix, fmt, W, H, case.prec))
            _check_forward(oracle, plan, planes, coeff.cpu().numpy(), case, family)
            assert np.array_equal(dpix.cpu().numpy(), pix), (case.id, family, "the source pixels changed")
        for family in cfamilies:
            if family == "pixelrange" and not case.pixelrange:
                continue
            buf, want = _coefficient_sets(oracle, plan, case, family, seam)
            out = torch.full((H, case.out_stride), 0x5A, dtype=torch.uint8, device=plan.device)
            dbuf = torch.from_numpy(buf).to(plan.device)
            if rgba8_entry:
                plan.inverse_rgba8(dbuf, out)
            else:
                plan.inverse_pixels(dbuf, out)
            plan.ctx.sync()
            o = out.cpu().numpy()
            assert np.array_equal(o[:, :W * bpp_out], oracle.create_image([p for p in want], case.prec)), (case.id, "inverse", family)
            assert (o[:, W * bpp_out:] == 0x5A).all(), (case.id, family, "row padding written")
    finally:
        plan.close()


@pytest.mark.parametrize("case", lc.rgba8_cases(), ids=lambda c: c.id)
def test_rgba8_level0(oracle, ctx_for, case):
    """forward_rgba8 / inverse_rgba8 under J2K_L0_WG, J2K_L0_WG_INVW, J2K_L0_WG_INV, J2K_L0_INV_WPE, J2K_L0_STORE, J2K_L0_FUSE, J2K_MEGA: the
    RGBA8 workgroup kernels, the fused levels 0 + 1, the merged launches, the pixel-reading / -writing marching kernels; padded rows.  The
    inverse runs on `noise`, `fullrange` and `pixelrange` coefficients against create_image of the oracle's inverse."""
    _pixel_case(oracle, ctx_for, case, ("noise", "impulse", "step", "checker"), ("noise", "fullrange", "pixelrange"), True)


@pytest.mark.parametrize("case", lc.packed_cases(), ids=lambda c: c.id)
def test_packed_formats(oracle, ctx_for, case):
    """forward_pixels / inverse_pixels for image.Gray / Gray16 / RGBA / RGBA64 / NRGBA / NRGBA64 through J2K_PIX_FUSE 0 / 1 / 2: the plane
    workgroup kernels' SRC / DST 1 ... 4 and the pixel-reading / -writing marching kernels; the inverse on `pixelrange` sets"""
    _pixel_case(oracle, ctx_for, case, ("noise", "impulse", "step", "const"), ("noise", "fullrange", "pixelrange"), False)


def _unit(fn, x, *a, ctx):
    y = np.array(x, np.int32).reshape(-1).copy()
    fn(y, *a, ctx=ctx)
    return y


@pytest.mark.parametrize("family", ["noise", "fullrange"])
@pytest.mark.parametrize("wg", lc.UNIT_WAVES, ids=lambda v: "wg%d" % v)
def test_host_unit_calls(oracle, ctx_for, wg, family):
    """dwt.Forward2D53 / Inverse2D53 / DecomposeMultiLevel53 / ReconstructMultiLevel53 (levels 1 and 3) under J2K_PLANE_WG 0 / 4 / 8 on the
    marching and workgroup shapes: all equal to the oracle's, `fullrange` through Go's wrapping arithmetic"""
    from j2kgfx import dwt
    ctx = ctx_for(J2K_PLANE_WG=wg)
    bad = []
    for w, h in lc.unit_shapes(wg):
        x = lc.coeff_plane(family, w, h, 9)
        ok = [np.array_equal(_unit(dwt.Forward2D53, x, w, h, ctx=ctx).reshape(h, w), oracle.fwd53_2d(x, w, h)),
              np.array_equal(_unit(dwt.Inverse2D53, x, w, h, ctx=ctx).reshape(h, w), oracle.inv53_2d(x, w, h))]
        for lv in lc.UNIT_LEVELS:
            ok += [np.array_equal(_unit(dwt.DecomposeMultiLevel53, x, w, h, lv, ctx=ctx).reshape(h, w), oracle.decompose53(x, w, h, lv)),
                   np.array_equal(_unit(dwt.ReconstructMultiLevel53, x, w, h, lv, ctx=ctx).reshape(h, w), oracle.reconstruct53(x, w, h, lv))]
        if not all(ok):
            bad.append((w, h, ok))
    assert not bad, "(w, h, [Forward2D53, Inverse2D53, Decompose 1, Reconstruct 1, Decompose 3, Reconstruct 3] equal to the oracle): %s" % bad
