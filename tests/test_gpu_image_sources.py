"""GPU: image.YCbCr / CMYK / Paletted sources (encoder.go:178-195, the default branch of extractImageData).  The branch makes
3 components at precision 8 from r>>8, g>>8, b>>8 of At(x, y).RGBA() -- exactly what image.RGBA gives with alpha ignored -- so
every call must equal, bit for bit, the J2K_PIX_RGBA8 call on the packed frame of the colours go_image_ref.py restates."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "go-jpeg2000_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import go_image_ref as ref  # noqa: E402


def _dev(a, device="cuda:0"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _ycbcr(rng, ratio, rect, pad=0, device=None):
    """(restated RGB (h, w, 3), image with numpy planes, image with device planes)"""
    from j2kgfx.pixels import YCbCr
    y, cb, cr, ys, cs = ref.random_ycbcr(rng, ratio, rect, pad)
    want = ref.ycbcr_image_rgb(y, cb, cr, ys, cs, ratio, rect)
    host = YCbCr(y, cb, cr, ys, cs, ratio, rect)
    return want, host, (YCbCr(_dev(y), _dev(cb), _dev(cr), ys, cs, ratio, rect) if device else None)


def _cmyk(rng, rect, pad=0):
    from j2kgfx.pixels import CMYK
    w, h = rect[2] - rect[0], rect[3] - rect[1]
    pix = rng.integers(0, 256, size=h * (4 * w + pad), dtype=np.uint8)
    return ref.cmyk_image_rgb(pix, 4 * w + pad, rect), CMYK(pix, 4 * w + pad, rect)


def _paletted(rng, rect, pad=0, npal=37):
    from j2kgfx.pixels import Paletted
    w, h = rect[2] - rect[0], rect[3] - rect[1]
    pix = rng.integers(0, npal, size=h * (w + pad), dtype=np.uint8)
    pal = rng.integers(0, 256, size=(npal, 3), dtype=np.uint8)
    return ref.paletted_image_rgb(pix, w + pad, rect, pal), Paletted(pix, w + pad, rect, pal)


def _to_dev(img):
    import copy
    d = copy.copy(img)
    d.planes = tuple(_dev(a) for a in img.planes)
    if img.palette is not None:
        d.palette = _dev(img.palette) if img.palette.size else img.palette
    return d


@pytest.mark.parametrize("w,h", [(1, 1), (37, 11), (513, 3)])
@pytest.mark.parametrize("mn", [(0, 0), (4, 2), (3, 5), (-3, -5), (-8, 1)])
def test_image_to_rgba8_equals_restatement(w, h, mn):
    from j2kgfx.pixels import image_to_rgba8
    rng = np.random.default_rng(abs(w * 7 + h + mn[0] * 3 + mn[1]))
    rect = (mn[0], mn[1], mn[0] + w, mn[1] + h)
    cases = [_ycbcr(rng, ratio, rect, pad)[:2] for ratio in range(6) for pad in (0, 5)]
    cases += [_cmyk(rng, rect, 0), _cmyk(rng, rect, 12), _paletted(rng, rect, 0), _paletted(rng, rect, 3, npal=256)]
    for want, img in cases:
        got = image_to_rgba8(_to_dev(img)).cpu().numpy()
        assert np.array_equal(got, ref.rgba8_frame(want)), (img.kind, img.ratio)


@pytest.mark.parametrize("target", [0, 8, 12, 16, 3])
def test_extract_image_planar_equals_oracle(target):
    import oracle as orc
    from j2kgfx import pixels
    rng = np.random.default_rng(target)
    for want, img in [_ycbcr(rng, 2, (-3, 1, 34, 12), 3)[:2], _ycbcr(rng, 5, (0, 0, 513, 3))[:2], _cmyk(rng, (1, 1, 38, 12), 4),
                      _paletted(rng, (0, 0, 37, 11), 2)]:
        got = pixels.extract_image_planar(img, target)
        w, h = img.width, img.height
        wanted = orc.extract_image_data(ref.rgba8_frame(want), 2, w, h, target)
        for g, wn in zip(got, wanted):
            assert np.array_equal(g, wn)


FWD_CASES = [  # W, H, tile, lossless, pix_fuse
    (3840, 2160, 512, True, 1), (3840, 2160, 512, True, 0), (3840, 2160, 512, False, 1), (3840, 2160, 0, True, 1),
    (1000, 600, 256, True, 1), (1000, 600, 256, False, 0)]


@pytest.mark.parametrize("W,H,tile,lossless,pix_fuse", FWD_CASES)
def test_forward_image_equals_forward_pixels(W, H, tile, lossless, pix_fuse):
    import torch
    from j2kgfx import Context
    from j2kgfx.codec import FramePlan
    ctx = Context(0)
    ctx.set_option("pix_fuse", pix_fuse)
    plan = FramePlan(W, H, 3, precision=8, lossless=lossless, quality=0 if lossless else 75, num_resolutions=6, cb=(64, 64),
                     tile=(tile, tile), coder=1, ctx=ctx)
    rng = np.random.default_rng(W + tile + pix_fuse)
    ratios = [2, 1, 0] if (W, tile, lossless) == (3840, 512, True) else [2]
    for ratio in ratios:
        want, _, dimg = _ycbcr(rng, ratio, (0, 0, W, H), device=True)
        fused = plan.image_fused(dimg)
        if (W, tile, lossless, pix_fuse) == (3840, 512, True, 1):
            assert fused                                     # 4:2:0, 4:2:2, 4:4:4 at 4K, 512 tiles, aligned planes
        if not lossless or pix_fuse == 0 or tile == 0:
            assert not fused
        if (W, tile, lossless, pix_fuse) == (1000, 256, True, 1):
            assert not fused                                 # no plane 384 columns wide: level 0 is not the workgroup kernel's (pick_cpl)
        ref_c = plan.forward_pixels(2, _dev(ref.rgba8_frame(want)))
        got = plan.forward_image(dimg)
        plan.ctx.sync()
        assert torch.equal(got, ref_c), ratio
    if (W, tile, lossless, pix_fuse) == (3840, 512, True, 1):
        want, _, dimg = _ycbcr(rng, 2, (1, 0, W + 1, H), device=True)   # odd Rect.Min.X: staged, same coefficients
        assert not plan.image_fused(dimg)
        ref_c = plan.forward_pixels(2, _dev(ref.rgba8_frame(want)))
        got = plan.forward_image(dimg)
        plan.ctx.sync()
        assert torch.equal(got, ref_c)
    plan.close()
    ctx.close()


@pytest.mark.parametrize("coder", [0, 1])
def test_encode_frame_image_closed_loop(coder):
    import torch
    from j2kgfx.codec import FramePlan
    W, H = 1024, 520
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=5, cb=(64, 64), tile=(512, 512), coder=coder, closed_loop=True)
    rng = np.random.default_rng(coder)
    imgs = [_ycbcr(rng, 2, (0, 0, W, H), device=True), _ycbcr(rng, 1, (2, 4, W + 2, H + 4), device=True)]
    want, himg = _paletted(rng, (0, 0, W, H))
    imgs.append((want, himg, _to_dev(himg)))
    assert plan.image_fused(imgs[0][2]) and plan.image_fused(imgs[1][2]) and not plan.image_fused(imgs[2][2])
    for want, _, dimg in imgs:
        out1, to1 = plan.encode_frame_pixels(2, _dev(ref.rgba8_frame(want)), sop=True, eph=True)
        plan.frame_status()
        n1 = int(to1[-1].item())
        out2, to2 = plan.encode_frame_image(dimg, sop=True, eph=True)
        plan.frame_status()
        n2 = int(to2[-1].item())
        assert n1 == n2 and torch.equal(out1[:n1], out2[:n2]) and torch.equal(to1, to2)
        if coder == 0:      # (the reference's HT decoder writes one row in four: an HT round trip is not the identity)
            back = torch.zeros((H, W * 4), dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(out2, n2, back, sop=True, eph=True)
            plan.frame_status()
            assert np.array_equal(back.cpu().numpy().reshape(H, W, 4)[..., :3], want)      # lossless: the restated colours


def test_encode_image_host_equals_encode_pixels_host():
    from j2kgfx.codec import FramePlan
    rng = np.random.default_rng(5)
    for closed in (False, True):
        W, H = 1000, 600
        plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=5, cb=(64, 64), tile=(256, 256), coder=1, closed_loop=closed)
        for want, img in [_ycbcr(rng, 2, (0, 0, W, H))[:2], _ycbcr(rng, 4, (-1, -1, W - 1, H - 1), 8)[:2], _cmyk(rng, (0, 0, W, H)),
                          _paletted(rng, (0, 0, W, H), 4)]:
            a = plan.encode_pixels_host(2, ref.rgba8_frame(want), sop=closed, eph=closed)
            b = plan.encode_image_host(img, sop=closed, eph=closed)
            for k in ("bytes", "tile_offs", "lens", "numbps"):
                assert np.array_equal(a[k], b[k]), k
        plan.close()


def test_errors_leave_output_untouched_and_context_usable():
    import torch
    from j2kgfx import J2KError, _lib
    from j2kgfx.codec import FramePlan
    from j2kgfx.pixels import Paletted
    W, H = 256, 64
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=4, cb=(32, 32), coder=1, closed_loop=True)
    rng = np.random.default_rng(9)
    pix = rng.integers(0, 8, size=W * H, dtype=np.uint8)
    pix[1234] = 8                                                       # one index past a palette of 8
    bad = Paletted(pix, W, (0, 0, W, H), rng.integers(0, 256, size=(8, 3), dtype=np.uint8))
    coeff = torch.full((int(plan.info.coeff_elems),), 77, dtype=torch.int32, device=plan.device)
    with pytest.raises(J2KError) as e:
        plan.forward_image(_to_dev(bad), coeff)
    assert e.value.status == _lib.ERR_GO_PANIC
    plan.ctx.sync()
    assert bool((coeff == 77).all())                                    # nothing written
    with pytest.raises(J2KError) as e:
        plan.encode_image_host(bad)
    assert e.value.status == _lib.ERR_GO_PANIC
    plan.encode_frame_image(_to_dev(bad))
    with pytest.raises(J2KError) as e:
        plan.frame_status()                                             # the asynchronous frame call reports it here
    assert e.value.status == _lib.ERR_GO_PANIC
    want, img = _paletted(rng, (0, 0, W, H), npal=9)
    gray = FramePlan(W, H, 1, precision=8, lossless=True, num_resolutions=4, cb=(32, 32), coder=1, ctx=plan.ctx)
    with pytest.raises(J2KError) as e:
        gray.forward_image(_to_dev(img))
    assert e.value.status == _lib.ERR_INVALID_ARG                      # a plan with ncomp != 3
    ref_c = plan.forward_pixels(2, _dev(ref.rgba8_frame(want)))         # the context still works
    got = plan.forward_image(_to_dev(img))
    plan.ctx.sync()
    assert torch.equal(got, ref_c)


def test_generic_image_case():
    """TestEncode_GenericImage (jpeg2000_test.go:738-751): an 8x8 all-zero image.YCbCr 4:4:4 encodes exactly like the RGBA8 frame of
    (0, 135, 0) -- lossless 5-3 and the reference's default lossy 9-7"""
    from j2kgfx import pixels
    from j2kgfx.codec import FramePlan
    z = np.zeros(64, np.uint8)
    img = pixels.YCbCr(z, z.copy(), z.copy(), 8, 8, 0, (0, 0, 8, 8))
    rgb = np.zeros((8, 8, 3), np.uint8)
    rgb[..., 1] = 135
    got = pixels.extract_image_planar(img)
    assert all(np.array_equal(g, rgb[..., c]) for c, g in enumerate(got))
    for lossless in (True, False):
        plan = FramePlan(8, 8, 3, precision=8, lossless=lossless, quality=0 if lossless else 75, num_resolutions=3, cb=(64, 64), coder=0)
        a = plan.encode_pixels_host(2, ref.rgba8_frame(rgb))
        b = plan.encode_image_host(img)
        assert np.array_equal(a["bytes"], b["bytes"]) and len(a["bytes"]) > 14
        plan.close()
