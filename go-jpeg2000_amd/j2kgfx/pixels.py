"""Pixel unpack / pack at native width -- mirror of the host loops on either side of the path:

    extract_image_data  <- encoder.extractImageData  (encoder.go:79-213, + the Options.Precision rescale)
    extract_image_planar <- its default branch (encoder.go:178-195) for YCbCr / CMYK / Paletted images
    create_image        <- decoder.createImage       (decoder.go:417-588)

Pixel buffers are Go image.* `Pix` layouts: numpy uint8 [h, stride] (16-bit samples big-endian)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PIX_GRAY8, PIX_GRAY16, PIX_RGBA8, PIX_RGBA64, PIX_NRGBA8, PIX_NRGBA64  # noqa: F401
from ._lib import YCBCR_444, YCBCR_422, YCBCR_420, YCBCR_440, YCBCR_411, YCBCR_410  # noqa: F401
from .context import default_context

_BPP = {PIX_GRAY8: 1, PIX_GRAY16: 2, PIX_RGBA8: 4, PIX_RGBA64: 8, PIX_NRGBA8: 4, PIX_NRGBA64: 8}


def components(fmt):
    return int(_lib.lib().j2k_pixels_components(int(fmt)))


def precision(fmt):
    return int(_lib.lib().j2k_pixels_precision(int(fmt)))


def extract_image_data(pix, fmt, w, h, target_precision=0, ctx=None):
    """pix: uint8 array of h rows x stride bytes.  Returns [component planes] (int32, h x w) like e.componentData."""
    ctx = ctx or default_context()
    pix = np.ascontiguousarray(pix, dtype=np.uint8).reshape(h, -1) if h else np.zeros((0, 0), np.uint8)
    stride = pix.shape[1] if h else w * _BPP[fmt]
    nc = components(fmt)
    planes = [np.zeros((h, w), dtype=np.int32) for _ in range(nc)]
    arr = (C.c_void_p * nc)(*[p.ctypes.data for p in planes])
    ctx.check(ctx.L.j2k_extract_image_data(ctx.h, int(fmt), pix.ctypes.data_as(C.c_void_p), C.c_size_t(stride), int(w), int(h),
                                           int(target_precision), arr))
    return planes


def create_image(planes, prec, stride=None, ctx=None):
    """planes: list of int32 [h, w] arrays.  Returns the uint8 Pix buffer [h, stride] createImage would fill."""
    ctx = ctx or default_context()
    nc = len(planes)
    h, w = planes[0].shape
    bpp = (1 if nc == 1 else 4) * (2 if prec > 8 else 1)
    stride = stride or w * bpp
    planes = [np.ascontiguousarray(p, dtype=np.int32) for p in planes]
    pix = np.zeros((h, stride), dtype=np.uint8)
    arr = (C.c_void_p * nc)(*[p.ctypes.data for p in planes])
    ctx.check(ctx.L.j2k_create_image(ctx.h, arr, nc, int(prec), int(w), int(h), pix.ctypes.data_as(C.c_void_p), C.c_size_t(stride)))
    return pix


# ---- what came out: squared error and PSNR of two DEVICE frames (j2k_pixels_sse) ---------------------------------------------
def sse(fmt, a, b, w, h, ctx=None):
    """a, b: torch uint8 [h, stride] on the context's device, the same Pix layout (strides may differ).  Returns numpy uint64 [channels as
    stored: 1 for the gray formats, 4 with alpha for the others]: the exact sum of squared sample differences of every channel.  The frames
    stay on the device; synchronises the context (what torch has queued on its current stream is waited for first)."""
    import torch
    ctx = ctx or default_context()
    assert a.dim() == 2 and b.dim() == 2 and a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.is_contiguous() and b.is_contiguous()
    if int(a.shape[0]) < int(h) or int(b.shape[0]) < int(h):
        raise _lib.J2KError(_lib.ERR_INVALID_ARG, "pixels.sse: fewer than h rows")
    nch = 1 if components(fmt) == 1 else 4
    sums = torch.zeros(4, dtype=torch.int64, device=a.device)
    torch.cuda.current_stream(a.device).synchronize()
    ctx.check(ctx.L.j2k_pixels_sse(ctx.h, int(fmt), C.c_void_p(a.data_ptr()), C.c_size_t(int(a.shape[1])), C.c_void_p(b.data_ptr()), C.c_size_t(int(b.shape[1])),
                                   int(w), int(h), C.c_void_p(sums.data_ptr())))
    ctx.sync()
    return sums.cpu().numpy().view(np.uint64)[:nch].copy()


def psnr(fmt, a, b, w, h, ctx=None):
    """10 log10(peak^2 * samples / squared error) of two device frames over the gray or the three colour channels (alpha is left out), peak =
    2^precision(fmt) - 1; inf for equal frames"""
    s = sse(fmt, a, b, w, h, ctx=ctx)
    nch = min(len(s), 3)
    total = int(s[:nch].astype(object).sum())
    if total == 0:
        return float("inf")
    peak = float((1 << precision(fmt)) - 1)
    return 10.0 * float(np.log10(peak * peak * float(int(w) * int(h) * nch) / float(total)))


# ---- the default branch (encoder.go:178-195): Go's *image.YCbCr, *image.CMYK, *image.Paletted by their fields -----------------
# Planes are 1-D uint8 buffers -- numpy arrays (host calls) or torch tensors (device calls) -- with Go's strides and lengths;
# rect = image.Rect(min_x, min_y, max_x, max_y).
def _ptr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _len(a):
    return int(a.numel()) if hasattr(a, "numel") else int(a.size)


class _GoImage:
    kind, ratio = 0, 0
    planes, strides, palette, npal = (), (), None, 0

    def struct(self):
        (x0, y0, x1, y1) = self.rect
        s = _lib.Image(kind=self.kind, ratio=self.ratio, min_x=x0, min_y=y0, width=x1 - x0, height=y1 - y0)
        for k, (a, st) in enumerate(zip(self.planes, self.strides)):
            s.plane[k], s.stride[k], s.len[k] = _ptr(a), int(st), _len(a)
        if self.palette is not None:
            s.palette, s.npal = (_ptr(self.palette) if _len(self.palette) else None), int(self.npal)
        return s

    @property
    def width(self):
        return self.rect[2] - self.rect[0]

    @property
    def height(self):
        return self.rect[3] - self.rect[1]

    def buffers(self):
        return [a for a in self.planes] + ([self.palette] if self.palette is not None else [])


class YCbCr(_GoImage):
    """image.YCbCr{Y, Cb, Cr, YStride, CStride, SubsampleRatio, Rect}"""
    kind = _lib.IMG_YCBCR

    def __init__(self, y, cb, cr, ystride, cstride, ratio, rect):
        self.planes, self.strides, self.ratio, self.rect = (y, cb, cr), (ystride, cstride, cstride), int(ratio), tuple(rect)


class CMYK(_GoImage):
    """image.CMYK{Pix, Stride, Rect}"""
    kind = _lib.IMG_CMYK

    def __init__(self, pix, stride, rect):
        self.planes, self.strides, self.rect = (pix,), (stride,), tuple(rect)


class Paletted(_GoImage):
    """image.Paletted{Pix, Stride, Rect, Palette}: palette = uint8 [npal, 3], Palette[i].RGBA() >> 8 (built by the caller)"""
    kind = _lib.IMG_PALETTED

    def __init__(self, pix, stride, rect, palette):
        self.planes, self.strides, self.rect = (pix,), (stride,), tuple(rect)
        self.palette = palette.reshape(-1) if palette is not None else palette
        self.npal = _len(self.palette) // 3 if palette is not None else 0


def validate_image(img, width=-1, height=-1):
    """j2k_image_validate: host only, no device (0, J2K_ERR_INVALID_ARG or J2K_ERR_GO_PANIC)"""
    s = img.struct()
    return int(_lib.lib().j2k_image_validate(C.byref(s), int(width), int(height)))


def extract_image_planar(img, target_precision=0, ctx=None):
    """the default branch of extractImageData for a HOST image (numpy planes): [3 int32 planes (h x w)]"""
    ctx = ctx or default_context()
    planes = [np.zeros((img.height, img.width), dtype=np.int32) for _ in range(3)]
    arr = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    s = img.struct()
    ctx.check(ctx.L.j2k_extract_image_planar(ctx.h, C.byref(s), int(target_precision), arr))
    return planes


def image_to_rgba8(img, pix=None, ctx=None):
    """a DEVICE image (torch planes) -> packed RGBA8 torch uint8 [h, w * 4] (alpha 255); synchronises the context"""
    import torch
    ctx = ctx or default_context()
    if pix is None:
        pix = torch.empty((img.height, img.width * 4), dtype=torch.uint8, device="cuda:%d" % ctx.device)
    torch.cuda.synchronize(ctx.device)
    s = img.struct()
    ctx.check(ctx.L.j2k_image_to_rgba8(ctx.h, C.byref(s), C.c_void_p(pix.data_ptr()), C.c_size_t(int(pix.shape[1]) if pix.dim() == 2 else img.width * 4)))
    ctx.sync()
    return pix
