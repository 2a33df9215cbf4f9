"""numpy restatement of Go's image / image/color arithmetic behind the default branch of encoder.extractImageData
(encoder.go:178-195): r>>8, g>>8, b>>8 of At(x, y).RGBA() for *image.YCbCr, *image.CMYK, *image.Paletted (Go >= 1.8).
Used by the tests only.  Go's `/` truncates toward zero; numpy's `//` floors, so it is not used on signed values here."""
import numpy as np

# image.YCbCrSubsampleRatio -> (horizontal, vertical) chroma divisors
RATIO_DIV = {0: (1, 1), 1: (2, 1), 2: (2, 2), 3: (1, 2), 4: (4, 1), 5: (4, 2)}


def go_div(a, b):
    """Go's integer division (truncating toward zero), elementwise"""
    a = np.asarray(a, dtype=np.int64)
    q = np.abs(a) // b
    return np.where(a < 0, -q, q)


def ycbcr_rgba(Y, Cb, Cr):
    """color.YCbCr{Y, Cb, Cr}.RGBA() -> (r, g, b) 16-bit"""
    Y, Cb, Cr = (np.asarray(v, dtype=np.int64) for v in (Y, Cb, Cr))
    yy1 = Y * 0x10100
    cb1, cr1 = Cb - 128, Cr - 128
    out = []
    for v in (yy1 + 91881 * cr1, yy1 - 22554 * cb1 - 46802 * cr1, yy1 + 116130 * cb1):
        out.append(np.where(v < 0, 0, np.where(v > 0xFFFFFF, 0xFFFF, v >> 8)))
    return tuple(out)


def ycbcr_rgb8(Y, Cb, Cr):
    return tuple(v >> 8 for v in ycbcr_rgba(Y, Cb, Cr))


def cmyk_rgb8(C, M, Yc, K):
    C, M, Yc, K = (np.asarray(v, dtype=np.int64) for v in (C, M, Yc, K))
    w = 0xFFFF - K * 0x101
    return tuple((((0xFFFF - v * 0x101) * w) // 0xFFFF) >> 8 for v in (C, M, Yc))    # all non-negative: // is Go's /


def ycbcr_offsets(ratio, min_x, min_y, w, h, ystride, cstride):
    """(yi, ci) arrays of shape (h, w): image.YCbCr.YOffset / COffset for every pixel of the rectangle"""
    hd, vd = RATIO_DIV[ratio]
    y = np.arange(min_y, min_y + h, dtype=np.int64)[:, None]
    x = np.arange(min_x, min_x + w, dtype=np.int64)[None, :]
    yi = (y - min_y) * ystride + (x - min_x)
    ci = (go_div(y, vd) - go_div(min_y, vd)) * cstride + (go_div(x, hd) - go_div(min_x, hd))
    return yi, ci


def ycbcr_image_rgb(y, cb, cr, ystride, cstride, ratio, rect):
    """uint8 (h, w, 3) of an image.YCbCr"""
    x0, y0, x1, y1 = rect
    yi, ci = ycbcr_offsets(ratio, x0, y0, x1 - x0, y1 - y0, ystride, cstride)
    r, g, b = ycbcr_rgb8(np.asarray(y)[yi], np.asarray(cb)[ci], np.asarray(cr)[ci])
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def cmyk_image_rgb(pix, stride, rect):
    x0, y0, x1, y1 = rect
    w, h = x1 - x0, y1 - y0
    o = np.arange(h, dtype=np.int64)[:, None] * stride + 4 * np.arange(w, dtype=np.int64)[None, :]
    pix = np.asarray(pix)
    r, g, b = cmyk_rgb8(pix[o], pix[o + 1], pix[o + 2], pix[o + 3])
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def paletted_image_rgb(pix, stride, rect, palette):
    x0, y0, x1, y1 = rect
    w, h = x1 - x0, y1 - y0
    o = np.arange(h, dtype=np.int64)[:, None] * stride + np.arange(w, dtype=np.int64)[None, :]
    return np.asarray(palette).reshape(-1, 3)[np.asarray(pix)[o]].astype(np.uint8)


def rgba8_frame(rgb):
    """packed image.RGBA Pix (h, w * 4) of (h, w, 3) colours, alpha 255"""
    h, w, _ = rgb.shape
    out = np.full((h, w, 4), 255, np.uint8)
    out[..., :3] = rgb
    return out.reshape(h, w * 4)


def random_ycbcr(rng, ratio, rect, pad=0):
    """Go-shaped buffers of an image.YCbCr (NewYCbCr's layout, + pad bytes per row): (y, cb, cr, ystride, cstride)"""
    x0, y0, x1, y1 = rect
    hd, vd = RATIO_DIV[ratio]
    w, h = x1 - x0, y1 - y0
    cw = int(go_div(x1 - 1, hd) - go_div(x0, hd)) + 1 if w else 0
    ch = int(go_div(y1 - 1, vd) - go_div(y0, vd)) + 1 if h else 0
    ystride, cstride = w + pad, cw + pad
    y = rng.integers(0, 256, size=h * ystride, dtype=np.uint8)
    cb = rng.integers(0, 256, size=ch * cstride, dtype=np.uint8)
    cr = rng.integers(0, 256, size=ch * cstride, dtype=np.uint8)
    return y, cb, cr, ystride, cstride
