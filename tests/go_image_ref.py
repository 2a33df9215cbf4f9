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


def ycbcr_rgba(Y, Cb, Cr, dtype=np.int64):
    """color.YCbCr{Y, Cb, Cr}.RGBA() -> (r, g, b) 16-bit (every intermediate is below 2^26: dtype = np.int32 is enough, and faster
    on the 2^24-entry table)"""
    Y, Cb, Cr = (np.asarray(v, dtype=dtype) for v in (Y, Cb, Cr))
    yy1 = Y * 0x10100
    cb1, cr1 = Cb - 128, Cr - 128
    out = []
    for v in (yy1 + 91881 * cr1, yy1 - 22554 * cb1 - 46802 * cr1, yy1 + 116130 * cb1):
        out.append(np.where(v < 0, 0, np.where(v > 0xFFFFFF, 0xFFFF, v >> 8)))
    return tuple(out)


def ycbcr_rgb8(Y, Cb, Cr, dtype=np.int64):
    return tuple(v >> 8 for v in ycbcr_rgba(Y, Cb, Cr, dtype))


def pack_rgba8(r, g, b):
    """uint32 R | G << 8 | B << 16 | 0xFF << 24: one packed image.RGBA pixel as a little-endian word"""
    return (np.asarray(r).astype(np.uint32) | np.asarray(g).astype(np.uint32) << 8 | np.asarray(b).astype(np.uint32) << 16
            | np.uint32(0xFF000000))


def ycbcr_table():
    """every (Y, Cb, Cr): entry i < 2^24 has Y = i & 255, Cb = (i >> 8) & 255, Cr = i >> 16 -> (Y, Cb, Cr uint8 [2^24], packed
    RGBA8 uint32 [2^24] by ycbcr_rgb8)"""
    i = np.arange(1 << 24, dtype=np.int32)
    Y, Cb, Cr = i & 255, (i >> 8) & 255, i >> 16
    packed = pack_rgba8(*ycbcr_rgb8(Y, Cb, Cr, dtype=np.int32))
    return Y.astype(np.uint8), Cb.astype(np.uint8), Cr.astype(np.uint8), packed


def cmyk_table():
    """256 x 256 image.CMYK pixels: pixel (row k, column c) = (C, M, Y, K) = (c, c ^ 0x5a, 255 - c, k), so every channel meets
    every (value, K) pair -> (Pix uint8 [256 * 1024], packed RGBA8 uint32 [256, 256] by cmyk_rgb8)"""
    k, c = np.mgrid[0:256, 0:256]
    pix = np.stack([c, c ^ 0x5A, 255 - c, k], axis=-1).astype(np.uint8)
    return pix.reshape(-1), pack_rgba8(*cmyk_rgb8(pix[..., 0], pix[..., 1], pix[..., 2], pix[..., 3]))


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


def ycbcr_image_rgb(y, cb, cr, ystride, cstride, ratio, rect, cstride2=None):
    """uint8 (h, w, 3) of an image.YCbCr (cstride2: a Cr stride other than Cb's, which the library's descriptor can say)"""
    x0, y0, x1, y1 = rect
    yi, ci = ycbcr_offsets(ratio, x0, y0, x1 - x0, y1 - y0, ystride, cstride)
    ci2 = ci if cstride2 is None else ycbcr_offsets(ratio, x0, y0, x1 - x0, y1 - y0, ystride, cstride2)[1]
    r, g, b = ycbcr_rgb8(np.asarray(y)[yi], np.asarray(cb)[ci], np.asarray(cr)[ci2])
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


def chroma_dims(ratio, rect):
    """(cw, ch): columns and rows of the chroma planes the rectangle reaches (image.NewYCbCr's, with Go's `/`)"""
    x0, y0, x1, y1 = rect
    hd, vd = RATIO_DIV[ratio]
    cw = int(go_div(x1 - 1, hd) - go_div(x0, hd)) + 1 if x1 > x0 else 0
    ch = int(go_div(y1 - 1, vd) - go_div(y0, vd)) + 1 if y1 > y0 else 0
    return cw, ch


def ycbcr_layout(rng, ratio, rect, ystride=None, cstride=None, offs=(0, 0, 0), slack=0, cstride2=None, content=None):
    """random_ycbcr with explicit strides, each plane at byte offset offs[k] of a larger buffer of its own with `slack` bytes behind
    the plane; everything random, pad bytes included.  Returns (bufs, spans, ystride, cstride): bufs[k] is the whole buffer, plane k
    is bufs[k][spans[k][0]:spans[k][1]] -- the same slice of a device copy of the buffer is the device plane.  cstride2: a Cr stride
    other than Cb's (Go has one CStride; the library's descriptor has a stride per plane).  content: (Y [h, w], Cb [ch, cw],
    Cr [ch, cw]) to put into the planes' pixel bytes, so that images of different layouts hold the same picture."""
    w, h = rect[2] - rect[0], rect[3] - rect[1]
    cw, ch = chroma_dims(ratio, rect)
    ystride = w if ystride is None else ystride
    cstride = cw if cstride is None else cstride
    strides = (ystride, cstride, cstride if cstride2 is None else cstride2)
    sizes = (h * strides[0], ch * strides[1], ch * strides[2])
    bufs = [rng.integers(0, 256, size=o + n + slack, dtype=np.uint8) for o, n in zip(offs, sizes)]
    spans = [(o, o + n) for o, n in zip(offs, sizes)]
    if content is not None:
        for b, (s0, s1), st, c in zip(bufs, spans, strides, content):
            c = np.asarray(c, dtype=np.uint8)
            b[s0:s1].reshape(-1, st)[:, :c.shape[1]] = c
    return bufs, spans, ystride, cstride


def rerandomise_pad(rng, plane, stride, row):
    """new random bytes in columns row .. stride - 1 of every row of `plane` (rows * stride bytes, modified in place): the bytes
    between the rows, which belong to no pixel"""
    if stride > row and plane.size:
        v = plane.reshape(-1, stride)
        v[:, row:] = rng.integers(0, 256, size=(v.shape[0], stride - row), dtype=np.uint8)


def random_ycbcr(rng, ratio, rect, pad=0):
    """Go-shaped buffers of an image.YCbCr (NewYCbCr's layout, + pad bytes per row): (y, cb, cr, ystride, cstride)"""
    w, h = rect[2] - rect[0], rect[3] - rect[1]
    cw, ch = chroma_dims(ratio, rect)
    ystride, cstride = w + pad, cw + pad
    y = rng.integers(0, 256, size=h * ystride, dtype=np.uint8)
    cb = rng.integers(0, 256, size=ch * cstride, dtype=np.uint8)
    cr = rng.integers(0, 256, size=ch * cstride, dtype=np.uint8)
    return y, cb, cr, ystride, cstride
