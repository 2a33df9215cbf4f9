"""CPU: the default branch of encoder.extractImageData (encoder.go:178-195) for the image types Go's decoders return --
image.YCbCr, image.CMYK, image.Paletted.  The restatement in go_image_ref.py against the pins of Go's image/color, its offset
tables at odd and negative Rect.Min, and the host-only j2k_image_validate (INVALID_ARG / GO_PANIC) through ctypes; the header and
the binding declare the new entries."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "go-jpeg2000_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import go_image_ref as ref  # noqa: E402

NEW_ENTRIES = ["j2k_image_validate", "j2k_image_to_rgba8", "j2k_extract_image_planar", "j2k_plan_forward_image", "j2k_plan_image_fused",
               "j2k_plan_encode_frame_image", "j2k_encode_image_host"]


def test_ycbcr_pins():
    # Go's doc comment of color.YCbCr.RGBA: YCbCr{0x7f, 0x7f, 0x7f} -> 0x7e18, 0x808d, 0x7db9
    assert tuple(int(v) for v in ref.ycbcr_rgba(0x7f, 0x7f, 0x7f)) == (0x7e18, 0x808d, 0x7db9)
    assert tuple(int(v) for v in ref.ycbcr_rgb8(0x7f, 0x7f, 0x7f)) == (0x7e, 0x80, 0x7d)
    assert tuple(int(v) for v in ref.ycbcr_rgb8(0, 0, 0)) == (0, 135, 0)          # what TestEncode_GenericImage encodes
    assert tuple(int(v) for v in ref.ycbcr_rgb8(255, 128, 128)) == (255, 255, 255)
    assert int(ref.ycbcr_rgb8(255, 128, 255)[0]) == 255                            # the sum saturates
    assert int(ref.ycbcr_rgb8(0, 128, 0)[0]) == 0                                  # the sum is negative


def test_cmyk_pins():
    assert tuple(int(v) for v in ref.cmyk_rgb8(128, 0, 0, 64)) == (95, 191, 191)
    for c in (0, 77, 255):
        assert tuple(int(v) for v in ref.cmyk_rgb8(c, 255 - c, c, 255)) == (0, 0, 0)
    assert tuple(int(v) for v in ref.cmyk_rgb8(0, 0, 0, 0)) == (255, 255, 255)


def test_go_div_truncates():
    assert list(ref.go_div(np.array([-5, -4, -3, -1, 0, 1, 3, 5]), 2)) == [-2, -2, -1, 0, 0, 0, 1, 2]
    assert list(ref.go_div(np.array([-5, -4, -3, 3, 4]), 4)) == [-1, -1, 0, 0, 1]


@pytest.mark.parametrize("ratio", range(6))
@pytest.mark.parametrize("min_x,min_y", [(0, 0), (3, 5), (-3, -5), (-4, 2), (1, -1), (-7, -6)])
def test_ycbcr_offset_table(ratio, min_x, min_y):
    """image.YCbCr.COffset written out per pixel (Go's `/`) equals the table's, for every ratio at odd and negative Rect.Min;
    the table starts at 0 and reaches exactly the chroma extent random_ycbcr allocates"""
    w, h, ystride, cstride = 9, 7, 12, 10
    yi, ci = ref.ycbcr_offsets(ratio, min_x, min_y, w, h, ystride, cstride)
    hd, vd = ref.RATIO_DIV[ratio]

    def tdiv(a, b):                       # Go's `/` on one int
        q = abs(a) // b
        return -q if a < 0 else q
    for j in range(h):
        for i in range(w):
            x, y = min_x + i, min_y + j
            assert yi[j, i] == (y - min_y) * ystride + (x - min_x)
            assert ci[j, i] == (tdiv(y, vd) - tdiv(min_y, vd)) * cstride + (tdiv(x, hd) - tdiv(min_x, hd))
    assert ci.min() == 0 and yi.min() == 0
    rng = np.random.default_rng(ratio)
    y, cb, cr, ys, cs = ref.random_ycbcr(rng, ratio, (min_x, min_y, min_x + w, min_y + h))
    yi2, ci2 = ref.ycbcr_offsets(ratio, min_x, min_y, w, h, ys, cs)
    assert yi2.max() == y.size - 1 and ci2.max() == cb.size - 1 == cr.size - 1


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "go-jpeg2000_amd")])
    from j2kgfx import _lib
    return _lib


def _validate(img, w=-1, h=-1):
    from j2kgfx import pixels
    return pixels.validate_image(img, w, h)


def test_validate_ycbcr(lib):
    from j2kgfx.pixels import YCbCr
    rng = np.random.default_rng(1)
    for ratio in range(6):
        for rect in [(0, 0, 37, 11), (-3, -5, 34, 6), (1, 1, 2, 2)]:
            y, cb, cr, ys, cs = ref.random_ycbcr(rng, ratio, rect)
            assert _validate(YCbCr(y, cb, cr, ys, cs, ratio, rect)) == lib.OK
            w, h = rect[2] - rect[0], rect[3] - rect[1]
            assert _validate(YCbCr(y, cb, cr, ys, cs, ratio, rect), w, h) == lib.OK
            assert _validate(YCbCr(y, cb, cr, ys, cs, ratio, rect), w + 1, h) == lib.ERR_INVALID_ARG   # not the plan's dims
            assert _validate(YCbCr(y, cb[:-1], cr, ys, cs, ratio, rect)) == lib.ERR_GO_PANIC       # a short Cb slice
            assert _validate(YCbCr(y, cb, cr[:-1], ys, cs, ratio, rect)) == lib.ERR_GO_PANIC
            assert _validate(YCbCr(y[:-1], cb, cr, ys, cs, ratio, rect)) == lib.ERR_GO_PANIC
            assert _validate(YCbCr(y, cb, cr, w - 1, cs, ratio, rect)) == lib.ERR_INVALID_ARG      # stride shorter than a row
    y, cb, cr, ys, cs = ref.random_ycbcr(rng, 0, (0, 0, 8, 8))
    assert _validate(YCbCr(y, cb, cr, ys, cs, 6, (0, 0, 8, 8))) == lib.ERR_INVALID_ARG             # no such ratio
    assert _validate(YCbCr(y, cb, cr, ys, cs, -1, (0, 0, 8, 8))) == lib.ERR_INVALID_ARG
    bad = YCbCr(y, cb, cr, ys, cs, 0, (0, 0, 8, 8))
    bad.kind = 3                                                                                  # a J2K_PIX_* number, not a kind
    assert _validate(bad) == lib.ERR_INVALID_ARG


def test_validate_cmyk_paletted(lib):
    from j2kgfx.pixels import CMYK, Paletted
    pix = np.zeros(5 * 40, np.uint8)
    assert _validate(CMYK(pix, 40, (0, 0, 10, 5))) == lib.OK
    assert _validate(CMYK(pix, 39, (0, 0, 10, 5))) == lib.ERR_INVALID_ARG
    assert _validate(CMYK(pix[:-1], 40, (0, 0, 10, 5))) == lib.ERR_GO_PANIC
    idx = np.zeros(5 * 12, np.uint8)
    pal = np.zeros((4, 3), np.uint8)
    assert _validate(Paletted(idx, 12, (2, 3, 12, 8), pal)) == lib.OK
    assert _validate(Paletted(idx, 9, (2, 3, 12, 8), pal)) == lib.ERR_INVALID_ARG
    assert _validate(Paletted(idx[:-3], 12, (2, 3, 12, 8), pal)) == lib.ERR_GO_PANIC
    assert _validate(Paletted(idx, 12, (2, 3, 12, 8), np.zeros((0, 3), np.uint8))) == lib.ERR_GO_PANIC   # At returns nil
    assert _validate(Paletted(idx, 12, (2, 3, 12, 8), np.zeros((257, 3), np.uint8))) == lib.ERR_INVALID_ARG


def test_header_and_binding_declare_the_new_entries(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "j2kgfx.h")).read(), flags=re.S)
    L = lib.lib()
    for n in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n in lib.SYMBOLS and hasattr(L, n), n
    assert "typedef struct j2k_image" in txt and "J2K_IMG_YCBCR = 16" in txt
    import ctypes as C
    assert C.sizeof(lib.Image) == 112


# ---- image_color.h itself, on the host: the header the staged kernel (image.hip) and the fused 5-3 level-0 kernel share ----------------
HOST_TABLES = r"""
#include <stddef.h>
#include "image_color.h"
extern "C" void ycc_table(uint32_t *out) {          // entry i: Y = i & 255, Cb = (i >> 8) & 255, Cr = i >> 16
    for (uint32_t i = 0; i < (1u << 24); i++) out[i] = j2k::ycbcr_rgba8((int)(i & 255), (int)((i >> 8) & 255), (int)(i >> 16));
}
extern "C" void cmyk_table(const uint8_t *pix, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) out[i] = j2k::cmyk_rgba8(pix[4 * i], pix[4 * i + 1], pix[4 * i + 2], pix[4 * i + 3]);
}
extern "C" int divisors(int ratio) { return j2k::ycc_hdiv(ratio) * 16 + j2k::ycc_vdiv(ratio); }
"""


@pytest.fixture(scope="module")
def color_lib(tmp_path_factory):
    import ctypes as C
    import shutil
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, c++, g++, clang++) to compile image_color.h with")
    d = tmp_path_factory.mktemp("image_color")
    src, so = d / "tables.cpp", d / "libtables.so"
    src.write_text(HOST_TABLES)
    subprocess.check_call([cxx, "-O2", "-shared", "-fPIC", "-D__host__=", "-D__device__=", "-D__forceinline__=inline",
                           "-I", os.path.join(ROOT, "go-jpeg2000_amd", "csrc"), str(src), "-o", str(so)])
    return C.CDLL(str(so))


def test_image_color_header_every_ycbcr_triple(color_lib):
    """ycbcr_rgba8 of image_color.h, compiled for the host, on all 2^24 (Y, Cb, Cr) against ycbcr_rgb8 (the table the GPU test
    test_gpu_image_sources_edges.py::test_every_ycbcr_triple_and_the_grid_stride_tail puts through image.hip)"""
    import ctypes as C
    packed = ref.ycbcr_table()[3]
    got = np.zeros(1 << 24, np.uint32)
    color_lib.ycc_table(got.ctypes.data_as(C.c_void_p))
    assert np.array_equal(got, packed)
    assert int(got[0]) == 0xFF000000 | 135 << 8 and int(got[0x7f7f7f]) == 0xFF000000 | 0x7e | 0x80 << 8 | 0x7d << 16     # the pins above


def test_image_color_header_every_cmyk_value_pair(color_lib):
    """cmyk_rgba8 on the 256 x 256 table in which every channel meets every (value, K) pair, against cmyk_rgb8; the chroma divisors
    of the six ratios against RATIO_DIV"""
    import ctypes as C
    pix, packed = ref.cmyk_table()
    got = np.zeros(1 << 16, np.uint32)
    color_lib.cmyk_table(pix.ctypes.data_as(C.c_void_p), C.c_size_t(1 << 16), got.ctypes.data_as(C.c_void_p))
    assert np.array_equal(got.reshape(256, 256), packed)
    for ratio, (hd, vd) in ref.RATIO_DIV.items():
        assert color_lib.divisors(ratio) == hd * 16 + vd


def test_ycbcr_layout_restates_the_same_picture():
    """the layout helper of the GPU edge tests: one picture at Rect.Min (0,0) / (2,4) / (6,2), padded strides, views into larger buffers
    and re-randomised pad bytes is one set of colours by the restatement; random_ycbcr's layout is its default"""
    rng = np.random.default_rng(11)
    W, H = 24, 7
    for ratio in (0, 1, 2):
        cw, ch = ref.chroma_dims(ratio, (0, 0, W, H))
        content = tuple(rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((H, W), (ch, cw), (ch, cw)))
        want = ref.ycbcr_image_rgb(content[0].reshape(-1), content[1].reshape(-1), content[2].reshape(-1), W, cw, ratio, (0, 0, W, H))
        for mn, ypad, cpad, offs, cpad2 in [((0, 0), 0, 0, (0, 0, 0), None), ((2, 4), 8, 4, (16, 4, 8), None), ((6, 2), 16, 0, (0, 8, 0), None),
                                            ((0, 2), 0, 4, (0, 0, 0), 8)]:
            rect = (mn[0], mn[1], mn[0] + W, mn[1] + H)
            assert ref.chroma_dims(ratio, rect) == (cw, ch)
            cs2 = None if cpad2 is None else cw + cpad2
            bufs, spans, ys, cs = ref.ycbcr_layout(rng, ratio, rect, W + ypad, cw + cpad, offs, 5, cs2, content)
            planes = [b[s0:s1] for b, (s0, s1) in zip(bufs, spans)]
            assert [p.size for p in planes] == [H * ys, ch * cs, ch * (cs2 or cs)] and all(b.size == s1 + 5 for b, (_, s1) in zip(bufs, spans))
            assert np.array_equal(ref.ycbcr_image_rgb(*planes, ys, cs, ratio, rect, cs2), want)
            before = [p.copy() for p in planes]
            for p, st, row in zip(planes, (ys, cs, cs2 or cs), (W, cw, cw)):
                ref.rerandomise_pad(rng, p, st, row)
            assert np.array_equal(ref.ycbcr_image_rgb(*planes, ys, cs, ratio, rect, cs2), want)
            assert (ypad == 0) == np.array_equal(before[0], planes[0])          # the pad bytes did change, where there are any
            assert all(np.array_equal(b.reshape(-1, st)[:, :row], p.reshape(-1, st)[:, :row])
                       for b, p, st, row in zip(before, planes, (ys, cs, cs2 or cs), (W, cw, cw)))
