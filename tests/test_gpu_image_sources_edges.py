"""GPU: the YCbCr source of the 5-3 level-0 workgroup kernel (dwt53_fwd_ycc_wg_kernel, dwt53_l0pix_fwd_body.inc under J2K_L0_YCC), the host
predicate that chooses it (image_fusable, j2k_image.cpp) and the staged conversion (image.hip) at their edges.  Every comparison is bit for
bit: there is no tolerance in this file.  The expected coefficients are the ORACLE's (oracle.preprocess of the cropped planes of the colours
go_image_ref.py restates), the product's own forward_pixels comes second.

(1) the fused kernel over the boundary shapes, three ratios, layouts   (2) every condition of the predicate, one at a time
(3) the colour arithmetic, exhaustively                                (4) the closed-loop frame call against the oracle's tile-parts

Which plans fuse at all: the packed-RGBA8 level-0 workgroup kernel, whose second row source this is, is built only where level 0 runs at 8
columns per lane, i.e. where the WIDEST tile plane has at least 384 columns (pick_cpl, j2k_planbuild.cpp); every plane of the plan then takes
it, however narrow.  So the narrow planes of the sweep (16, 24, 40 ... columns) are the edge tiles of frames whose first tile is 384 wide."""
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
import closed_loop_ref as cl  # noqa: E402
import go_image_ref as ref  # noqa: E402


def _dev(a, device="cuda:0"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _tile(tile):
    return tile if isinstance(tile, tuple) else (tile, tile)


def _content(rng, ratio, W, H):
    """one picture: (Y [H, W], Cb [ch, cw], Cr [ch, cw]) of an image at an even Rect.Min"""
    cw, ch = ref.chroma_dims(ratio, (0, 0, W, H))
    return tuple(rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((H, W), (ch, cw), (ch, cw)))


class _Image:
    """an image.YCbCr in host buffers and on the device: planes are views at spans[k] of bufs[k] on either side"""

    def __init__(self, rng, ratio, W, H, mn=(0, 0), ypad=0, cpad=0, offs=(0, 0, 0), slack=0, cpad2=None, content=None):
        self.ratio, self.rect = ratio, (mn[0], mn[1], mn[0] + W, mn[1] + H)
        self.W, self.cw = W, ref.chroma_dims(ratio, self.rect)[0]
        self.cs2 = None if cpad2 is None else self.cw + cpad2
        self.bufs, self.spans, self.ys, self.cs = ref.ycbcr_layout(rng, ratio, self.rect, W + ypad, self.cw + cpad, offs, slack, self.cs2, content)

    def planes(self, bufs=None):
        return [b[s0:s1] for b, (s0, s1) in zip(bufs or self.bufs, self.spans)]

    def rgb(self):
        """the colours Go reads from it: uint8 (H, W, 3)"""
        return ref.ycbcr_image_rgb(*self.planes(), self.ys, self.cs, self.ratio, self.rect, self.cs2)

    def device(self):
        from j2kgfx.pixels import YCbCr
        dbufs = [_dev(b) for b in self.bufs]
        assert all(d.data_ptr() % 256 == 0 for d in dbufs)       # (the allocator's: a plane's alignment is its offset's)
        img = YCbCr(*self.planes(dbufs), self.ys, self.cs, self.ratio, self.rect)
        if self.cs2 is not None:
            img.strides = (self.ys, self.cs, self.cs2)
        return img

    def rerandomise_pads(self, rng):
        for p, st, row in zip(self.planes(), (self.ys, self.cs, self.cs2 or self.cs), (self.W, self.cw, self.cw)):
            ref.rerandomise_pad(rng, p, st, row)


def _oracle_coeff(orc, plan, rgb, nres, lossless=True, quality=0):
    """encoder.preprocess of every tile of the colours, by the oracle: [(offset, int32 [h * w])] in the plan's coefficient buffer"""
    out = []
    planes = plan.planes()
    for t in np.unique(planes[:, 0]):
        rows = planes[planes[:, 0] == t]
        x0, y0, w, h = (int(v) for v in rows[0, 2:6])
        crop = [rgb[y0:y0 + h, x0:x0 + w, c].astype(np.int32) for c in range(3)]
        want = orc.preprocess(crop, w, h, 8, lossless, nres, quality)
        out += [(int(row[6]), want[int(row[1])].reshape(-1)) for row in rows]
    return out


def _assert_coeff(coeff, expected, what=None):
    hc = coeff.cpu().numpy()
    for off, want in expected:
        assert np.array_equal(hc[off:off + want.size], want), (what, off)


# ---- (1) ------------------------------------------------------------------------------------------------------------------------------------------
# (W, H, tile): the small shapes at which the kernel can still go wrong.  Listed in the issue with planes narrower than 384 columns on their
# own -- (16,2) (16,6) (24,2) (24,3) (40,37) (64,114) (128,10) (256,110) untiled, (768,300) in 256 tiles, (512,150) in (256,75) tiles, (264,40)
# in 24 tiles -- which do NOT qualify at default options (see the module docstring: image_fused is false for them, as it is for the RGBA8
# frame).  Each is replaced by the nearest frame that does and still has that plane: the same plane as the EDGE tile behind one 384-column
# tile (W + 384, tile (384, 384)); (768,300) takes 384 tiles; the odd tile origin row and the x origin at 8 mod 16 keep their purpose with
# the smallest tile widths that qualify (384 and 392 = 8 mod 16).
SHAPES = [
    (400, 2, 384), (400, 6, 384), (408, 2, 384), (408, 3, 384), (424, 37, 384), (448, 114, 384), (512, 10, 384), (640, 110, 384),
    (496, 200, 0), (512, 4, 0), (512, 258, 0), (512, 511, 0), (768, 300, 384), (1280, 624, 512),
    (1040, 64, 512),            # edge tile 16 columns wide
    (640, 150, (384, 75)),      # tile origin row 75 is odd: under 4:2:0 rows 74 and 75 of different tiles share chroma row 37 (edge tiles 256 wide)
    (808, 40, 392),             # tile x origins 392 = 8 mod 16: gx >> 1 is 4 mod 8 (edge tile 24 wide, at 784)
]


@pytest.mark.parametrize("ratio", [0, 1, 2], ids=["444", "422", "420"])
@pytest.mark.parametrize("nres", [2, 4])
@pytest.mark.parametrize("W,H,tile", SHAPES)
def test_fused_kernel_shape_sweep_against_the_oracle(oracle, W, H, tile, nres, ratio):
    """dwt53_fwd_ycc_wg_kernel on every boundary shape: heights 2 and 3, odd heights (the last chroma row of 4:2:0 serves one luma row), the
    clamped halo rows of the first and the last band, planes of 16 / 24 / 40 / 64 columns, more than one band (7 pair-rows each), tiles, an
    odd tile origin row, tile x origins at 8 mod 16; levels = 1 (nothing behind level 0) and 3 (a deep or tail launch behind it, and for
    the narrow edge tiles no separate level 1 worth the name).  Twice: the second run is on an idle device (a different issue timing,
    see test_gpu_pixels.py::test_rgba8_workgroup_kernels_shapes)."""
    import torch
    from j2kgfx.codec import FramePlan
    rng = np.random.default_rng(W * 7 + H + nres * 3 + ratio)
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=nres, cb=(64, 64), tile=_tile(tile), coder=1)
    img = _Image(rng, ratio, W, H)
    dimg, rgb = img.device(), img.rgb()
    assert plan.image_fused(dimg)
    expected = _oracle_coeff(oracle, plan, rgb, nres)
    prod = plan.forward_pixels(2, _dev(ref.rgba8_frame(rgb)))
    for run in range(2):
        got = plan.forward_image(dimg)
        plan.ctx.sync()
        _assert_coeff(got, expected, run)
        assert torch.equal(got, prod), run
    plan.close()


LAYOUT_SHAPES = [(424, 37, 384), (1040, 64, 512), (640, 150, (384, 75))]      # one small, one tiled, the odd tile origin row


@pytest.mark.parametrize("ratio", [0, 1, 2], ids=["444", "422", "420"])
@pytest.mark.parametrize("W,H,tile", LAYOUT_SHAPES)
def test_fused_kernel_layouts(oracle, W, H, tile, ratio):
    """ONE picture in every layout the fused kernel accepts gives ONE set of coefficients, the oracle's: Rect.Min (2,4), (6,2), (0,2) (4:2:0 at
    min_y = 2: Go's COffset folds Min.Y / 2 into the plane, the chroma row is the frame row >> 1), rows further apart than a row is long
    (the bytes between them random, and random again), planes that are views at aligned offsets of larger buffers with random bytes
    before and behind them."""
    import torch
    from j2kgfx.codec import FramePlan
    nres = 4
    rng = np.random.default_rng(W + H + ratio)
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=nres, cb=(64, 64), tile=_tile(tile), coder=1)
    content = _content(rng, ratio, W, H)
    base = _Image(rng, ratio, W, H, content=content)
    rgb = base.rgb()
    expected = _oracle_coeff(oracle, plan, rgb, nres)
    dimg = base.device()
    assert plan.image_fused(dimg)
    first = plan.forward_image(dimg)
    plan.ctx.sync()
    _assert_coeff(first, expected, "contiguous")
    ca = 8 if ratio == 0 else 4                                   # the chroma loads: 8 bytes per lane at 4:4:4, else 4
    layouts = [dict(mn=(2, 4)), dict(mn=(6, 2)), dict(mn=(0, 2)),
               dict(ypad=8, cpad=ca), dict(ypad=16, cpad=ca), dict(ypad=16),
               dict(offs=(16, ca, ca), slack=24), dict(offs=(16, ca, 2 * ca), slack=8, mn=(2, 2), ypad=8, cpad=ca)]
    for lay in layouts:
        img = _Image(rng, ratio, W, H, content=content, **lay)
        assert np.array_equal(img.rgb(), rgb), lay                # the same picture by the restatement
        for again in range(2 if (lay.get("ypad") or lay.get("cpad")) else 1):
            if again:
                img.rerandomise_pads(rng)                         # the pad bytes only
                assert np.array_equal(img.rgb(), rgb), lay
            dimg = img.device()
            assert plan.image_fused(dimg), lay
            got = plan.forward_image(dimg)
            plan.ctx.sync()
            _assert_coeff(got, expected, lay)
            assert torch.equal(got, first), lay
    plan.close()


def _saturating(kind, ratio, W, H):
    cw, ch = ref.chroma_dims(ratio, (0, 0, W, H))
    if kind in ("white", "zero"):
        v = 255 if kind == "white" else 0
        return tuple(np.full(s, v, np.uint8) for s in ((H, W), (ch, cw), (ch, cw)))
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = np.mgrid[0:ch, 0:cw]
    alt = ((cy + cx) & 1).astype(np.uint8) * 255                 # (0, 255, 0) and (255, 0, 255) sample by sample
    return (((yy + xx) & 1) * 255).astype(np.uint8), 255 - alt, alt


@pytest.mark.parametrize("ratio", [2, 0], ids=["420", "444"])
@pytest.mark.parametrize("kind", ["white", "zero", "alternating"])
def test_fused_kernel_saturating_content(oracle, kind, ratio):
    """Y = Cb = Cr = 255, all zeros, and (0, 255, 0) next to (255, 0, 255): every clamp of ycc_clamp16 at both ends feeding the RCT and the DPP lifting
    their extremes.  ((64,114) of the issue as the edge tile of (448,114): see SHAPES.)"""
    import torch
    from j2kgfx.codec import FramePlan
    W, H, nres = 448, 114, 4
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=nres, cb=(64, 64), tile=(384, 384), coder=1)
    img = _Image(np.random.default_rng(1), ratio, W, H, content=_saturating(kind, ratio, W, H))
    rgb, dimg = img.rgb(), img.device()
    if kind == "white":
        assert tuple(rgb[0, 0]) == tuple(int(v) for v in ref.ycbcr_rgb8(255, 255, 255)) and (rgb == rgb[0, 0]).all()
    if kind == "alternating":
        assert rgb.min() == 0 and rgb.max() == 255              # both clamps in use
    assert plan.image_fused(dimg)
    expected = _oracle_coeff(oracle, plan, rgb, nres)
    prod = plan.forward_pixels(2, _dev(ref.rgba8_frame(rgb)))
    for run in range(2):
        got = plan.forward_image(dimg)
        plan.ctx.sync()
        _assert_coeff(got, expected, run)
        assert torch.equal(got, prod)
    plan.close()


# ---- (2) ------------------------------------------------------------------------------------------------------------------------------------------
# One condition of image_fusable flipped per case, from an image and a plan for which it says "fused" (the controls).  The issue's example
# shape 64 x 34 is 384 x 34 here (see the module docstring), W = 20 and W = 64 follow it: 388 and 384.
# (name, image arguments, plan arguments, context option, fused?)
PW, PH, PNRES = 384, 34, 3
MEGA_PLAN = dict(W=768, H=68, tile=(384, 34), nres=4)      # the smallest plan that has a merged launch to offer: a deep launch from level 1 on
                                                           # (level 1 192 columns: not in LDS; level 2 is) over at least 12 tile-components
PREDICATE_CASES = [
    ("control-420", dict(ratio=2), {}, None, True),
    ("control-444", dict(ratio=0), {}, None, True),
    ("control-422-min-even-padded-views", dict(ratio=1, mn=(2, 2), ypad=8, cpad=4, offs=(16, 4, 8), slack=8), {}, None, True),
    ("min-x-odd", dict(ratio=2, mn=(1, 0)), {}, None, False),
    ("min-y-odd", dict(ratio=2, mn=(0, 1)), {}, None, False),
    ("min-x-negative", dict(ratio=2, mn=(-2, 0)), {}, None, False),
    ("min-y-negative", dict(ratio=2, mn=(0, -2)), {}, None, False),
    ("ratio-440", dict(ratio=3), {}, None, False),
    ("ratio-411", dict(ratio=4), {}, None, False),
    ("ratio-410", dict(ratio=5), {}, None, False),
    ("y-view-at-8", dict(ratio=2, offs=(8, 0, 0)), {}, None, False),
    ("ystride-w-plus-4", dict(ratio=2, ypad=4), {}, None, False),
    ("cb-view-at-2-420", dict(ratio=2, offs=(0, 2, 0)), {}, None, False),
    ("cr-view-at-2-420", dict(ratio=2, offs=(0, 0, 2)), {}, None, False),
    ("cb-view-at-4-444", dict(ratio=0, offs=(0, 4, 0)), {}, None, False),
    ("cstride-cw-plus-2", dict(ratio=2, cpad=2), {}, None, False),
    ("cstride-cw-plus-4-444", dict(ratio=0, cpad=4), {}, None, False),
    ("cb-cr-strides-differ", dict(ratio=2, cpad=4, cpad2=8), {}, None, False),      # (pixels.YCbCr takes one; the descriptor's third stride is set behind it)
    ("wavelet-9-7", dict(ratio=2), dict(lossless=False), None, False),
    # (a 1-component plan is J2K_ERR_INVALID_ARG: test_gpu_image_sources.py::test_errors_leave_output_untouched_and_context_usable.  mct off:
    #  FramePlan cannot make a 3-component plan without the colour transform -- S.mct = ncomp >= 3, encoder.go:223 -- so that condition of
    #  plan_rgba8_wg_fusable has no case)
    ("width-not-8n", dict(ratio=2), dict(W=388), None, False),
    ("edge-tile-8-columns", dict(ratio=2), dict(W=520, tile=(512, 512)), None, False),
    ("widest-plane-below-384", dict(ratio=2), dict(W=376), None, False),
    ("pix_fuse-0", dict(ratio=2), {}, ("pix_fuse", 0), False),
    ("l0_store-0", dict(ratio=2), {}, ("l0_store", 0), False),
    ("l0_fuse-8", dict(ratio=2), {}, ("l0_fuse", 8), False),
    ("l0_wg-0", dict(ratio=2), {}, ("l0_wg", 0), False),
    ("control-mega-plan", dict(ratio=2), MEGA_PLAN, None, True),
    ("mega-1", dict(ratio=2), MEGA_PLAN, ("mega", 1), False),
]


@pytest.mark.parametrize("name,image,plan_args,option,fused", PREDICATE_CASES, ids=[c[0] for c in PREDICATE_CASES])
def test_fusing_predicate_one_condition_at_a_time(oracle, name, image, plan_args, option, fused):
    """image_fusable says "fused" for the controls and "staged" with any one of its conditions flipped; either way forward_image gives the
    oracle's coefficients (twice), so a predicate that sends an image to the wrong side shows on one of the two assertions."""
    import torch
    from j2kgfx import Context
    from j2kgfx.codec import FramePlan
    W, H, nres = plan_args.get("W", PW), plan_args.get("H", PH), plan_args.get("nres", PNRES)
    lossless = plan_args.get("lossless", True)
    ctx = Context(0)
    if option:
        ctx.set_option(*option)
    plan = FramePlan(W, H, 3, precision=8, lossless=lossless, quality=0 if lossless else 75, num_resolutions=nres, cb=(32, 32),
                     tile=plan_args.get("tile", (0, 0)), coder=1, ctx=ctx)
    rng = np.random.default_rng(len(name) * 131 + W)
    img = _Image(rng, W=W, H=H, **image)
    rgb, dimg = img.rgb(), img.device()
    assert plan.image_fused(dimg) == fused
    expected = _oracle_coeff(oracle, plan, rgb, nres, lossless, 0 if lossless else 75)
    prod = plan.forward_pixels(2, _dev(ref.rgba8_frame(rgb)))
    for run in range(2):
        got = plan.forward_image(dimg)
        ctx.sync()
        _assert_coeff(got, expected, run)
        assert torch.equal(got, prod)
    plan.close()
    ctx.close()


# ---- (3) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ycc_table():
    return ref.ycbcr_table()


def test_every_ycbcr_triple_and_the_grid_stride_tail(ycc_table):
    """image_to_rgba8 of a 4:4:4 image of 4096 x 4100 whose pixel i < 2^24 is (Y, Cb, Cr) = (i & 255, (i >> 8) & 255, i >> 16): all 2^24
    triples against ycbcr_rgb8.  The launch is capped at 65 536 workgroups of 256 threads = 2^24 pixels: the last four rows (the first four
    again) are the second trip of the grid-stride loop."""
    from j2kgfx.pixels import YCbCr, image_to_rgba8
    Y, Cb, Cr, packed = ycc_table
    W, H, n = 4096, 4100, 1 << 24
    planes = [np.concatenate([p, p[:4 * W]]) for p in (Y, Cb, Cr)]
    got = image_to_rgba8(YCbCr(*[_dev(p) for p in planes], W, W, 0, (0, 0, W, H))).cpu().numpy().view(np.uint32).reshape(-1)
    assert got.size == W * H
    assert np.array_equal(got[:n], packed)
    assert np.array_equal(got[n:], packed[:4 * W])


def test_every_cmyk_value_pair_and_every_palette_entry():
    """a 256 x 256 image.CMYK whose pixel (k, c) is (C, M, Y, K) = (c, c ^ 0x5a, 255 - c, k): every channel meets every (value, K) pair,
    against cmyk_rgb8; an image.Paletted with all 256 entries in use and every byte value in each channel of the palette"""
    from j2kgfx.pixels import CMYK, Paletted, image_to_rgba8
    pix, packed = ref.cmyk_table()
    got = image_to_rgba8(CMYK(_dev(pix), 1024, (0, 0, 256, 256))).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, packed)
    rng = np.random.default_rng(3)
    pal = np.stack([rng.permutation(256) for _ in range(3)], axis=-1).astype(np.uint8)      # every byte value once per channel
    idx = np.concatenate([rng.permutation(256) for _ in range(4)]).astype(np.uint8)         # every index, four times
    assert len(np.unique(idx)) == 256 and all(len(np.unique(pal[:, c])) == 256 for c in range(3))
    got = image_to_rgba8(Paletted(_dev(idx), 64, (0, 0, 64, 16), _dev(pal))).cpu().numpy()
    assert np.array_equal(got, ref.rgba8_frame(ref.paletted_image_rgb(idx, 64, (0, 0, 64, 16), pal)))


# ---- (4) ------------------------------------------------------------------------------------------------------------------------------------------
def _closed_loop_image(kind, rng, W, H):
    """(colours (H, W, 3), device image)"""
    from j2kgfx.pixels import CMYK
    if kind == "ycc420":              # every image condition of the fused source holds: Rect.Min (2,2), padded strides
        img = _Image(rng, 2, W, H, mn=(2, 2), ypad=8, cpad=4)
        return img.rgb(), img.device()
    if kind == "ycc411":              # staged: the ratio, and Rect.Min (-3,5)
        img = _Image(rng, 4, W, H, mn=(-3, 5), ypad=3, cpad=1)
        return img.rgb(), img.device()
    stride = 4 * W + 12
    pix = rng.integers(0, 256, size=H * stride, dtype=np.uint8)
    return ref.cmyk_image_rgb(pix, stride, (1, 1, W + 1, H + 1)), CMYK(_dev(pix), stride, (1, 1, W + 1, H + 1))


# (W, H, tile, num_resolutions, code block): the issue's two, whose planes are too narrow for the fused kernel (the 4:2:0 image is staged
# there, like the rest), and one on which the 4:2:0 image IS read by the level-0 kernel
CLOSED_LOOP_GEOMETRIES = [(96, 50, 32, 3, 16), (64, 34, 0, 3, 32), (400, 34, 384, 3, 32)]


@pytest.mark.parametrize("coder", [0, 1], ids=["mq", "ht"])
@pytest.mark.parametrize("sop,eph", [(1, 1), (0, 0)])
@pytest.mark.parametrize("kind", ["ycc420", "ycc411", "cmyk"])
@pytest.mark.parametrize("W,H,tile,nres,cb", CLOSED_LOOP_GEOMETRIES)
def test_encode_frame_image_against_the_oracle(oracle, W, H, tile, nres, cb, kind, sop, eph, coder):
    """j2k_plan_encode_frame_image: the tile-parts are, byte for byte, the oracle's composition (closed_loop_ref.oracle_frame) on the restated
    colours at precision 8, lossless; lengths and numBPS of the parsed block tables are the oracle's (numBPS where a block has bytes, as
    check_every_stage compares it); with the MQ coder decode_frame_pixels gives the restated colours back."""
    import torch
    import t2ref
    from j2kgfx.codec import FramePlan
    orc = oracle
    rng = np.random.default_rng(W + H + coder * 5 + sop)
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=nres, cb=(cb, cb), tile=(tile, tile), coder=coder, closed_loop=True)
    rgb, dimg = _closed_loop_image(kind, rng, W, H)
    assert plan.image_fused(dimg) == (kind == "ycc420" and W == 400)
    frm = np.ascontiguousarray(rgb.transpose(2, 0, 1)).astype(np.int32)
    want = cl.oracle_frame(frm, W, H, tile or W, tile or H, nres, cb, coder, sop, eph, orc, t2ref)      # (HT: outside the reference encoder's panic domain, or a ValueError here)
    out, toffs = plan.encode_frame_image(dimg, sop=sop, eph=eph)
    plan.frame_status()
    h_cs, h_t = out.cpu().numpy(), toffs.cpu().numpy()
    assert len(want) == len(h_t) - 1
    for t in sorted(want):
        assert bytes(h_cs[int(h_t[t]):int(h_t[t + 1])]) == want[t]["part"], t
    total = int(h_t[-1])
    _, lens, numbps = plan.decode_tile_parts(out, total, tile_offs=toffs, sop=sop, eph=eph)
    plan.frame_status()
    want_lens = np.concatenate([want[t]["lens"] for t in sorted(want)])
    want_nb = np.concatenate([want[t]["numbps"] for t in sorted(want)])
    n, coded = want_lens.size, want_lens > 0
    assert n == int(plan.info.blocks)
    assert np.array_equal(lens.cpu().numpy()[:n].astype(np.uint32), want_lens)
    assert np.array_equal(numbps.cpu().numpy()[:n][coded], want_nb[coded])
    if coder == 0:
        back = torch.zeros((H, W * 4), dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(out, total, back, tile_offs=toffs, sop=sop, eph=eph)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy().reshape(H, W, 4)[..., :3], rgb)
    plan.close()
