"""GPU: the 16-bit hand-off of level 1's input X_1 between the packed-RGBA8 level-0 launch and the deep launch (context option
l0_scr16, J2K_L0_SCR16: bit 0 forward, dwt53_fwd_rgba8_wg16_kernel -> dwt53_deep_fwd16_kernel, static; bit 1 inverse,
dwt53_deep_inv16_kernel -> dwt53_inv_rgba8_wg16_kernel, a format chosen per stored row and recorded in a byte table), against the
oracle and against the same plan with the option off.  "On" below is J2K_L0_SCR16=3, both directions.  Which kernels a call launched
is read back from the plan (FramePlan.scr16_state bits 4 / 8 = the last forward / inverse call took the 16-bit kernels).

Geometries.  The narrow kernels run where the level-0 workgroup form does (some tile at least 384 wide, every tile 16 ... 512 wide
in multiples of 8) AND the deep launch starts at level 1 (12 tile-components, every level-1 plane at least 2 rows) -- checked
through FramePlan.scr16, which must say what tests/lossless53_cases.py's restated plan builder says:
  128x128 t64x64       the smallest frame with 12 tile-components: its planes are too narrow for the workgroup form, the LDS tail
                       takes level 1 -- stays int32
  904x113 t512x37      ragged: odd tile height, last tile column 392 wide, last tile row 2 high -- a level-1 plane of one row
                       rules the deep launch out -- stays int32
  904x114 t512x37      the same with a last tile row 3 high: 24 planes, level-1 planes 256x19 (deep + mid) ... 196x2 -- narrow
  1024x512 t512x512    the real row width (512), two tiles, with J2K_DEEP_MIN_PLANES=1 -- narrow
The forward contents push X_1 to its bound: per channel 0, 255, checkerboards and stripes of 0 / 255 both ways (period 1 and 2),
channels in opposite phase (so that U = B - G and V = R - G swing over +-255), the phase flipped from tile to tile, + seeded noise.
What level 0 of the reference makes of them (DC shift, RCT, one Forward2D53) stays within 4 * 255 + 3 + 128: asserted with the oracle."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NRES = 6
BOUND = 4 * 255 + 3 + 128            # J2K_SCR16_BOUND + dc_shift (csrc/j2k_internal.h)

# id, W, H, tile, extra environment, takes the 16-bit hand-off
GEOMS = [("128x128-t64", 128, 128, (64, 64), {}, False),
         ("904x113-t512x37", 904, 113, (512, 37), {}, False),
         ("904x114-t512x37", 904, 114, (512, 37), {}, True),
         ("1024x512-t512", 1024, 512, (512, 512), {"J2K_DEEP_MIN_PLANES": 1}, True)]
GEOM_IDS = [g[0] for g in GEOMS]


def _ctx(env):
    from j2kgfx import Context
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _plan(W, H, tile, env, on, C=3):
    from j2kgfx.codec import FramePlan
    ctx = _ctx(dict(env, J2K_L0_SCR16=3 if on else 0))
    return FramePlan(W, H, C, ctx=ctx, precision=8, lossless=True, num_resolutions=NRES, cb=(64, 64), tile=tile, coder=1)


def _tiles(W, H, tile):
    return [(x0, y0, min(tile[0], W - x0), min(tile[1], H - y0)) for y0 in range(0, H, tile[1]) for x0 in range(0, W, tile[0])]


def _frames(W, H, tile):
    """uint8 [H, W, 3] frames, named"""
    yy, xx = np.mgrid[0:H, 0:W]
    flip = ((xx // tile[0]) + (yy // tile[1])) & 1                # the phase changes from tile to tile
    pat = {"0": np.zeros((H, W), np.int64), "255": np.ones((H, W), np.int64),
           "chk": (xx + yy + flip) & 1, "hs": (yy + flip) & 1, "vs": (xx + flip) & 1,
           "chk2": ((xx >> 1) + (yy >> 1) + flip) & 1, "hs2": ((yy >> 1) + flip) & 1, "vs2": ((xx >> 1) + flip) & 1}
    inv = lambda a: 1 - a
    out = []
    for name, (r, g, b) in [("all0", ("0", "0", "0")), ("all255", ("255", "255", "255")), ("r255g0b255", ("255", "0", "255")),
                            ("r0g255b0", ("0", "255", "0"))]:
        out.append((name, np.stack([pat[r], pat[g], pat[b]], axis=2)))
    for p in ("chk", "hs", "vs", "chk2", "hs2", "vs2"):
        out.append((p + "-same", np.stack([pat[p]] * 3, axis=2)))
        out.append((p + "-opposed", np.stack([pat[p], inv(pat[p]), pat[p]], axis=2)))
    rng = np.random.default_rng(W * 7 + H)
    frames = [(n, (a * 255).astype(np.uint8)) for n, a in out]
    frames.append(("noise", rng.integers(0, 256, (H, W, 3), dtype=np.uint8)))
    mix = frames[5][1].copy()                                     # chk-opposed with a fifth of its samples replaced by noise
    m = rng.random((H, W, 3)) < 0.2
    mix[m] = rng.integers(0, 256, int(m.sum()), dtype=np.uint8)
    frames.append(("chk-opposed+noise", mix))
    return frames


def _pix(rgb):
    H, W, _ = rgb.shape
    return np.ascontiguousarray(np.concatenate([rgb, np.full((H, W, 1), 255, np.uint8)], axis=2).reshape(H, W * 4))


def _want_coeff(oracle, pix, W, H, tile):
    """per tile: [3] planes of encoder.preprocess on the cropped image.RGBA"""
    out = []
    for x0, y0, w, h in _tiles(W, H, tile):
        crop = np.ascontiguousarray(pix.reshape(H, W, 4)[y0:y0 + h, x0:x0 + w].reshape(h, w * 4))
        out.append(oracle.preprocess(oracle.extract_image_data(crop, 2, w, h), w, h, 8, True, NRES))
    return out


def _check_coeff(plan, hco, want, W, H, tile, what):
    planes = plan.planes()
    for tl, (x0, y0, w, h) in enumerate(_tiles(W, H, tile)):
        for c in range(3):
            row = planes[tl * 3 + c]
            assert (int(row[0]), int(row[1]), int(row[4]), int(row[5])) == (tl, c, w, h)
            off = int(row[6])
            assert np.array_equal(hco[off:off + w * h].reshape(h, w), want[tl][c]), (what, tl, c)


def _want_pixels(oracle, plan, coef_h, W, H, tile):
    """ReconstructMultiLevel53 + InverseRCT + DC shift + createImage of every tile's coefficients -> uint8 [H, W * 4]"""
    planes = plan.planes()
    out = np.zeros((H, W, 4), np.uint8)
    for tl, (x0, y0, w, h) in enumerate(_tiles(W, H, tile)):
        rec = []
        for c in range(3):
            off = int(planes[tl * 3 + c][6])
            rec.append(oracle.reconstruct53(coef_h[off:off + w * h].reshape(h, w), w, h, NRES - 1))
        out[y0:y0 + h, x0:x0 + w] = oracle.create_image(oracle.postprocess(rec, 8, True), 8).reshape(h, w, 4)
    return out.reshape(H, W * 4)


def _inverse(plan, coef_h):
    import torch
    back = plan.inverse_rgba8(torch.from_numpy(coef_h).to(plan.device))
    plan.ctx.sync()
    return back.cpu().numpy()


def _level1_input_bound(oracle, rgb):
    """max |X_1| of one tile by the oracle: DC shift, RCT, one Forward2D53; X_1 = the first ceil(h/2) * (w/2) elements"""
    h, w, _ = rgb.shape
    comps = [oracle.dc_shift_fwd(np.ascontiguousarray(rgb[:, :, k]).astype(np.int32), 8) for k in range(3)]
    worst = 0
    for p in oracle.rct_fwd(*comps):
        x = oracle.fwd53_2d(np.ascontiguousarray(p.reshape(h, w)), w, h).reshape(-1)[:((h + 1) // 2) * (w // 2)]
        worst = max(worst, int(np.abs(x.astype(np.int64)).max()))
    return worst


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_plan_condition(geom):
    """FramePlan.scr16 under the option = the restated plan builder's 'workgroup level 0 and a deep launch from level 1'; never with
    the option off, with a fourth component (the plane kernels write its prefix), or on a Mallat plan"""
    import lossless53_cases as lc
    from j2kgfx.codec import FramePlan
    _, W, H, tile, env, narrow = geom
    R = lc.route(W, H, 3, tile, NRES, tuple(sorted(env.items())))
    assert (R["deep_l0"] == 1 and bool(R["rgba8"]) and R["rgba8"]["fwd_wg"] is not None) == narrow
    assert _plan(W, H, tile, env, True).scr16 == narrow
    assert _plan(W, H, tile, env, True).scr16_state == (3 if narrow else 0)
    assert not _plan(W, H, tile, env, False).scr16_state
    assert not _plan(W, H, tile, env, True, C=4).scr16_state
    for v in (1, 2):
        ctx = _ctx(dict(env, J2K_L0_SCR16=v))
        assert FramePlan(W, H, 3, ctx=ctx, precision=8, lossless=True, num_resolutions=NRES, cb=(64, 64), tile=tile, coder=1).scr16_state == (v if narrow else 0)
    ctx = _ctx(dict(env, J2K_L0_SCR16=3))
    if narrow:
        assert not FramePlan(W, H, 3, ctx=ctx, precision=8, lossless=True, num_resolutions=NRES, cb=(64, 64), tile=tile, coder=0, mallat=True).scr16_state


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_forward_bound(oracle, geom):
    """every content: coefficients = the oracle's, and byte for byte the same plan's with J2K_L0_SCR16=0"""
    import torch
    _, W, H, tile, env, narrow = geom
    on, off = _plan(W, H, tile, env, True), _plan(W, H, tile, env, False)
    assert on.scr16 == narrow
    x0, y0, w, h = _tiles(W, H, tile)[0]
    worst = 0
    for name, rgb in _frames(W, H, tile):
        pix = _pix(rgb)
        b = _level1_input_bound(oracle, rgb[y0:y0 + h, x0:x0 + w])
        worst = max(worst, b)
        assert b <= BOUND, (name, b)
        d = torch.from_numpy(pix).to(on.device)
        c_on, c_off = on.forward_rgba8(d), off.forward_rgba8(d)
        on.ctx.sync(); off.ctx.sync()
        assert bool(on.scr16_state & 4) == narrow and not off.scr16_state & 4      # the call did launch the 16-bit kernels / did not
        h_on, h_off = c_on.cpu().numpy(), c_off.cpu().numpy()
        assert h_on.tobytes() == h_off.tobytes(), name
        _check_coeff(on, h_on, _want_coeff(oracle, pix, W, H, tile), W, H, tile, name)
    print("%s: largest |X_1| of the first tile over the contents: %d (bound %d)" % (geom[0], worst, BOUND))
    assert worst >= 2 * 255                       # the contents do reach beyond one lifting step's range


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_inverse_narrow_wide_mixed(oracle, geom):
    """(a) the forward's own coefficients give the pixels back; (b) full-range int32 junk; (c) constant planes at the edge of int16 -- X_1 then
    holds the constant itself; (d) small coefficients with one large one per tile: all as the oracle reconstructs them"""
    import torch
    _, W, H, tile, env, narrow = geom
    plan = _plan(W, H, tile, env, True)
    rng = np.random.default_rng(W + 3 * H)
    rgb = _frames(W, H, tile)[-1][1]
    pix = _pix(rgb)
    coeff = plan.forward_rgba8(torch.from_numpy(pix).to(plan.device))
    back = plan.inverse_rgba8(coeff)
    plan.ctx.sync()
    assert bool(plan.scr16_state & 8) == narrow          # the call did launch dwt53_deep_inv16_kernel + dwt53_inv_rgba8_wg16_kernel
    assert np.array_equal(back.cpu().numpy(), pix)                                                   # (a)
    n = coeff.numel()
    junk = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)                       # (b)
    assert np.array_equal(_inverse(plan, junk), _want_pixels(oracle, plan, junk, W, H, tile))
    edge = np.zeros(n, np.int32)                                                                     # (c)
    consts = (32767, 32768, -32768, -32769, 0)
    planes = plan.planes()
    for i, row in enumerate(planes):
        w, h, off, c = int(row[4]), int(row[5]), int(row[6]), consts[i % 5]
        k = oracle.decompose53(np.full((h, w), c, np.int32), w, h, NRES - 1)
        edge[off:off + w * h] = k.reshape(-1)
        if i < 5 and h >= 2:                          # on the CPU first: X_1 of these coefficients holds the constant (and zeros) only
            w1, h1 = w // 2, (h + 1) // 2
            x1 = oracle.reconstruct53(np.ascontiguousarray(k.reshape(-1)[:w1 * h1].reshape(h1, w1)), w1, h1, NRES - 2)
            assert set(np.unique(x1).tolist()) == {0, c}, (i, c)
    assert np.array_equal(_inverse(plan, edge), _want_pixels(oracle, plan, edge, W, H, tile))
    mixed = rng.integers(-200, 201, n).astype(np.int32)                                              # (d)
    for i, row in enumerate(planes):
        w, h, off = int(row[4]), int(row[5]), int(row[6])
        mixed[off + int(rng.integers(0, w * h))] = (1 << 20) * (1 if i & 1 else -1)
    assert np.array_equal(_inverse(plan, mixed), _want_pixels(oracle, plan, mixed, W, H, tile))
    assert bool(plan.scr16_state & 8) == narrow
    # the same four through the same plan with the option off: byte for byte
    off = _plan(W, H, tile, env, False)
    for co in (junk, edge, mixed):
        assert np.array_equal(_inverse(off, co), _inverse(plan, co))
    assert not off.scr16_state & 8


def _want_planes(oracle, plan, coef_h, W, H, tile):
    """the planar inverse: ReconstructMultiLevel53 + InverseRCT + DC shift of every tile -> int32 [3, H, W]"""
    planes = plan.planes()
    out = np.zeros((3, H, W), np.int32)
    for tl, (x0, y0, w, h) in enumerate(_tiles(W, H, tile)):
        rec = [oracle.reconstruct53(coef_h[int(planes[tl * 3 + c][6]):int(planes[tl * 3 + c][6]) + w * h].reshape(h, w), w, h, NRES - 1) for c in range(3)]
        for c, p in enumerate(oracle.postprocess(rec, 8, True)):
            out[c, y0:y0 + h, x0:x0 + w] = p
    return out


@pytest.mark.parametrize("geom", GEOMS[2:], ids=GEOM_IDS[2:])
def test_no_stale_format(oracle, geom):
    """one plan, one scratch buffer: junk through the inverse (int32 rows), pixels through the forward (int16 rows), full-range int32 PLANES through
    the planar forward (int32 rows in the same slots), the pixels again, junk again -- every result exact"""
    import torch
    _, W, H, tile, env, narrow = geom
    plan = _plan(W, H, tile, env, True)
    assert plan.scr16
    rng = np.random.default_rng(5 * W + H)
    pix = _pix(_frames(W, H, tile)[5][1])
    want = _want_coeff(oracle, pix, W, H, tile)
    d = torch.from_numpy(pix).to(plan.device)
    n = plan.alloc_coeff().numel()
    junk = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    want_junk = _want_pixels(oracle, plan, junk, W, H, tile)
    frame = rng.integers(-2 ** 31, 2 ** 31, (3, H, W), dtype=np.int64).astype(np.int32)
    want_planar = [oracle.preprocess([np.ascontiguousarray(frame[c, y0:y0 + h, x0:x0 + w]) for c in range(3)], w, h, 8, True, NRES)
                   for x0, y0, w, h in _tiles(W, H, tile)]

    def fwd_pixels():
        c = plan.forward_rgba8(d)
        plan.ctx.sync()
        return c.cpu().numpy()
    assert np.array_equal(_inverse(plan, junk), want_junk)
    _check_coeff(plan, fwd_pixels(), want, W, H, tile, "pixels after junk")
    c = plan.forward(torch.from_numpy(frame).to(plan.device))
    plan.ctx.sync()
    _check_coeff(plan, c.cpu().numpy(), want_planar, W, H, tile, "planes after pixels")
    _check_coeff(plan, fwd_pixels(), want, W, H, tile, "pixels after planes")
    assert np.array_equal(_inverse(plan, junk), want_junk)
    small = rng.integers(-300, 300, n).astype(np.int32)
    want_small = _want_pixels(oracle, plan, small, W, H, tile)
    assert np.array_equal(_inverse(plan, small), want_small)
    assert np.array_equal(_inverse(plan, junk), want_junk)
    # another reader of the same scratch: the planar inverse (the general level-0 kernel) gets int32 rows from its own deep launch, whatever the
    # table says after the call before it; then the pixels again
    assert np.array_equal(_inverse(plan, small), want_small) and plan.scr16_state & 8
    back = plan.inverse(torch.from_numpy(junk).to(plan.device))
    plan.ctx.sync()
    assert not plan.scr16_state & 8
    assert np.array_equal(back.cpu().numpy(), _want_planes(oracle, plan, junk, W, H, tile))
    back = plan.inverse(torch.from_numpy(small).to(plan.device))
    plan.ctx.sync()
    assert np.array_equal(back.cpu().numpy(), _want_planes(oracle, plan, small, W, H, tile))
    assert np.array_equal(_inverse(plan, small), want_small) and plan.scr16_state & 8
    # an option changed after the plan was made: the call falls back to the int32 kernels of that setting
    plan.ctx.set_option("l0_store", 0)
    _check_coeff(plan, fwd_pixels(), want, W, H, tile, "pixels, l0_store 0 set after the plan")
    assert not plan.scr16_state & 4
    plan.ctx.set_option("l0_inv_wpe", 6)
    assert np.array_equal(_inverse(plan, junk), want_junk) and not plan.scr16_state & 8


def _child_arrays(W, H, tile, env):
    """what the child process computes, from seeds alone: (pixels, junk coefficients)"""
    rng = np.random.default_rng(77)
    pix = _pix(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    return pix, rng


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=[GEOM_IDS[0], GEOM_IDS[2]])
def test_off_switch_in_a_child_process(oracle, geom):
    """J2K_L0_SCR16=0 in the environment of a fresh process: the coefficients and pixels of a build without the option, which are the oracle's"""
    name, W, H, tile, env, narrow = geom
    e = dict(os.environ, J2K_TUNING="1", J2K_L0_SCR16="0", **{k: str(v) for k, v in env.items()})
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True, text=True, timeout=300, env=e)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    got = dict(l.split("=", 1) for l in out.stdout.strip().splitlines() if "=" in l)
    assert got["scr16"] == "0"
    pix, rng = _child_arrays(W, H, tile, env)
    want = _want_coeff(oracle, pix, W, H, tile)
    plan = _plan(W, H, tile, env, False)             # (for the plane table and the oracle's side only)
    n = plan.alloc_coeff().numel()
    co = np.zeros(n, np.int32)
    for tl, (x0, y0, w, h) in enumerate(_tiles(W, H, tile)):
        for c in range(3):
            off = int(plan.planes()[tl * 3 + c][6])
            co[off:off + w * h] = want[tl][c].reshape(-1)
    junk = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    assert got["coeff"] == _digest(co)
    assert got["back"] == _digest(pix)
    assert got["back_junk"] == _digest(_want_pixels(oracle, plan, junk, W, H, tile))


def _child(name):
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "go-jpeg2000_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    from j2kgfx import Context
    from j2kgfx.codec import FramePlan
    _, W, H, tile, env, narrow = GEOMS[GEOM_IDS.index(name)]
    plan = FramePlan(W, H, 3, ctx=Context(0), precision=8, lossless=True, num_resolutions=NRES, cb=(64, 64), tile=tile, coder=1)
    pix, rng = _child_arrays(W, H, tile, env)
    coeff = plan.forward_rgba8(torch.from_numpy(pix).to(plan.device))
    back = plan.inverse_rgba8(coeff)
    plan.ctx.sync()
    junk = rng.integers(-2 ** 31, 2 ** 31, coeff.numel(), dtype=np.int64).astype(np.int32)
    print("scr16=%d" % int(plan.scr16))
    print("coeff=" + _digest(coeff.cpu().numpy()))
    print("back=" + _digest(back.cpu().numpy()))
    print("back_junk=" + _digest(_inverse(plan, junk)))


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--child"
    _child(sys.argv[2])
