"""GPU: the region-of-interest encode (roi=, roi_gain= of encode_blocks(planes=True) / encode_frame_pixels / encode_pixels_host; j2k_plan_roi_windows,
j2k_plan_encode_blocks_planes_roi, j2k_plan_encode_frame_pixels_roi, j2k_encode_pixels_host_roi) against tests/roi_cases.py.

  windows      roi_windows equals the definition exactly on roi_cases.GEOMETRIES x 5-3 / 9-7 and all their rectangles
  tables       D_roi is bit for bit the definition on the device's own coefficients, gains 1, 2, 16, 65535; slots, lens, numbps and rate are those
               of the call without roi; one hand-made coefficient frame per KMAX class (numBPS 8, 12, 16, 31) whose rectangles cut blocks partially,
               with a sub-window narrower than its 64-wide block and one of a single sample
  frames       encode_frame_pixels(max_body_bytes=, roi=) and (layer_bytes=[...] x 3, roi=) are byte for byte the composition of the stage calls;
               kept is rate_cases.allocate on the device's R and the definition's D_roi; encode_pixels_host gives the same bytes; roi_gain=1 gives
               the bytes of the call without roi -- 5-3 on the three-component tiled geometry, 9-7 with dequantize=True on the gray one
  round trip   decode_frame_pixels(truncated=True) / (layers=k) return the coarse reconstruction of kept bit for bit; area=roi returns its crop; the
               effect inequalities of tests/test_roi_cases.py on the device's own rate tables
  refusals     every listed case returns its status and leaves the output buffers alone
"""
import ctypes as C
import functools

import numpy as np
import pytest

import area_cases as ac
import closed_loop_ref as ref
import coarse_cases as cc
import layer_cases as lc
import mallat_cases as mc
import rate_cases as rc
import roi_cases as roi
import test_gpu_layers as tl
import test_gpu_rate_frames as rf

pytestmark = pytest.mark.gpu
Q97 = mc.LOSSY[0][6]
FILL = 0x77
# (case, lossless, quality, cb) as tests/test_gpu_layers.py's plan specs, and the rectangle of the frame tests
SPEC53 = (roi.GEOMETRIES[0][0], True, 0, roi.GEOMETRIES[0][1])
SPEC97 = (roi.GEOMETRIES[1][0], False, Q97, roi.GEOMETRIES[1][1])
FRAME_SPECS = [(SPEC53, (37, 11, 90, 40)), (SPEC97, (20, 12, 44, 36))]
FRAME_IDS = ["130x70x3-tiled-53", "64x48-97q%d" % Q97]


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    from j2kgfx import Context
    ctx = Context(0)
    yield torch, orc, ctx
    ctx.close()


def _geometry_plan(ctx, g, wavelet, **kw):
    (case, cb) = g
    return tl._plan(ctx, (case, wavelet == "53", 0 if wavelet == "53" else Q97, cb), **kw)


def _u(t):
    return t.cpu().numpy().view(np.uint32 if t.element_size() == 4 else np.uint64)


def _block_values(plan, h_coeff):
    """every block's coefficients out of the plan's flat coefficient buffer (host copy)"""
    rows = {(int(r[0]), int(r[1])): (int(r[4]), int(r[5]), int(r[6])) for r in plan.planes()}
    Cn, out = plan.ncomp, []
    for b in plan.blocks():
        w, h, off = rows[(int(b["plane"]) // Cn, int(b["plane"]) % Cn)]
        p = h_coeff[off:off + w * h].reshape(h, w)
        out.append(p[int(b["y0"]):int(b["y0"]) + int(b["h"]), int(b["x0"]):int(b["x0"]) + int(b["w"])])
    return out


def _same_codewords(plan, a, b):
    """slots (the coded bytes of every block), lens, numbps and rate of two encode_blocks(planes=True) results are identical"""
    n = int(plan.info.blocks)
    assert np.array_equal(_u(a[1])[:n], _u(b[1])[:n]) and np.array_equal(a[2].cpu().numpy()[:n], b[2].cpu().numpy()[:n])
    assert np.array_equal(_u(a[3])[:n], _u(b[3])[:n])
    sa, sb, lens = a[0].cpu().numpy(), b[0].cpu().numpy(), _u(a[1])[:n]
    for j, lo in enumerate(tl._slot_offsets(plan)):
        assert bytes(sa[lo:lo + int(lens[j])]) == bytes(sb[lo:lo + int(lens[j])]), j


# ---- windows ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", roi.WAVELETS)
@pytest.mark.parametrize("g", roi.GEOMETRIES, ids=[roi.geometry_id(g) for g in roi.GEOMETRIES])
def test_roi_windows(env, g, wavelet):
    torch, orc, ctx = env
    (W, H, Cn, _prec, tile, nres), cb = g
    plan = _geometry_plan(ctx, g, wavelet)
    try:
        bl = plan.blocks()
        some = 0
        for q in roi.rectangles(W, H):
            want = roi.frame_windows(bl, Cn, W, H, tile, nres, q, wavelet)
            got = plan.roi_windows(q)
            ctx.sync()
            assert np.array_equal(got.cpu().numpy(), want), q
            some += int((want[:, 2] > 0).sum())
        assert some > 0
    finally:
        plan.close()


# ---- distortion tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", roi.WAVELETS)
@pytest.mark.parametrize("g", roi.GEOMETRIES, ids=[roi.geometry_id(g) for g in roi.GEOMETRIES])
def test_distortion_tables(env, g, wavelet):
    """a pixel frame through the device's own forward transform; D_roi of its coefficients for every gain on two rectangles"""
    torch, orc, ctx = env
    (W, H, Cn, prec, tile, nres), cb = g
    plan = _geometry_plan(ctx, g, wavelet)
    try:
        fmt = mc.PIX_FORMAT[(Cn, prec)]
        pix, _, _, _ = ref.pixel_frame(fmt, W, H, 17, orc, noise=(1 << prec) // 16)
        coeff = plan.forward_pixels(fmt, torch.from_numpy(pix).to(plan.device))
        plain = plan.encode_blocks(coeff, planes=True)
        ctx.sync()
        n = int(plan.info.blocks)
        vals, nbs, bl = _block_values(plan, coeff.cpu().numpy()), plain[2].cpu().numpy()[:n], plan.blocks()
        D0 = _u(plain[4])[:n]
        assert np.array_equal(D0, roi.frame_distortion(vals, nbs, [(0, 0, 0, 0)] * n, 1))
        rects = roi.rectangles(W, H)
        for q in (rects[3], rects[-1]):                              # the odd-origin rectangle across the seams; the last of the list
            wins = roi.frame_windows(bl, Cn, W, H, tile, nres, q, wavelet)
            assert any(0 < F[2] * F[3] < int(b["w"]) * int(b["h"]) for F, b in zip(wins, bl)), "vacuous: no block cut by the footprint"
            for gain in roi.GAINS:
                got = plan.encode_blocks(coeff, planes=True, roi=q, roi_gain=gain)
                ctx.sync()
                D = _u(got[4])[:n]
                assert np.array_equal(D, roi.frame_distortion(vals, nbs, wins, gain)), (q, gain)
                assert np.array_equal(D, D0) == (gain == 1), (q, gain)
                if gain in (1, 65535):
                    _same_codewords(plan, got, plain)
    finally:
        plan.close()


@functools.lru_cache(None)
def _kmax_tiles(W, H, cb, nres, bits):
    """a coefficient frame whose every block has numBPS = bits: random magnitudes below 2^bits, the top value once per block"""
    import oracle as orc
    rng = np.random.default_rng(1000 + bits)
    t = rng.integers(-(1 << bits) + 1, 1 << bits, (1, H, W)).astype(np.int64)
    for b in orc.enumerate_blocks(1, W, H, nres, cb, cb, 1):
        t[0, int(b["y0"]) + int(b["h"]) // 2, int(b["x0"]) + int(b["w"]) // 2] = (1 << bits) - 1 if bits & 1 else -(1 << bits) + 1
    return [t.astype(np.int32)]


# (W, H, resolutions, cb, rectangles): 64-wide blocks cut to sub-windows narrower than their 64 lanes; a sub-window of a single sample
KMAX_PLANS = [(130, 70, 2, 64, ((37, 11, 90, 40), (128, 0, 130, 3))), (33, 17, 2, 64, ((32, 16, 33, 17),))]


@pytest.mark.parametrize("bits", [8, 12, 16, 31])
def test_every_kmax_class_through_the_sub_window(env, bits):
    torch, orc, ctx = env
    from j2kgfx.codec import FramePlan
    narrow = single = 0
    for W, H, nres, cb, rects in KMAX_PLANS:
        plan = FramePlan(W, H, 1, precision=16, lossless=True, num_resolutions=nres, cb=(cb, cb), coder=0, ctx=ctx, mallat=True)
        try:
            tiles = _kmax_tiles(W, H, cb, nres, bits)
            coeff = torch.from_numpy(mc.flat_coeff(plan.planes(), tiles, int(plan.info.coeff_elems))).to(plan.device)
            n, bl = int(plan.info.blocks), plan.blocks()
            vals = _block_values(plan, coeff.cpu().numpy())
            for q in rects:
                wins = roi.frame_windows(bl, 1, W, H, (0, 0), nres, q, "53")
                narrow += sum(1 for F, b in zip(wins, bl) if 0 < F[2] < int(b["w"]) == 64)
                single += sum(1 for F, b in zip(wins, bl) if (F[2], F[3]) == (1, 1) and int(b["w"]) * int(b["h"]) > 1)
                for gain in (16, 65535):
                    got = plan.encode_blocks(coeff, planes=True, roi=q, roi_gain=gain)
                    ctx.sync()
                    nbs = got[2].cpu().numpy()[:n]
                    assert (nbs == bits).all()
                    assert np.array_equal(_u(got[4])[:n], roi.frame_distortion(vals, nbs, wins, gain)), (W, q, gain)
        finally:
            plan.close()
    assert narrow > 0 and single > 0


# ---- frames -------------------------------------------------------------------------------------------------------------------------------------
_FRAMES = {}


@pytest.fixture()
def shared(env, request):
    """(spec, rectangle, plan, test_gpu_layers.Frame, the definition's D_roi for gain 16) -- the Frame and the tables once per spec"""
    torch, orc, ctx = env
    spec, q = FRAME_SPECS[request.param]
    plan = tl._plan(ctx, spec)
    try:
        if request.param not in _FRAMES:
            F = tl.Frame(torch, plan, spec)
            (W, H, Cn, prec, tile, nres) = spec[0]
            coeff = plan.forward_pixels(F.fmt, F.d_pix)
            plan.ctx.sync()
            wins = roi.frame_windows(plan.blocks(), Cn, W, H, tile, nres, q, "53" if spec[1] else "97")
            vals = _block_values(plan, coeff.cpu().numpy())
            F.Droi = {g: roi.frame_distortion(vals, F.nbs, wins, g) for g in (1, 16)}
            assert np.array_equal(F.Droi[1], F.D)
            _FRAMES[request.param] = F
        yield spec, q, plan, _FRAMES[request.param]
    finally:
        plan.close()


def _bytes(cs, toffs):
    return bytes(cs.cpu().numpy()[:int(toffs[-1].item())])


def _budgets(F):
    return F.U // 4, [F.U // 10, F.U // 4, F.U // 2]


@pytest.mark.parametrize("shared", range(len(FRAME_SPECS)), ids=FRAME_IDS, indirect=True)
def test_frames_are_the_composition_of_the_stage_calls(env, shared):
    torch, orc, ctx = env
    spec, q, plan, F = shared
    B, LB = _budgets(F)
    n = F.n
    coeff = plan.forward_pixels(F.fmt, F.d_pix)
    slots, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True, roi=q, roi_gain=16)
    plan.ctx.sync()
    assert np.array_equal(_u(dist)[:n], F.Droi[16]) and np.array_equal(_u(rate)[:n].astype(np.int64), F.R)
    offs, stream = plan.compact(slots, lens)
    for marks in (False, True):
        # one budget: kept is the yardstick's allocation on the device's R and the definition's D_roi
        kept, chosen = plan.rate_allocate(rate, dist, nbs, B)
        want_ps, want_chosen = rc.allocate(F.R, F.Droi[16], F.nbs, F.ws, B)
        plain_ps, _ = rc.allocate(F.R, F.D, F.nbs, F.ws, B)
        stage, stoffs = plan.encode_tile_parts(stream, offs, lens, nbs, sop=marks, eph=marks, kept=kept, rate=rate)
        cs, toffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, max_body_bytes=B, roi=q, roi_gain=16)
        plan.frame_status()
        assert kept.cpu().numpy()[:n].tolist() == want_ps and int(chosen.item()) == want_chosen <= B
        assert want_ps != plain_ps, "vacuous: the weight moved nothing"
        assert _bytes(cs, toffs) == _bytes(stage, stoffs) and toffs.cpu().numpy().tolist() == stoffs.cpu().numpy().tolist()
        host = plan.encode_pixels_host(F.fmt, F.pix, sop=marks, eph=marks, max_body_bytes=B, roi=q, roi_gain=16)
        assert bytes(host["bytes"]) == _bytes(cs, toffs) and host["tile_offs"].tolist() == toffs.cpu().numpy().tolist() and "layer_offs" not in host
        assert host["lens"].tolist() == F.lens and host["numbps"].tolist() == F.nbs
        one, otoffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, max_body_bytes=B, roi=q, roi_gain=1)
        base, btoffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, max_body_bytes=B)
        plan.frame_status()
        assert _bytes(one, otoffs) == _bytes(base, btoffs) != _bytes(cs, toffs)
        # three layers
        lkept, lchosen = plan.rate_allocate_layers(rate, dist, nbs, LB)
        want_k, want_c = lc.allocate_layers(F.R, F.Droi[16], F.nbs, F.ws, LB)
        stage, stoffs, sloffs = plan.encode_tile_parts(stream, offs, lens, nbs, sop=marks, eph=marks, kept=lkept, rate=rate, layers=3)
        cs, toffs, loffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, layer_bytes=LB, roi=q, roi_gain=16)
        plan.frame_status()
        assert lkept.cpu().numpy().tolist() == want_k and lchosen.cpu().numpy().tolist() == want_c
        assert _bytes(cs, toffs) == _bytes(stage, stoffs) and loffs.cpu().numpy().tolist() == sloffs.cpu().numpy().tolist()
        host = plan.encode_pixels_host(F.fmt, F.pix, sop=marks, eph=marks, layer_bytes=LB, roi=q, roi_gain=16)
        assert bytes(host["bytes"]) == _bytes(cs, toffs) and host["layer_offs"].tolist() == loffs.cpu().numpy().tolist()
        one, otoffs, oloffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, layer_bytes=LB, roi=q, roi_gain=1)
        base, btoffs, bloffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, layer_bytes=LB)
        plan.frame_status()
        assert _bytes(one, otoffs) == _bytes(base, btoffs) != _bytes(cs, toffs) and oloffs.cpu().numpy().tolist() == bloffs.cpu().numpy().tolist()
        # one layer through the layered form is the single-budget stream
        l1, l1toffs, _ = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, layer_bytes=[B], roi=q, roi_gain=16)
        r1, r1toffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, max_body_bytes=B, roi=q, roi_gain=16)
        plan.frame_status()
        assert _bytes(l1, l1toffs) == _bytes(r1, r1toffs)


@pytest.mark.parametrize("shared", range(len(FRAME_SPECS)), ids=FRAME_IDS, indirect=True)
def test_round_trip(env, shared):
    torch, orc, ctx = env
    spec, q, plan, F = shared
    (W, H, Cn, prec, tile, nres) = spec[0]
    B, LB = _budgets(F)
    bpp = ac.bytes_per_pixel(Cn, prec)
    ah, aw = plan.area_shape(q)
    # one budget, truncated=True
    ps, _ = rc.allocate(F.R, F.Droi[16], F.nbs, F.ws, B)
    cs, toffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=True, eph=True, max_body_bytes=B, roi=q, roi_gain=16)
    plan.frame_status()
    length = int(toffs[-1].item())
    exp = F.expected(orc, spec, ps, 0, 0)
    back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
    plan.decode_frame_pixels(cs, length, back, sop=True, eph=True, truncated=True)
    plan.frame_status()
    assert np.array_equal(back.cpu().numpy(), exp)
    part = torch.full((ah, aw * bpp), 0x5A, dtype=torch.uint8, device=plan.device)
    plan.decode_frame_pixels(cs, length, part, sop=True, eph=True, truncated=True, area=q)
    plan.frame_status()
    assert np.array_equal(part.cpu().numpy(), ac.crop(exp, q, 0, bpp))
    # three layers, layers=k for every k
    kept, _ = lc.allocate_layers(F.R, F.Droi[16], F.nbs, F.ws, LB)
    Q = list(zip(*[lc.normalise(F.R[j], [kept[l][j] for l in range(3)]) for j in range(F.n)]))
    cs, toffs, loffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=False, eph=False, layer_bytes=LB, roi=q, roi_gain=16)
    plan.frame_status()
    length = int(toffs[-1].item())
    for k in (1, 2, 3):
        exp = F.expected(orc, spec, Q[k - 1], 0, 0)
        back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, length, back, layers=k)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp), k
        part = torch.full((ah, aw * bpp), 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, length, part, layers=k, area=q)
        plan.frame_status()
        assert np.array_equal(part.cpu().numpy(), ac.crop(exp, q, 0, bpp)), k


def test_effect_on_the_device_tables(env):
    """the frame of tests/test_roi_cases.py's effect test through the device: at 25 % and 50 % of the uncut body bytes the decoded frame's squared
    error inside the rectangle is smaller with roi_gain=16 than without roi, the error outside is not, and the body bytes stay within the budget.
    The decoded pixels are first held to the definition's cuts on the device's R (R[p] = the coder's byte index + 5 is looser than
    layer_cases.shortest_rates, which the CPU test uses), so the inequalities are evaluated on exactly those tables."""
    torch, orc, ctx = env
    E = roi.EFFECT
    case, q = E["case"], E["roi"]
    W, H, Cn, prec, tile, nres = case
    spec = (case, True, 0, E["cb"])
    plan = tl._plan(ctx, spec)
    try:
        fmt = mc.PIX_FORMAT[(Cn, prec)]
        pix, _, _, planes = ref.pixel_frame(fmt, W, H, E["seed"], orc, noise=E["noise"])
        ctiles = mc.forward_frame(orc, planes, tile, prec, nres, True, 0)
        d_pix = torch.from_numpy(pix).to(plan.device)
        coeff = plan.forward_pixels(fmt, d_pix)
        slots, lens, nbs_t, rate, dist = plan.encode_blocks(coeff, planes=True)
        plan.ctx.sync()
        n = int(plan.info.blocks)
        R, nbs = _u(rate)[:n].astype(np.int64), [int(x) for x in nbs_t.cpu().numpy()[:n]]
        U = int(_u(lens)[:n].astype(np.int64).sum())
        w, res, bl = plan.rate_weights(), rf._block_res(plan), plan.blocks()
        ws = [float(w[0, res[j], int(b["band"])]) for j, b in enumerate(bl)]
        wins = rf._windows(plan, ctiles, Cn)
        vals = _block_values(plan, coeff.cpu().numpy())
        fw = roi.frame_windows(bl, Cn, W, H, tile, nres, q, "53")
        for frac in E["budgets"]:
            B = int(U * frac)
            err = {}
            for g in E["gains"]:
                ps, chosen = rc.allocate(R, roi.frame_distortion(vals, nbs, fw, g), nbs, ws, B)
                assert chosen <= B
                kw = dict(roi=q, roi_gain=g) if g > 1 else {}
                cs, toffs = plan.encode_frame_pixels(fmt, d_pix, max_body_bytes=B, **kw)
                plan.frame_status()
                back = torch.full(pix.shape, 0x5A, dtype=torch.uint8, device=plan.device)
                plan.decode_frame_pixels(cs, int(toffs[-1].item()), back, truncated=True)
                plan.frame_status()
                got = back.cpu().numpy()
                assert np.array_equal(got, rf._expected_pixels(orc, case, True, 0, ctiles, wins, [nb - p for nb, p in zip(nbs, ps)], 0)), (frac, g)
                err[g] = roi.split_error(got[:, :W], pix[:, :W], q)
            print("budget %.0f %% (%d of %d bytes): inside %d -> %d, outside %d -> %d" % (100 * frac, B, U, err[1][0], err[16][0], err[1][1], err[16][1]))
            assert err[16][0] < err[1][0], frac
            assert err[16][1] >= err[1][1], frac
    finally:
        plan.close()


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------------
def test_graph(env):
    """one roi frame encode captured after a warm call, replayed on a second frame: the rectangle and the gain are arguments of the captured
    launches, the frame is what the buffer holds"""
    torch, orc, _ = env
    from j2kgfx import Context
    spec, q = FRAME_SPECS[0]
    (W, H, Cn, prec, tile, nres) = spec[0]
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    ctx = Context(0)
    plan = tl._plan(ctx, spec)
    try:
        frames, wants = [], []
        for seed in (81, 82):
            pix, _, _, _ = ref.pixel_frame(fmt, W, H, seed, orc, noise=(1 << prec) // 16)
            d = torch.from_numpy(pix).to(plan.device)
            cs, toffs = plan.encode_frame_pixels(fmt, d, sop=True, eph=True, max_body_bytes=3000, roi=q, roi_gain=16)
            plan.frame_status()
            frames.append(d)
            wants.append(_bytes(cs, toffs))
        assert wants[0] != wants[1]
        d_pix = frames[0].clone()
        out = torch.zeros(plan.frame_bound(), dtype=torch.uint8, device=plan.device)
        toffs = torch.zeros(int(plan.info.tiles) + 1, dtype=torch.int64, device=plan.device)
        kw = dict(sop=True, eph=True, out=out, tile_offs=toffs, max_body_bytes=3000, roi=q, roi_gain=16)
        with ctx.capture() as gr:
            plan.encode_frame_pixels(fmt, d_pix, **kw)
        for i in (1, 0, 1):
            d_pix.copy_(frames[i])
            out.zero_()
            torch.cuda.synchronize()
            gr.launch()
            ctx.sync()
            assert _bytes(out, toffs) == wants[i], i
        gr.close()
    finally:
        plan.close()
        ctx.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    torch, orc, ctx = env
    from j2kgfx import J2KError, _lib
    from j2kgfx.codec import FramePlan
    (W, H, Cn, prec, tile, nres), cb = roi.GEOMETRIES[0]
    q = (37, 11, 90, 40)

    def mk(**kw):
        kw.setdefault("mallat", True)
        c = kw.pop("cb", cb)
        return FramePlan(W, kw.pop("height", H), Cn, precision=prec, lossless=True, num_resolutions=nres, cb=(c, c), tile=kw.pop("tile", tile), coder=kw.pop("coder", 0),
                         ctx=ctx, **kw)

    def status(fn):
        try:
            fn()
        except J2KError as e:
            assert str(e)
            return e.status
        return _lib.OK

    def every_call(p, rect, gain, windows=True):
        """the status of every roi entry of plan p (all must agree); every output buffer keeps its fill pattern"""
        n, nt, Hp = int(p.info.blocks), int(p.info.tiles), int(p.height)
        dev = lambda k, dt=torch.uint8: torch.full((max(int(k), 4) * torch.empty((), dtype=dt).element_size(),), FILL, dtype=torch.uint8, device=p.device).view(dt)
        pix = torch.zeros((Hp, W * 4), dtype=torch.uint8, device=p.device)
        h_pix = np.zeros((Hp, W * 4), np.uint8)
        coeff = torch.zeros(max(int(p.info.coeff_elems), 4), dtype=torch.int32, device=p.device)
        win, slots, lens, nbs = dev(4 * n, torch.int32), dev(p.info.bytes_cap), dev(n, torch.int32), dev(n)
        out, toffs = dev(1 << 16), dev(nt + 1, torch.int64)
        st = set()
        if windows:
            st.add(status(lambda: p.roi_windows(rect, win=win.view(-1, 4))))
        st.add(status(lambda: p.encode_blocks(coeff, slots=slots, lens=lens, numbps=nbs, planes=True, roi=rect, roi_gain=gain)))
        st.add(status(lambda: p.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, tile_offs=toffs, max_body_bytes=1000, roi=rect, roi_gain=gain)))
        st.add(status(lambda: p.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, tile_offs=toffs, layer_bytes=[500, 1000], roi=rect, roi_gain=gain)))
        st.add(status(lambda: p.encode_pixels_host(_lib.PIX_RGBA8, h_pix, max_body_bytes=1000, roi=rect, roi_gain=gain)))
        st.add(status(lambda: p.encode_pixels_host(_lib.PIX_RGBA8, h_pix, layer_bytes=[500, 1000], roi=rect, roi_gain=gain)))
        ctx.sync()
        for t in (win, slots, lens, nbs, out, toffs):
            assert bool((t.view(torch.uint8) == FILL).all())
        assert len(st) == 1, st
        return st.pop()

    plan = mk()
    others = dict(ht=mk(coder=1), no_closed_loop=mk(mallat=False), batch=mk(height=2 * H, frame_rows=H, tile=(0, 0)), blocks_128=mk(cb=128, tile=(0, 0)),
                  prefix=mk(mallat=False, closed_loop=True), shard=mk(tile_first=1, tile_count=2))
    try:
        for name, p in others.items():
            assert every_call(p, q, 16) == _lib.ERR_UNSUPPORTED, name
        for a in ((90, 11, 37, 40), (37, 40, 90, 11), (37, 11, 37, 40), (37, 11, 90, 11), (-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, W + 1, 4), (0, 0, 4, H + 1), (W, 0, W + 1, 4)):
            assert every_call(plan, a, 16) == _lib.ERR_INVALID_ARG, a
        for gain in (0, -1, 65536):
            assert every_call(plan, q, gain, windows=False) == _lib.ERR_INVALID_ARG, gain
        # budgets: none (the binding raises before the call; the C entries refuse a null pointer), and what the _layers call refuses of them
        pix = torch.zeros((H, W * 4), dtype=torch.uint8, device=plan.device)
        h_pix = np.zeros((H, W * 4), np.uint8)
        out = torch.full((1 << 16,), FILL, dtype=torch.uint8, device=plan.device)
        toffs = torch.full(((int(plan.info.tiles) + 1) * 8,), FILL, dtype=torch.uint8, device=plan.device).view(torch.int64)
        loffs = torch.full((int(plan.info.tiles) * 32 * 8,), FILL, dtype=torch.uint8, device=plan.device).view(torch.int64)
        with pytest.raises(ValueError):
            plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, tile_offs=toffs, roi=q)
        with pytest.raises(ValueError):
            plan.encode_pixels_host(_lib.PIX_RGBA8, h_pix, roi=q)
        with pytest.raises(ValueError):
            plan.encode_blocks(torch.zeros(int(plan.info.coeff_elems), dtype=torch.int32, device=plan.device), roi=q)
        rect = _lib.Rect(*q)
        L = ctx.L

        def frame_call(arr, nl, layered=True):
            return L.j2k_plan_encode_frame_pixels_roi(plan.h, _lib.PIX_RGBA8, plan._p(pix), C.c_size_t(W * 4), 0, 0, arr, nl, C.byref(rect), 16, plan._p(out),
                                                      C.c_size_t(int(out.numel())), plan._p(toffs), plan._p(loffs) if layered else None)

        def host_call(arr, nl, layered=True):
            hout, olen = np.full(1 << 16, FILL, np.uint8), C.c_size_t(0)
            r = L.j2k_encode_pixels_host_roi(plan.h, _lib.PIX_RGBA8, h_pix.ctypes.data_as(C.c_void_p), C.c_size_t(W * 4), 0, 0, arr, nl, C.byref(rect), 16,
                                             hout.ctypes.data_as(C.c_void_p), C.c_size_t(hout.size), C.byref(olen), None,
                                             np.zeros(int(plan.info.tiles) * 32, np.uint64).ctypes.data_as(C.c_void_p) if layered else None, None, None)
            assert (hout == FILL).all()
            return r
        i64 = lambda *v: (C.c_int64 * len(v))(*v)
        for arr, nl, layered in ((None, 1, False), (None, 2, True), (i64(1000), 0, True), (i64(*([1000] * 33)), 33, True), (i64(-1), 1, False), (i64(1000, 999), 2, True),
                                 (i64(500, 1000), 2, False)):
            assert frame_call(arr, nl, layered) == _lib.ERR_INVALID_ARG, (nl, layered)
            assert host_call(arr, nl, layered) == _lib.ERR_INVALID_ARG, (nl, layered)
        assert L.j2k_plan_encode_frame_pixels_roi(plan.h, _lib.PIX_RGBA8, plan._p(pix), C.c_size_t(W * 4), 0, 0, i64(1000), 1, None, 16, plan._p(out),
                                                  C.c_size_t(int(out.numel())), plan._p(toffs), None) == _lib.ERR_INVALID_ARG
        ctx.sync()
        for t in (out, toffs, loffs):
            assert bool((t.view(torch.uint8) == FILL).all())
        # and the plan still works
        assert status(lambda: plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, max_body_bytes=1000, roi=q)) == _lib.OK
        plan.frame_status()
    finally:
        plan.close()
        for p in others.values():
            p.close()
