"""GPU: the quality-targeted MQ encode against tests/quality_cases.py -- rate_allocate_quality bit for bit (kept, chosen, achieved as raw
float64 bits) on the device's own tables and on synthetic ones, its duality with rate_allocate, the frame calls encode_frame_pixels(min_psnr= /
max_distortion= / layer_psnr= / layer_distortion=) and encode_pixels_host against the stage calls byte for byte, the round trip through the
truncated / layered decoders against the oracle composition of the rate and layer tests, roi=, the refusals, and pixels.sse / pixels.psnr.

Frames: 8-bit RGB, 8 x 8 blocks, Mallat closed-loop MQ plans; 64 x 48 with 2 resolutions (144 blocks: fewer than one per thread of the
allocation's workgroup) and 192 x 128 with 3 (1 152 blocks: some threads hold two, and the count is no multiple of 1024); the 5-3 and the
9-7 at quality 20."""
import numpy as np
import pytest

import layer_cases as lc
import quality_cases as qc
import rate_cases as rc
import roi_cases as roi
import test_gpu_layers as tl
import test_gpu_rate_frames as rf
import test_gpu_roi_encode as tr

pytestmark = pytest.mark.gpu
Q97 = 20
FILL = 0x77
SMALL, LARGE = (64, 48, 3, 8, (0, 0), 2), (192, 128, 3, 8, (0, 0), 3)
SPECS = [(SMALL, True, 0, 8), (SMALL, False, Q97, 8), (LARGE, True, 0, 8), (LARGE, False, Q97, 8)]
SPEC_IDS = ["64x48-53", "64x48-97q20", "192x128-53", "192x128-97q20"]
BLOCKS = {SMALL: 144, LARGE: 1152}
ROI = (20, 12, 44, 36)


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    from j2kgfx import Context
    ctx = Context(0)
    yield torch, orc, ctx
    ctx.close()


_FRAMES = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_freed_device_memory_zeroed():
    """This module frees small device tensors full of bytes with the top bit set (pixel rows of 0xFF, distortions near 2^63, code-stream
    bytes).  torch's caching allocator hands such blocks on as they are to the next torch.empty of a later module, and an output tensor that
    a test reads before the library's stream has written it then shows this module's bytes.  So at the end the module zeroes every free
    block of the allocator's small pool: best fit gives a request of a free block's exact size that block (blocks above the 1 MiB request
    limit of the pool are taken 1 MiB at a time)."""
    yield
    import torch
    torch.cuda.synchronize()
    held = []
    for _ in range(4):
        sizes = sorted(b["size"] for seg in torch.cuda.memory_snapshot() if seg["segment_type"] == "small"
                       for b in seg["blocks"] if b["state"] == "inactive")
        if not sizes:
            break
        held += [torch.zeros(min(s, 1 << 20), dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    del held


@pytest.fixture()
def shared(env, request):
    """(spec, plan, test_gpu_layers.Frame + the definition's hulls): the Frame once per spec, the plan the test's own"""
    torch, orc, ctx = env
    spec = SPECS[request.param]
    plan = tl._plan(ctx, spec)
    try:
        if request.param not in _FRAMES:
            F = tl.Frame(torch, plan, spec)
            assert F.n == BLOCKS[spec[0]]
            F.H = qc.Hulls(F.R, F.D, F.nbs, F.ws)
            F.start = F.H.choice((1 << 63) - 1)                     # the start points: (kept, bytes, S)
            F.cache = {}
            _FRAMES[request.param] = F
        yield spec, plan, _FRAMES[request.param]
    finally:
        plan.close()


def _want(F, T):
    key = qc.float_bits(T)
    if key not in F.cache:
        F.cache[key] = F.H.search(T)
    return F.cache[key]


def _bits(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def _bytes(cs, toffs):
    return bytes(cs.cpu().numpy()[:int(toffs[-1].item())])


def _tables(plan, F):
    return plan.encode_blocks(plan.forward_pixels(F.fmt, F.d_pix), planes=True)


def _attainable(F, frac):
    """(T, cuts, bytes) of the byte budget frac * U by rate_cases.allocate: an exactly attainable S"""
    ps, b = rc.allocate(F.R, F.D, F.nbs, F.ws, int(F.U * frac))
    return qc.weighted_distortion(F.D, F.ws, ps), ps, b


def _layer_targets(F, L):
    """L falling targets from above the start-point sum down to 0"""
    s0 = F.start[2]
    return [s0 * 2.0] + [s0 * 4.0 ** -l for l in range(1, L - 1)] + [0.0] if L > 1 else [s0 / 50.0]


def _check_alloc(plan, tables, H, targets, n):
    slots, lens, nbs, rate, dist = tables
    kept, chosen, achieved = plan.rate_allocate_quality(rate, dist, nbs, targets)
    plan.ctx.sync()
    want = [H.search(T) for T in targets]
    assert kept.shape == (len(targets), n)
    for l, (ps, b, S) in enumerate(want):
        print("layer %d: target %r -> bytes %d (device %d), S %r (device %r)" % (l, targets[l], b, int(chosen[l].item()), S, float(achieved[l].item())))
        assert kept[l].cpu().numpy().tolist() == ps, l
        assert int(chosen[l].item()) == b, l
        assert _bits(achieved)[l] == qc.float_bits(S) and S <= targets[l], l
    return want


# ---- 1. the stage call against the definition, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", range(len(SPECS)), ids=SPEC_IDS, indirect=True)
def test_allocate_quality_on_the_devices_tables(env, shared):
    torch, orc, ctx = env
    spec, plan, F = shared
    tables = _tables(plan, F)
    T_att, ps_att, b_att = _attainable(F, 0.3)
    s0 = F.start[2]
    assert s0 > 0.0 and 0.0 < T_att < s0
    for T in (0.0, s0 * 1.5, s0, T_att, float(np.nextafter(T_att, 0.0)), s0 / 1000.0):
        _check_alloc(plan, tables, F.H, [T], F.n)
    for L in (3, 32):
        want = _check_alloc(plan, tables, F.H, _layer_targets(F, L), F.n)
        assert want[0][0] == F.start[0] and want[0][1] == 0                       # above the start-point sum: nothing coded
        assert want[-1][1] == F.U or want[-1][2] == 0.0                           # target 0: no distortion left
        assert len({tuple(w[0]) for w in want}) >= 3, "vacuous: the layers do not differ"
    got = _want(F, T_att)
    assert got[0] == ps_att and got[1] <= b_att and any(0 < p < nb for p, nb in zip(got[0], F.nbs))


@pytest.mark.parametrize("shared", [0, 2], ids=[SPEC_IDS[0], SPEC_IDS[2]], indirect=True)
def test_allocate_quality_on_synthetic_tables(env, shared):
    """tables uploaded in the place of the device's: D near 2^63 (uint64 -> float64 rounds), blocks of no planes, bands of weight 0"""
    torch, orc, ctx = env
    spec, plan, F = shared
    (W, H, Cn, prec, tile, nres) = spec[0]
    w = plan.rate_weights().copy()
    w[1, :, :] *= 0.7071067811865476
    w[2, nres - 1, 1] = 0.0                                                       # a band of weight 0
    w[0, 0, 0] = 0.0
    plan.set_rate_weights(w)
    res, bl = rf._block_res(plan), plan.blocks()
    ws = [float(w[int(b["plane"]) % Cn, res[j], int(b["band"])]) for j, b in enumerate(bl)]
    Rs, Ds, nbs, _ = qc.random_tables(77 + F.n, F.n, big=True)
    assert 0 in nbs and 0.0 in ws and max(int(D[0]) for D in Ds) > (1 << 63) - (1 << 21)
    rate = torch.from_numpy(np.stack(Rs).view(np.int32)).to(plan.device)
    dist = torch.from_numpy(np.stack(Ds).view(np.int64)).to(plan.device)
    d_nbs = torch.from_numpy(np.array(nbs, np.uint8)).to(plan.device)
    Hs = qc.Hulls(Rs, Ds, nbs, ws)
    s0 = Hs.choice((1 << 63) - 1)[2]
    ps, b = rc.allocate(Rs, Ds, nbs, ws, sum(int(R[nb]) for R, nb in zip(Rs, nbs)) // 3)
    T_att = qc.weighted_distortion(Ds, ws, ps)
    tables = (None, None, d_nbs, rate, dist)
    for T in (0.0, s0 * 2.0, T_att, s0 / 3.0):
        want = _check_alloc(plan, tables, Hs, [T], F.n)
    zero = Hs.search(0.0)[0]
    assert all(int(Rs[j][zero[j]]) == 0 for j in range(F.n) if ws[j] == 0.0)      # weight 0: dropped entirely
    assert Hs.search(T_att)[0] == ps
    for L in (3, 32):
        _check_alloc(plan, tables, Hs, [s0 * 2.0] + [s0 * 3.0 ** -l for l in range(1, L - 1)] + [0.0], F.n)


# ---- 2. duality on the device ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", range(len(SPECS)), ids=SPEC_IDS, indirect=True)
def test_duality_with_rate_allocate(env, shared):
    torch, orc, ctx = env
    spec, plan, F = shared
    slots, lens, nbs, rate, dist = _tables(plan, F)
    cut = 0
    for frac in (0.05, 0.2, 0.5, 0.8):
        kept_b, chosen_b = plan.rate_allocate(rate, dist, nbs, int(F.U * frac))
        plan.ctx.sync()
        ps = kept_b.cpu().numpy()[:F.n].tolist()
        if ps == F.nbs:
            continue
        cut += 1
        T = qc.weighted_distortion(F.D, F.ws, ps)                                  # achieved of that choice
        kept, chosen, achieved = plan.rate_allocate_quality(rate, dist, nbs, [T])
        plan.ctx.sync()
        assert kept[0].cpu().numpy().tolist() == ps, frac
        assert _bits(achieved)[0] == qc.float_bits(T) and int(chosen[0].item()) <= int(chosen_b.item()), frac
    assert cut >= 3


# ---- 3. bytes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", range(len(SPECS)), ids=SPEC_IDS, indirect=True)
def test_frame_bytes(env, shared):
    torch, orc, ctx = env
    spec, plan, F = shared
    slots, lens, nbs, rate, dist = _tables(plan, F)
    offs, stream = plan.compact(slots, lens)
    # target 0 on default weights: nothing is cut
    for marks in (False, True):
        full, ftoffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, max_body_bytes=2 ** 62)
        zero, ztoffs, zach = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, max_distortion=0)
        plan.frame_status()
        assert _bytes(zero, ztoffs) == _bytes(full, ftoffs) and _bits(zach) == [0]
    # one target: the stream of the stage calls fed the definition's cuts; dB and T ask the same thing; the host call agrees
    T_att = _attainable(F, 0.3)[0]
    db = 38.0
    T_db = plan.psnr_distortion(db)
    (W, H, Cn, prec, tile, nres), lossless, q, cb = spec
    assert T_db == pytest.approx(qc.psnr_distortion(W, H, Cn, prec, lossless, q, db), rel=1e-12)
    for T, marks in ((T_att, False), (T_db, True), (F.start[2] * 2.0, True)):
        ps, b, S = _want(F, T)
        d_kept = torch.from_numpy(np.array(ps, np.uint8)).to(plan.device)
        stage, stoffs = plan.encode_tile_parts(stream, offs, lens, nbs, sop=marks, eph=marks, kept=d_kept, rate=rate)
        cs, toffs, ach = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, max_distortion=T)
        plan.frame_status()
        assert _bytes(cs, toffs) == _bytes(stage, stoffs) and toffs.cpu().numpy().tolist() == stoffs.cpu().numpy().tolist()
        assert _bits(ach) == [qc.float_bits(S)]
        host = plan.encode_pixels_host(F.fmt, F.pix, sop=marks, eph=marks, max_distortion=T)
        assert bytes(host["bytes"]) == _bytes(cs, toffs) and host["tile_offs"].tolist() == toffs.cpu().numpy().tolist() and "layer_offs" not in host
        assert host["achieved"].view(np.uint64).tolist() == [qc.float_bits(S)]
        assert host["lens"].tolist() == F.lens and host["numbps"].tolist() == F.nbs
    by_db, dtoffs, dach = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=True, eph=True, min_psnr=db)
    by_T, ttoffs, tach = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=True, eph=True, max_distortion=T_db)
    plan.frame_status()
    assert _bytes(by_db, dtoffs) == _bytes(by_T, ttoffs) and _bits(dach) == _bits(tach)
    assert 0 < _want(F, T_db)[1] < F.U, "vacuous: 38 dB cuts nothing or everything"
    # layers: the layered stream of the stage calls
    for L, marks in ((3, False), (32, True)):
        targets = _layer_targets(F, L)
        kept = [_want(F, T)[0] for T in targets]
        d_kept = torch.from_numpy(np.array(kept, np.uint8)).to(plan.device)
        stage, stoffs, sloffs = plan.encode_tile_parts(stream, offs, lens, nbs, sop=marks, eph=marks, kept=d_kept, rate=rate, layers=L)
        cs, toffs, loffs, ach = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=marks, eph=marks, layer_distortion=targets)
        plan.frame_status()
        assert _bytes(cs, toffs) == _bytes(stage, stoffs) and loffs.cpu().numpy().tolist() == sloffs.cpu().numpy().tolist()
        assert _bits(ach) == [qc.float_bits(_want(F, T)[2]) for T in targets]
        host = plan.encode_pixels_host(F.fmt, F.pix, sop=marks, eph=marks, layer_distortion=targets)
        assert bytes(host["bytes"]) == _bytes(cs, toffs) and host["layer_offs"].tolist() == loffs.cpu().numpy().tolist()
        assert host["achieved"].view(np.uint64).tolist() == _bits(ach)
    dbs = [30.0, 38.0, 46.0]
    a = plan.encode_frame_pixels(F.fmt, F.d_pix, layer_psnr=dbs)
    b = plan.encode_frame_pixels(F.fmt, F.d_pix, layer_distortion=[plan.psnr_distortion(d) for d in dbs])
    plan.frame_status()
    assert _bytes(a[0], a[1]) == _bytes(b[0], b[1]) and _bits(a[3]) == _bits(b[3])


# ---- 4. round trip ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", range(len(SPECS)), ids=SPEC_IDS, indirect=True)
def test_round_trip(env, shared):
    """the decoders are untouched: truncated=True / layers=k of the quality streams give the oracle composition for the definition's cuts"""
    torch, orc, ctx = env
    spec, plan, F = shared
    T = plan.psnr_distortion(36.0)
    ps = _want(F, T)[0]
    cs, toffs, ach = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=True, eph=True, min_psnr=36.0)
    plan.frame_status()
    exp = F.expected(orc, spec, ps, 0, 0)
    back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
    plan.decode_frame_pixels(cs, int(toffs[-1].item()), back, sop=True, eph=True, truncated=True)
    plan.frame_status()
    assert np.array_equal(back.cpu().numpy(), exp)
    host = plan.decode_pixels_host(_bytes(cs, toffs), exp.shape, sop=True, eph=True, truncated=True)
    assert np.array_equal(host, exp)
    targets = [plan.psnr_distortion(d) for d in (28.0, 36.0, 44.0)]
    kept = [_want(F, t)[0] for t in targets]
    Q = list(zip(*[lc.normalise(F.R[j], [kept[l][j] for l in range(3)]) for j in range(F.n)]))
    cs, toffs, loffs, ach = plan.encode_frame_pixels(F.fmt, F.d_pix, layer_distortion=targets)
    plan.frame_status()
    for k in (1, 2, 3):
        exp = F.expected(orc, spec, Q[k - 1], 0, 0)
        back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, int(toffs[-1].item()), back, layers=k)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp), k
    assert Q[0] != Q[1] != Q[2]


@pytest.mark.parametrize("shared", [0, 1], ids=SPEC_IDS[:2], indirect=True)
def test_roi_tables_feed_the_same_search(env, shared):
    """roi=: the search runs on D_roi of tests/roi_cases.py, everything else is unchanged"""
    torch, orc, ctx = env
    spec, plan, F = shared
    (W, H, Cn, prec, tile, nres) = spec[0]
    coeff = plan.forward_pixels(F.fmt, F.d_pix)
    plan.ctx.sync()
    wins = roi.frame_windows(plan.blocks(), Cn, W, H, tile, nres, ROI, "53" if spec[1] else "97")
    Droi = roi.frame_distortion(tr._block_values(plan, coeff.cpu().numpy()), F.nbs, wins, 16)
    Hr = qc.Hulls(F.R, Droi, F.nbs, F.ws)
    T = plan.psnr_distortion(34.0)
    ps, b, S = Hr.search(T)
    assert ps != _want(F, T)[0], "vacuous: the weight moved nothing"
    slots, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True, roi=ROI, roi_gain=16)
    offs, stream = plan.compact(slots, lens)
    d_kept = torch.from_numpy(np.array(ps, np.uint8)).to(plan.device)
    stage, stoffs = plan.encode_tile_parts(stream, offs, lens, nbs, kept=d_kept, rate=rate)
    cs, toffs, ach = plan.encode_frame_pixels(F.fmt, F.d_pix, min_psnr=34.0, roi=ROI, roi_gain=16)
    plan.frame_status()
    assert _bytes(cs, toffs) == _bytes(stage, stoffs) and _bits(ach) == [qc.float_bits(S)]
    host = plan.encode_pixels_host(F.fmt, F.pix, min_psnr=34.0, roi=ROI, roi_gain=16)
    assert bytes(host["bytes"]) == _bytes(cs, toffs)
    one = plan.encode_frame_pixels(F.fmt, F.d_pix, min_psnr=34.0, roi=ROI, roi_gain=1)
    plain = plan.encode_frame_pixels(F.fmt, F.d_pix, min_psnr=34.0)
    plan.frame_status()
    assert _bytes(one[0], one[1]) == _bytes(plain[0], plain[1])                     # gain 1 weighs nothing
    targets = [plan.psnr_distortion(d) for d in (28.0, 40.0)]
    kept = [Hr.search(t)[0] for t in targets]
    stage, stoffs, sloffs = plan.encode_tile_parts(stream, offs, lens, nbs, kept=torch.from_numpy(np.array(kept, np.uint8)).to(plan.device), rate=rate, layers=2)
    cs, toffs, loffs, ach = plan.encode_frame_pixels(F.fmt, F.d_pix, layer_psnr=(28.0, 40.0), roi=ROI, roi_gain=16)
    plan.frame_status()
    assert _bytes(cs, toffs) == _bytes(stage, stoffs) and loffs.cpu().numpy().tolist() == sloffs.cpu().numpy().tolist()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why,kw", [
    ("ht", dict(coder=1)),
    ("batch", dict(frame_rows=35)),
    ("blocks_128", dict(cb=128)),
    ("no_closed_loop", dict(mallat=False)),
    ("prefix_roi", dict(mallat=False, closed_loop=True, roi=(8, 8, 40, 40))),
    ("shard_roi", dict(tile=(64, 32), tile_first=1, tile_count=2, roi=(8, 8, 40, 40))),
])
def test_plan_refusals(env, why, kw):
    """what rate_check / roi_check refuse of a plan, with their code, before the first launch"""
    torch, orc, ctx = env
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    from j2kgfx.codec import FramePlan
    kw = dict(kw)
    cb, r = kw.pop("cb", 64), kw.pop("roi", None)
    plan = FramePlan(130, 70, 3, precision=8, lossless=True, num_resolutions=4, cb=(cb, cb), coder=kw.pop("coder", 0), ctx=ctx, mallat=kw.pop("mallat", True), **kw)
    try:
        pix = torch.zeros((70, 130 * 4), dtype=torch.uint8, device=plan.device)
        out = torch.full((1 << 16,), FILL, dtype=torch.uint8, device=plan.device)
        for q in (dict(max_distortion=1000.0), dict(min_psnr=40.0), dict(layer_distortion=[2000.0, 1000.0]), dict(layer_psnr=[30.0, 40.0])):
            with pytest.raises(J2KError) as e:
                plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, roi=r, **q)
            assert e.value.status == _lib.ERR_UNSUPPORTED, q
            with pytest.raises(J2KError) as e:
                plan.encode_pixels_host(_lib.PIX_RGBA8, pix.cpu().numpy(), roi=r, **q)
            assert e.value.status == _lib.ERR_UNSUPPORTED, q
        if r is None:
            n = max(int(plan.info.blocks), 1)
            z = torch.zeros((n, 32), dtype=torch.int64, device=plan.device)
            with pytest.raises(J2KError) as e:
                plan.rate_allocate_quality(z.to(torch.int32), z, torch.zeros(n, dtype=torch.uint8, device=plan.device), [1.0])
            assert e.value.status == _lib.ERR_UNSUPPORTED
        ctx.sync()
        assert bool((out == FILL).all())
    finally:
        plan.close()


def test_argument_refusals(env):
    """targets that are negative, NaN, infinite or rising, L outside 1 ... 32, a bad rectangle or gain: J2K_ERR_INVALID_ARG before the first
    launch; a quality argument beside a byte budget or beside another one: ValueError"""
    torch, orc, ctx = env
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    plan = tl._plan(ctx, SPECS[0])
    try:
        n = int(plan.info.blocks)
        pix = torch.zeros((48, 64 * 4), dtype=torch.uint8, device=plan.device)
        out = torch.full((1 << 16,), FILL, dtype=torch.uint8, device=plan.device)
        kept = torch.full((33 * n,), FILL, dtype=torch.uint8, device=plan.device)
        z = torch.zeros((n, 32), dtype=torch.int64, device=plan.device)
        nbs = torch.zeros(n, dtype=torch.uint8, device=plan.device)
        inf, nan = float("inf"), float("nan")
        bad = [dict(max_distortion=-1.0), dict(max_distortion=nan), dict(max_distortion=inf), dict(min_psnr=nan), dict(min_psnr=inf), dict(min_psnr=-inf),
               dict(layer_distortion=[1.0, 2.0]), dict(layer_distortion=[5.0, -0.5]), dict(layer_distortion=[inf, 1.0]), dict(layer_distortion=[]),
               dict(layer_distortion=[1.0] * 33), dict(layer_psnr=[40.0, 30.0]), dict(layer_psnr=[30.0, nan]), dict(layer_psnr=[]),
               dict(min_psnr=40.0, roi=(10, 10, 10, 20)), dict(min_psnr=40.0, roi=(0, 0, 65, 10)), dict(max_distortion=1.0, roi=(0, 0, 8, 8), roi_gain=0),
               dict(layer_psnr=[30.0], roi=(0, 0, 8, 8), roi_gain=65536)]
        for q in bad:
            with pytest.raises(J2KError) as e:
                plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, **q)
            assert e.value.status == _lib.ERR_INVALID_ARG, q
            with pytest.raises(J2KError) as e:
                plan.encode_pixels_host(_lib.PIX_RGBA8, pix.cpu().numpy(), **q)
            assert e.value.status == _lib.ERR_INVALID_ARG, q
        for targets in ([-1.0], [nan], [inf], [1.0, 2.0], [], [0.0] * 33):
            with pytest.raises(J2KError) as e:
                plan.rate_allocate_quality(z.to(torch.int32), z, nbs, targets, kept=kept)
            assert e.value.status == _lib.ERR_INVALID_ARG, targets
        for q in (dict(min_psnr=40.0, max_body_bytes=100), dict(max_distortion=1.0, layer_bytes=[1, 2]), dict(min_psnr=40.0, max_distortion=1.0),
                  dict(layer_psnr=[30.0], layer_distortion=[1.0]), dict(min_psnr=40.0, layer_psnr=[30.0]), dict(layer_distortion=[1.0], layer_bytes=[5])):
            with pytest.raises(ValueError):
                plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, **q)
            with pytest.raises(ValueError):
                plan.encode_pixels_host(_lib.PIX_RGBA8, pix.cpu().numpy(), **q)
        with pytest.raises(J2KError) as e:
            plan.psnr_distortion(nan)
        assert e.value.status == _lib.ERR_INVALID_ARG
        ctx.sync()
        assert bool((out == FILL).all()) and bool((kept == FILL).all())
    finally:
        plan.close()


# ---- 6. pixels.sse / pixels.psnr ----------------------------------------------------------------------------------------------------------------------
def _np_sse(fmt, a, b, w, h, bpp, wide, nch):
    out = []
    for c in range(nch):
        if wide:
            sa = a[:h, :w * bpp].reshape(h, w * bpp // 2, 2).astype(np.int64)
            sb = b[:h, :w * bpp].reshape(h, w * bpp // 2, 2).astype(np.int64)
            va, vb = sa[..., 0] * 256 + sa[..., 1], sb[..., 0] * 256 + sb[..., 1]
        else:
            va, vb = a[:h, :w * bpp].astype(np.int64), b[:h, :w * bpp].astype(np.int64)
        out.append(int(((va[:, c::nch] - vb[:, c::nch]) ** 2).sum()))
    return out


@pytest.mark.parametrize("fmt", range(6), ids=["gray8", "gray16", "rgba8", "rgba64", "nrgba8", "nrgba64"])
def test_pixels_sse(env, fmt):
    """all six formats against numpy, exactly: widths with a ragged 16-byte tail, rows longer than a wavefront's 1024-byte chunk, strides above
    w * bpp (16-byte aligned rows and unaligned ones), frames that differ in one sample of the last row"""
    torch, orc, ctx = env
    from j2kgfx import pixels
    bpp = {0: 1, 1: 2, 2: 4, 3: 8, 4: 4, 5: 8}[fmt]
    wide, nch = fmt in (1, 3, 5), 1 if fmt < 2 else 4
    rng = np.random.default_rng(5 + fmt)
    for w, h, pad_a, pad_b in ((1, 1, 0, 0), (1, 3, 16 - bpp, 16 - bpp), (5, 4, 0, 3), (67, 9, 16 * 70 - 67 * bpp, 16 * 80 - 67 * bpp), (67, 5, 1, 0),
                               (300, 33, 0, 0), (1030, 3, 32 * 1030 - 1030 * bpp, 0)):
        a = rng.integers(0, 256, (h, w * bpp + pad_a), dtype=np.uint8)
        b = rng.integers(0, 256, (h, w * bpp + pad_b), dtype=np.uint8)
        d_a, d_b = torch.from_numpy(a).to("cuda:%d" % ctx.device), torch.from_numpy(b).to("cuda:%d" % ctx.device)
        want = _np_sse(fmt, a, b, w, h, bpp, wide, nch)
        got = pixels.sse(fmt, d_a, d_b, w, h, ctx=ctx)
        assert got.dtype == np.uint64 and got.tolist() == want, (w, h, pad_a, pad_b)
        assert pixels.sse(fmt, d_a, d_a, w, h, ctx=ctx).tolist() == [0] * nch
        assert pixels.psnr(fmt, d_a, d_a, w, h, ctx=ctx) == float("inf")
        colour = want[:1] if nch == 1 else want[:3]
        if sum(colour):
            assert pixels.psnr(fmt, d_a, d_b, w, h, ctx=ctx) == pytest.approx(qc.psnr(sum(colour), w * h * len(colour), 65535 if wide else 255), rel=1e-12)
        # one sample of the last row differs (its low byte, by 3): the last channel of the last pixel
        c = a.copy()
        c[h - 1, w * bpp - 1] = (int(c[h - 1, w * bpp - 1]) + 3) % 256 if int(c[h - 1, w * bpp - 1]) <= 252 else int(c[h - 1, w * bpp - 1]) - 3
        one = pixels.sse(fmt, d_a, torch.from_numpy(c).to(d_a.device), w, h, ctx=ctx).tolist()
        assert one == [0] * (nch - 1) + [9], (w, h)
        # all-different extremes: the sums stay exact
        lo, hi = np.zeros_like(a), np.full_like(a, 255)
        full = pixels.sse(fmt, torch.from_numpy(lo).to(d_a.device), torch.from_numpy(hi).to(d_a.device), w, h, ctx=ctx).tolist()
        assert full == [w * h * (65535 ** 2 if wide else 255 ** 2)] * nch
    with pytest.raises(Exception):
        pixels.sse(fmt, d_a, d_b, w, h + 1, ctx=ctx)
