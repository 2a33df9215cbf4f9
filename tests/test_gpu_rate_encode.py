"""GPU: the rate-limited MQ encode against tests/rate_cases.py, bit for bit.

  block tables   the shapes of coarse_cases.ONE_LAUNCH_SHAPES (4- / 8- / 16-bit data dense and 80 % zeros, a zero block, a 1-plane block), each as
                 the single block of a closed-loop plan, through the split path (context kernel + lanes kernel) and the one-kernel path: bytes,
                 lens and numbps are the oracle's, D is numpy's, R[0] = 0, R[nb] = len, R is monotone, and every (block, plane) has the prefix
                 property with the oracle's decoder.  The slack of R over the shortest valid prefix is printed, not asserted (measured: mean
                 2.94 bytes, 0 ... 5, over 300 pairs; docs/KERNEL_NOTES.md 4u).
  frames         coarse_cases.FRAME_CASES as Mallat plans with 8 blocks per wavefront of the lanes kernel: the same checks on every block; and a
                 symbol workspace too small for some blocks' planes (they fall to the one-kernel form)
  allocation     on those frames' tables the device's kept planes and chosen bytes equal rate_cases.allocate for budgets of 0, 1, 10 %, 50 %,
                 100 % of the total and the total + 1; hand-made tables (no more bytes, rising distortion, equal slopes) the same
  weights        plan.rate_weights() is rate_cases.default_weights; set / restore
  refusals       HT, batch, 128 x 128 blocks, no closed loop: J2K_ERR_UNSUPPORTED; a negative budget: J2K_ERR_INVALID_ARG
  decoder forms  a floor per block, floors[j] = (7 j + 3) mod (nb_j + 1) (deep blocks: 0), through every MQ decode kernel form on coarse_cases' three
                 families with skip_planes 0 and 2: coarse(full decode, max(skip_planes, floor)); all-zero floors = the call without floors
(whole frames: tests/test_gpu_rate_frames.py)
"""
import functools

import numpy as np
import pytest

import coarse_cases as cc
import mallat_cases as mc
import rate_cases as rc

pytestmark = pytest.mark.gpu

FORMS = {"split": dict(t1_split=1), "one_kernel": dict(t1_split=0)}


def _ctx_with(**opts):
    from j2kgfx import Context
    ctx = Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


@functools.lru_cache(None)
def _shape_blocks():
    """per shape: (band, v, oracle bytes, oracle numBPS) of 8 blocks -- computed once, shared, never written"""
    import oracle as orc
    rng = np.random.default_rng(20270)
    out = {}
    for si, (w, h) in enumerate(cc.ONE_LAUNCH_SHAPES):
        vs = [cc.samples(rng, w, h, bits, sparse) for bits in (4, 8, 16) for sparse in (False, True)]
        vs += [np.zeros((h, w), np.int32), cc.samples(rng, w, h, 1)]
        rows = []
        for v in vs:
            data, nb = orc.t1_encode(v, w, h, 0)                    # the single block of a one-resolution plan is its LL band
            v.setflags(write=False)
            rows.append((v, np.asarray(data, np.uint8), int(nb)))
        out[(w, h)] = rows
    return out


def _check_tables(orc, v, band, data, nb, R, D, slack):
    assert int(R[0]) == 0 and int(R[nb]) == len(data)
    assert np.all(np.diff(R[:nb + 1].astype(np.int64)) >= 0)
    assert np.all(R[nb:] == len(data)) and not D[nb:].any()
    assert [int(x) for x in D[:nb + 1]] == rc.distortion(v, nb)
    for p in range(nb + 1):
        assert rc.prefix_ok(orc, data, int(R[p]), nb, band, v, p), (v.shape, nb, p, int(R[p]))
        if slack is not None and 0 < p < nb:
            m = int(R[p])
            while m > 0 and rc.prefix_ok(orc, data, m - 1, nb, band, v, p):
                m -= 1
            slack.append(int(R[p]) - m)


def _tables(t):
    return t.cpu().numpy().view(np.uint32 if t.element_size() == 4 else np.uint64)


# ---- block tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
def test_block_tables(form):
    import torch
    import oracle as orc
    from j2kgfx.codec import FramePlan
    ctx = _ctx_with(**FORMS[form])
    slack = []
    try:
        for (w, h), rows in _shape_blocks().items():
            plan = FramePlan(w, h, 1, precision=16, lossless=True, num_resolutions=1, cb=(64, 64), coder=0, ctx=ctx, closed_loop=True)
            try:
                assert int(plan.info.blocks) == 1
                b = plan.blocks()[0]
                assert (int(b["w"]), int(b["h"]), int(b["band"])) == (w, h, 0)
                for v, data, nb in rows:
                    coeff = torch.from_numpy(mc.flat_coeff(plan.planes(), [v[None]], int(plan.info.coeff_elems))).to(plan.device)
                    slots, lens, numbps, rate, dist = plan.encode_blocks(coeff, planes=True)
                    ctx.sync()
                    n = int(lens.cpu().numpy().view(np.uint32)[0])
                    assert n == len(data) and int(numbps.cpu().numpy()[0]) == nb
                    assert bytes(slots.cpu().numpy()[:n]) == bytes(data)
                    _check_tables(orc, v, 0, data, nb, _tables(rate)[0], _tables(dist)[0], slack if form == "split" else None)
            finally:
                plan.close()
    finally:
        ctx.close()
    if slack:
        print("R[p] minus the shortest valid prefix over %d (block, plane) pairs: mean %.3f, min %d, max %d" % (len(slack), np.mean(slack), min(slack), max(slack)))


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _frame(ci):
    """(coefficient tiles, per block: (v, oracle bytes, numBPS)) of FRAME_CASES[ci] -- once, shared"""
    import oracle as orc
    W, H, Cn, prec, tile, nres = cc.FRAME_CASES[ci]
    rng = np.random.default_rng(300 + ci)
    frm = rng.integers(0, 1 << prec, (Cn, H, W)).astype(np.int32)
    frm[:, :, : W // 3] = 1 << (prec - 1)                           # a flat area: blocks without planes
    return mc.forward_frame(orc, frm, tile, prec, nres)


def _frame_tables(ctx, ci, tiles=None):
    import torch
    from j2kgfx.codec import FramePlan
    W, H, Cn, prec, tile, nres = cc.FRAME_CASES[ci]
    tiles = _frame(ci) if tiles is None else tiles
    plan = FramePlan(W, H, Cn, precision=prec, lossless=True, num_resolutions=nres, cb=(64, 64), tile=tile, coder=0, ctx=ctx, mallat=True)
    coeff = torch.from_numpy(mc.flat_coeff(plan.planes(), tiles, int(plan.info.coeff_elems))).to(plan.device)
    slots, lens, numbps, rate, dist = plan.encode_blocks(coeff, planes=True)
    s2, l2, n2 = plan.encode_blocks(coeff)
    ctx.sync()
    n = int(plan.info.blocks)
    assert torch.equal(lens[:n], l2[:n]) and torch.equal(numbps[:n], n2[:n])
    return plan, tiles, slots.cpu().numpy(), s2.cpu().numpy(), lens.cpu().numpy().view(np.uint32)[:n], numbps.cpu().numpy()[:n], rate, dist


@pytest.mark.parametrize("ci", list(range(len(cc.FRAME_CASES))) + ["small_ws"])
def test_frame_tables(ci):
    """small_ws: the third geometry (13 blocks) with coefficients of 21 bits on the left and 6 on the right and a symbol workspace of 1 MiB, which
    holds 17 planes per block: the context kernel hands the deep blocks on and the one-kernel PLANES form fills their tables"""
    import oracle as orc
    tiles = None
    if ci == "small_ws":
        ci = 2
        W, H = cc.FRAME_CASES[ci][:2]
        rng = np.random.default_rng(41)
        t = rng.integers(-(1 << 6) + 1, 1 << 6, (1, H, W)).astype(np.int32)
        t[:, :, : W // 2] = rng.integers(-(1 << 21) + 1, 1 << 21, (1, H, W // 2))
        tiles = [t]
        ctx = _ctx_with(t1_lanes=8, t1_sym_mb=1)
    else:
        ctx = _ctx_with(t1_lanes=8)
    Cn = cc.FRAME_CASES[ci][2]
    try:
        plan, tiles, slots, slots2, lens, nbs, rate, dist = _frame_tables(ctx, ci, tiles)
        R, D = _tables(rate), _tables(dist)
        bl, bound = plan.blocks(), 0
        if tiles is not _frame(ci):
            assert (nbs > 17).any() and ((nbs > 0) & (nbs <= 17)).any()
        else:
            assert int(nbs.max()) >= 8 and len(set(nbs.tolist())) >= 3
        for j, b in enumerate(bl):
            w, h, band = int(b["w"]), int(b["h"]), int(b["band"])
            v = tiles[int(b["plane"]) // Cn][int(b["plane"]) % Cn][int(b["y0"]):int(b["y0"]) + h, int(b["x0"]):int(b["x0"]) + w]
            data, nb = orc.t1_encode(np.ascontiguousarray(v), w, h, band)
            n = int(lens[j])
            assert n == len(data) and int(nbs[j]) == nb
            assert bytes(slots[bound:bound + n]) == bytes(data) == bytes(slots2[bound:bound + n])
            _check_tables(orc, v, band, np.asarray(data, np.uint8), nb, R[j], D[j], None)
            bound += (rc_block_bound(w, h) + 15) & ~15
        plan.close()
    finally:
        ctx.close()


def rc_block_bound(w, h):
    from j2kgfx import entropy
    return entropy.block_bound(0, w, h)


# ---- allocation -------------------------------------------------------------------------------------------------------------------------
def _allocate_both(plan, ctx, rate, dist, numbps_t, budget):
    import torch
    kept, chosen = plan.rate_allocate(rate, dist, numbps_t, budget)
    ctx.sync()
    n = int(plan.info.blocks)
    return [int(x) for x in kept.cpu().numpy()[:n]], int(chosen.cpu().numpy()[0])


def _block_weights(plan):
    w = plan.rate_weights()
    Cn = plan.ncomp
    res = _block_res(plan)
    return [float(w[int(b["plane"]) % Cn, res[j], int(b["band"])]) for j, b in enumerate(plan.blocks())]


def _block_res(plan):
    """resolution of every job: jobs run component -> resolution -> band, and the band index restarts at LL / HL with every resolution"""
    out, r, last = [], 0, None
    for b in plan.blocks():
        key = (int(b["plane"]), int(b["band"]))
        if last is not None and key != last:
            if key[0] != last[0]:
                r = 0
            elif key[1] < last[1] or last[1] == 0:
                r += 1
        out.append(r)
        last = key
    return out


@pytest.mark.parametrize("ci", range(len(cc.FRAME_CASES)))
def test_allocation_on_frame_tables(ci):
    import torch
    ctx = _ctx_with()
    try:
        plan, tiles, slots, _s2, lens, nbs, rate, dist = _frame_tables(ctx, ci)
        n = int(plan.info.blocks)
        R, D = _tables(rate), _tables(dist)
        ws = _block_weights(plan)
        assert len(set(ws)) > 3                                      # Mallat weights: not all equal
        nb_t = torch.from_numpy(nbs.copy()).to(plan.device)
        total = int(lens.astype(np.int64).sum())
        cut_inside = dropped = False
        for budget in (0, 1, total // 10, total // 2, total, total + 1):
            want = rc.allocate(R[:n], D[:n], nbs, ws, budget)
            got = _allocate_both(plan, ctx, rate, dist, nb_t, budget)
            assert got == want, budget
            assert got[1] <= budget
            cut_inside |= any(0 < p < nb for p, nb in zip(got[0], nbs) if nb >= 2)
            dropped |= any(p == 0 for p, nb in zip(got[0], nbs) if nb > 0)
        assert cut_inside and dropped                                # otherwise the comparison is vacuous
        # other weights: another answer, still the yardstick's
        w2 = plan.rate_weights()
        w2[:, 0, :] = 1e6
        w2[:, -1, :] = 0.0
        plan.set_rate_weights(w2)
        ws2 = _block_weights(plan)
        want = rc.allocate(R[:n], D[:n], nbs, ws2, total // 4)
        assert _allocate_both(plan, ctx, rate, dist, nb_t, total // 4) == want
        plan.set_rate_weights(None)
        assert _block_weights(plan) == ws
        plan.close()
    finally:
        ctx.close()


def test_allocation_on_hand_made_tables():
    """tables no encoder writes: no more bytes for less distortion, distortion that rises, equal slopes, huge distortions (uint64 -> float64 rounds)"""
    import torch
    ctx = _ctx_with()
    try:
        W, H, Cn, prec, tile, nres = cc.FRAME_CASES[0]
        from j2kgfx.codec import FramePlan
        plan = FramePlan(W, H, Cn, precision=prec, lossless=True, num_resolutions=nres, cb=(64, 64), tile=tile, coder=0, ctx=ctx, mallat=True)
        n = int(plan.info.blocks)
        rng = np.random.default_rng(77)
        nbs = rng.integers(0, 32, n).astype(np.uint8)
        R = np.zeros((n, 32), np.uint32)
        D = np.zeros((n, 32), np.uint64)
        for j in range(n):
            nb = int(nbs[j])
            R[j, 1:nb + 1] = np.cumsum(rng.integers(0, 3 if j % 3 == 0 else 500, nb))         # j % 3 == 0: many steps of no more bytes
            R[j, nb + 1:] = R[j, nb]
            d = np.sort(rng.integers(0, 1 << (62 if j % 5 == 0 else 20), nb + 1).astype(np.uint64))[::-1]
            d[nb] = 0
            if nb >= 4 and j % 4 == 1:
                d[2] = d[0] + np.uint64(5)                                                    # rises above the start
            if nb >= 4 and j % 4 == 2:
                R[j, :4] = (0, 10, 20, 30); d[:4] = (3000, 2000, 1000, 500); R[j, 4:] = np.maximum(R[j, 4:], 30); R[j] = np.maximum.accumulate(R[j])
            D[j, :nb + 1] = d
        ws = _block_weights(plan)
        rate = torch.from_numpy(R.view(np.int32)).to(plan.device)
        dist = torch.from_numpy(D.view(np.int64)).to(plan.device)
        nb_t = torch.from_numpy(nbs).to(plan.device)
        total = int(sum(int(R[j, nbs[j]]) for j in range(n)))
        for budget in (0, 1, total // 10, total // 2, total - 1, total, total + 1):
            assert _allocate_both(plan, ctx, rate, dist, nb_t, budget) == rc.allocate(R, D, nbs, ws, budget), budget
        plan.close()
    finally:
        ctx.close()


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lossless", [True, False], ids=["53", "97"])
def test_default_weights(lossless):
    from j2kgfx.codec import FramePlan
    ctx = _ctx_with()
    try:
        plan = FramePlan(130, 70, 3, precision=8, lossless=lossless, quality=0 if lossless else 75, num_resolutions=4, cb=(64, 64), coder=0, ctx=ctx, mallat=True)
        w = plan.rate_weights()
        assert w.shape == (3, 4, 4)
        assert np.allclose(w, rc.default_weights(3, 4, lossless), rtol=1e-12, atol=0)
        plan.close()
        plan = FramePlan(130, 70, 3, precision=8, lossless=lossless, quality=0 if lossless else 75, num_resolutions=4, cb=(64, 64), coder=0, ctx=ctx, closed_loop=True)
        assert np.all(plan.rate_weights() == 1.0)
        plan.close()
    finally:
        ctx.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why,kw", [
    ("ht", dict(coder=1, mallat=True)),
    ("batch", dict(coder=0, mallat=True, frame_rows=35)),
    ("blocks_128", dict(coder=0, mallat=True, cb=(128, 128))),
    ("no_closed_loop", dict(coder=0)),
])
def test_refusals(why, kw):
    import torch
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    from j2kgfx.codec import FramePlan
    ctx = _ctx_with()
    try:
        kw = dict(kw)
        plan = FramePlan(130, 70, 3, precision=8, lossless=True, num_resolutions=4, cb=kw.pop("cb", (64, 64)), ctx=ctx, **kw)
        n = int(plan.info.blocks)
        coeff = torch.zeros(int(plan.info.coeff_elems), dtype=torch.int32, device=plan.device)
        with pytest.raises(J2KError) as e:
            plan.encode_blocks(coeff, planes=True)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        rate = torch.zeros((n, 32), dtype=torch.int32, device=plan.device)
        dist = torch.zeros((n, 32), dtype=torch.int64, device=plan.device)
        nb = torch.zeros(n, dtype=torch.uint8, device=plan.device)
        kept = torch.full((n,), 77, dtype=torch.uint8, device=plan.device)
        with pytest.raises(J2KError) as e:
            plan.rate_allocate(rate, dist, nb, 100, kept=kept)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        ctx.sync()
        assert bool((kept == 77).all())                              # refused before any launch
        plan.close()
    finally:
        ctx.close()


def test_negative_budget():
    import torch
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    from j2kgfx.codec import FramePlan
    ctx = _ctx_with()
    try:
        plan = FramePlan(130, 70, 3, precision=8, lossless=True, num_resolutions=4, cb=(64, 64), coder=0, ctx=ctx, mallat=True)
        n = int(plan.info.blocks)
        rate = torch.zeros((n, 32), dtype=torch.int32, device=plan.device)
        dist = torch.zeros((n, 32), dtype=torch.int64, device=plan.device)
        nb = torch.zeros(n, dtype=torch.uint8, device=plan.device)
        kept = torch.full((n,), 77, dtype=torch.uint8, device=plan.device)
        with pytest.raises(J2KError) as e:
            plan.rate_allocate(rate, dist, nb, -1, kept=kept)
        assert e.value.status == _lib.ERR_INVALID_ARG
        ctx.sync()
        assert bool((kept == 77).all())
        plan.close()
    finally:
        ctx.close()


# ---- decoder forms: a floor per block through every MQ decode kernel form -----------------------------------------------------------------
@functools.lru_cache(None)
def _family(name):
    """(blocks, the oracle's full decode of each, floors): computed once, shared, never written"""
    import oracle as orc
    blocks = cc.FAMILIES[name][0](orc)
    full = [cc.full_decode(orc, b) for b in blocks]
    for f in full:
        f.setflags(write=False)
    floors = np.array([(7 * j + 3) % (b["nb"] + 1) if b["nb"] <= 31 else 0 for j, b in enumerate(blocks)], np.uint8)     # deep blocks: floor 0
    floors.setflags(write=False)
    return blocks, full, floors


def _decode_floors(blocks, ctx, k, floors):
    from j2kgfx import entropy
    from j2kgfx.entropy import BLOCK_DTYPE
    bl = np.zeros(len(blocks), dtype=BLOCK_DTYPE)
    offs, pos = [], 0
    for i, b in enumerate(blocks):
        bl[i] = (0, b["band"], 0, 0, b["w"], b["h"])
        offs.append(pos)
        pos += b["data"].size
    stream = np.concatenate([b["data"] for b in blocks]) if pos else np.zeros(0, np.uint8)
    return entropy.decode_blocks(0, stream, np.array(offs, np.uint64), np.array([b["data"].size for b in blocks], np.uint32),
                                 np.array([b["nb"] for b in blocks], np.uint8), bl, ctx=ctx, skip_planes=k, floors=floors)


def _check_floors(name, ctx):
    blocks, full, floors = _family(name)
    assert len(set(floors.tolist())) > 4 and (floors == 0).any()
    for k in (0, 2):
        got = _decode_floors(blocks, ctx, k, floors)
        for i, g in enumerate(got):
            assert np.array_equal(g, cc.coarse(full[i], max(k, int(floors[i])))), (name, k, i, blocks[i]["w"], blocks[i]["h"], blocks[i]["nb"], int(floors[i]))
        zero = _decode_floors(blocks, ctx, k, np.zeros(len(blocks), np.uint8))
        plain = _decode_floors(blocks, ctx, k, None)
        for a, b in zip(zero, plain):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("general", [0, 1])
def test_floors_one_launch_kernels(general):
    ctx = _ctx_with(t1_dec_split=0, t1_dec_general=general)
    try:
        _check_floors("one_launch", ctx)
    finally:
        ctx.close()


@pytest.mark.parametrize("lanes", [2, 1, 0])
def test_floors_plane_stepped_forms(lanes):
    ctx = _ctx_with(t1_dec_split=1, t1_dec_lanes=lanes)
    try:
        _check_floors("stepped", ctx)
    finally:
        ctx.close()


@pytest.mark.parametrize("knob", [("J2K_T1_BIG_DEC_CLASSES", "0"), ("J2K_T1_BIG_DEC_CLASSES", "1"), ("J2K_T1_BIG_DEC", "0")], ids=lambda p: "%s=%s" % p)
def test_floors_big_blocks(monkeypatch, knob):
    monkeypatch.setenv(*knob)
    ctx = _ctx_with()
    try:
        _check_floors("big", ctx)
    finally:
        ctx.close()


def test_floors_refusals():
    from j2kgfx import _lib, entropy
    from j2kgfx._lib import J2KError
    from j2kgfx.entropy import BLOCK_DTYPE
    ctx = _ctx_with()
    try:
        bl = np.zeros(1, dtype=BLOCK_DTYPE)
        bl[0] = (0, 0, 0, 0, 4, 4)
        args = (np.zeros(4, np.uint8), np.zeros(1, np.uint64), np.array([4], np.uint32), np.array([3], np.uint8), bl)
        with pytest.raises(J2KError) as e:
            entropy.decode_blocks(0, *args, ctx=ctx, floors=np.array([32], np.uint8))
        assert e.value.status == _lib.ERR_INVALID_ARG
        with pytest.raises(J2KError) as e:
            entropy.decode_blocks(1, *args, ctx=ctx, floors=np.array([1], np.uint8))
        assert e.value.status == _lib.ERR_UNSUPPORTED
    finally:
        ctx.close()
