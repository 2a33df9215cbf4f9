"""GPU: rate-limited frames end to end against tests/rate_cases.py -- encode_frame_pixels(max_body_bytes=...) and decode_frame_pixels(truncated=True).

coarse_cases.FRAME_CASES as Mallat MQ plans (5-3), the first also as 9-7 with the dequantiser.  The tables R, D of a frame come from the stage
call encode_blocks(planes=True) (held to the oracle block by block in tests/test_gpu_rate_encode.py); everything after them is the yardstick's:
rate_cases.allocate picks p_j, the tile-parts must carry exactly the prefixes R_j[p_j] under headers that say (31 - nb_j, 3 p_j - 2) -- read back
with oracle/t2ref.py's PacketDecoder -- and the truncated decode must equal mallat_cases forward -> coarse(v, max(skip_planes, nb_j - p_j)) per
block -> mallat_cases inverse, bit for bit, at reduce 0 / 1 / 2 and skip_planes 0 / 3.  Budgets: "infinity" (2^62), the exact unconstrained body
bytes, 50 %, 10 %, 0."""
import functools

import numpy as np
import pytest

import closed_loop_ref as ref
import coarse_cases as cc
import mallat_cases as mc
import rate_cases as rc

pytestmark = pytest.mark.gpu
CB = 64
CASES = [(c, True, 0) for c in cc.FRAME_CASES] + [(mc.LOSSY[0][:6], False, mc.LOSSY[0][6])]
IDS = [mc.case_id(c) + ("" if ll else "-97q%d" % q) for c, ll, q in CASES]


@pytest.fixture(scope="module")
def env():
    import torch
    import oracle as orc
    from j2kgfx import Context
    ctx = Context(0)
    yield torch, orc, ctx
    ctx.close()


def _plan(ctx, case, lossless, q, **kw):
    from j2kgfx.codec import FramePlan
    W, H, Cn, prec, tile, nres = case
    kw.setdefault("mallat", True)
    return FramePlan(W, H, Cn, precision=prec, lossless=lossless, quality=q, num_resolutions=nres, cb=(CB, CB), tile=tile, coder=kw.pop("coder", 0), ctx=ctx,
                     dequantize=not lossless and kw.get("mallat", False), **kw)


@functools.lru_cache(None)
def _frame(case, lossless, q):
    """(pix, forward coefficient tiles by the oracle) -- once, shared"""
    import oracle as orc
    W, H, Cn, prec, tile, nres = case
    pix, _, _, planes = ref.pixel_frame(mc.PIX_FORMAT[(Cn, prec)], W, H, 91, orc, noise=(1 << prec) // 16)
    return pix, mc.forward_frame(orc, planes, tile, prec, nres, lossless, q)


def _block_res(plan):
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


def _windows(plan, tiles, Cn):
    """every block's coefficients (views into the oracle's tiles) and the slice that addresses them"""
    out = []
    for b in plan.blocks():
        t, c = int(b["plane"]) // Cn, int(b["plane"]) % Cn
        out.append((t, c, slice(int(b["y0"]), int(b["y0"]) + int(b["h"])), slice(int(b["x0"]), int(b["x0"]) + int(b["w"]))))
    return out


def _tables(torch, plan, case, pix):
    """R, D, numbps, lens of the frame (device stage calls) and the weight of every block"""
    Cn, prec = case[2], case[3]
    coeff = plan.forward_pixels(mc.PIX_FORMAT[(Cn, prec)], torch.from_numpy(pix).to(plan.device))
    slots, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True)
    plan.ctx.sync()
    n = int(plan.info.blocks)
    w = plan.rate_weights()
    res = _block_res(plan)
    ws = [float(w[int(b["plane"]) % Cn, res[j], int(b["band"])]) for j, b in enumerate(plan.blocks())]
    return (rate.cpu().numpy().view(np.uint32)[:n], dist.cpu().numpy().view(np.uint64)[:n], nbs.cpu().numpy()[:n].astype(np.int64),
            lens.cpu().numpy().view(np.uint32)[:n].astype(np.int64), slots.cpu().numpy(), ws)


def _expected_pixels(orc, case, lossless, q, tiles, wins, floors, reduce):
    W, H, Cn, prec, tile, nres = case
    cut = [t.copy() for t in tiles]
    for (t, c, ys, xs), k in zip(wins, floors):
        cut[t][c, ys, xs] = cc.coarse(tiles[t][c, ys, xs], int(k))
    kw = {} if lossless else dict(lossless=False, quality=q, dequantize=True)
    return mc.pixels(orc, mc.inverse_frame(orc, cut, W, H, tile, prec, nres, reduce=reduce, **kw), prec)


def _read_headers(t2ref, plan, h_cs, h_toffs, marks):
    """(zero_bit_planes, num_passes, body length, included) of every block, read with the oracle's PacketDecoder tile by tile"""
    bl, res = plan.blocks(), _block_res(plan)
    Cn = plan.ncomp
    out, j = [], 0
    for t in range(int(plan.info.tiles)):
        part = bytes(h_cs[int(h_toffs[t]):int(h_toffs[t + 1])])
        dec = t2ref.PacketDecoder(part[14:], len_bits=5, seated=True)
        while j < len(bl) and int(bl[j]["plane"]) // Cn == t:
            k = j
            while k < len(bl) and int(bl[k]["plane"]) == int(bl[j]["plane"]) and res[k] == res[j]:
                k += 1
            blocks = [t2ref.CodeBlock(None, 0, 0, 0) for _ in range(k - j)]
            dec.decode_packet(t2ref.Precinct([blocks]), 0, marks, marks)
            out += [(b.zero_bit_planes, b.num_passes, b.dlen(), b.included_in_layers == 0 and b.dlen() > 0) for b in blocks]
            j = k
    assert j == len(bl)
    return out


@pytest.mark.parametrize("marks", [False, True], ids=["bare", "sop_eph"])
@pytest.mark.parametrize("case,lossless,q", CASES, ids=IDS)
def test_rate_limited_frames(env, case, lossless, q, marks):
    import t2ref
    torch, orc, ctx = env
    W, H, Cn, prec, tile, nres = case
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    pix, tiles = _frame(case, lossless, q)
    plan = _plan(ctx, case, lossless, q)
    try:
        R, D, nbs, lens, slots, ws = _tables(torch, plan, case, pix)
        n = len(nbs)
        wins = _windows(plan, tiles, Cn)
        total = int(lens.sum())
        d_pix = torch.from_numpy(pix).to(plan.device)
        plain, ptoffs = plan.encode_frame_pixels(fmt, d_pix, sop=marks, eph=marks)
        plan.frame_status()
        plain_bytes = bytes(plain.cpu().numpy()[:int(ptoffs[-1].item())])
        for name, budget in (("inf", 1 << 62), ("exact", total), ("50", total // 2), ("10", total // 10), ("0", 0)):
            cs, toffs = plan.encode_frame_pixels(fmt, d_pix, sop=marks, eph=marks, max_body_bytes=budget)
            plan.frame_status()
            length = int(toffs[-1].item())
            h_cs, h_toffs = cs.cpu().numpy(), toffs.cpu().numpy()
            ps, chosen = rc.allocate(R, D, nbs, ws, budget)
            if name in ("inf", "exact"):
                assert bytes(h_cs[:length]) == plain_bytes, name
                assert ps == [int(x) for x in nbs]
            # the block tables the device reads back: bodies within the budget, the prefixes R[p], floors nb - p
            offs2, lens2, nb2, fl2 = plan.decode_tile_parts(cs, length, tile_offs=toffs, sop=marks, eph=marks, floors=True)
            plan.frame_status()
            o2, l2, n2, f2 = offs2.cpu().numpy(), lens2.cpu().numpy().view(np.uint32), nb2.cpu().numpy(), fl2.cpu().numpy()
            body = int(l2[:n].astype(np.int64).sum())
            assert body <= budget and body == chosen, (name, body, chosen, budget)
            heads = _read_headers(t2ref, plan, h_cs, h_toffs, marks)
            floors = []
            for j in range(n):
                p, nb = ps[j], int(nbs[j])
                want_len = int(R[j, p]) if p > 0 else 0
                assert int(l2[j]) == want_len, (name, j)
                zbp, npass, dlen, incl = heads[j]
                assert dlen == want_len and incl == (want_len > 0), (name, j)
                if want_len:
                    assert (zbp, npass) == (31 - nb, rc.passes_of(p)), (name, j)
                    assert rc.floors_from_header(zbp, npass) == (nb - p, nb)
                    assert (int(f2[j]), int(n2[j])) == (nb - p, nb), (name, j)
                    lo = plan_slot_offset(plan, j)
                    assert bytes(h_cs[int(o2[j]):int(o2[j]) + want_len]) == bytes(slots[lo:lo + want_len]), (name, j)
                else:
                    assert (int(f2[j]), int(n2[j])) == (0, 0), (name, j)
                floors.append(nb - p)
            if name == "50":
                assert any(0 < ps[j] < nbs[j] for j in range(n) if nbs[j] >= 2), "vacuous: no block cut inside"
            if name == "10":
                assert any(ps[j] == 0 and nbs[j] > 0 for j in range(n)), "vacuous: no block dropped"
            if name == "0":
                assert body == 0 and not any(ps)
            for r in (0, 1, 2):
                assert r in mc.admissible(W, H, tile, nres)
                for k in (0, 3):
                    exp = _expected_pixels(orc, case, lossless, q, tiles, wins, [max(k, f) for f in floors], r)
                    back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
                    plan.decode_frame_pixels(cs, length, back, tile_offs=toffs if k else None, sop=marks, eph=marks, reduce=r, skip_planes=k, truncated=True)
                    plan.frame_status()
                    assert np.array_equal(back.cpu().numpy(), exp), (name, r, k)
                    if name == "0" and r == 0 and k == 0:           # the frame of all-zero coefficients
                        zero = _expected_pixels(orc, case, lossless, q, [np.zeros_like(t) for t in tiles], wins, [0] * n, 0)
                        assert np.array_equal(exp, zero)
    finally:
        plan.close()


_SLOT_CACHE = {}


def plan_slot_offset(plan, j):
    """byte offset of job j's coding slot (the slots are the blocks' bounds rounded up to 16, in job order)"""
    import weakref
    from j2kgfx import entropy
    # (the entry is its plan's while that very object lives: a later plan may get a closed one's id(), and with it another geometry's offsets)
    ref, offs = _SLOT_CACHE.get("plan", (None, None))
    if ref is None or ref() is not plan:
        offs, pos = [], 0
        for b in plan.blocks():
            offs.append(pos)
            pos += (entropy.block_bound(0, int(b["w"]), int(b["h"])) + 15) & ~15
        _SLOT_CACHE["plan"] = (weakref.ref(plan), offs)
    return offs[j]


def test_cut_stream_without_truncated_keeps_the_old_rule(env):
    """a rate-limited stream through decode_frame_pixels WITHOUT truncated=True: every block decodes by the old rule, numbps = (passes + 2) / 3 --
    the oracle's decode of the kept prefix with p planes, placed and inverted"""
    torch, orc, ctx = env
    case = cc.FRAME_CASES[0]
    W, H, Cn, prec, tile, nres = case
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    pix, tiles = _frame(case, True, 0)
    plan = _plan(ctx, case, True, 0)
    try:
        R, D, nbs, lens, slots, ws = _tables(torch, plan, case, pix)
        wins = _windows(plan, tiles, Cn)
        budget = int(lens.sum()) // 2
        ps, _ = rc.allocate(R, D, nbs, ws, budget)
        assert any(0 < p < nb for p, nb in zip(ps, nbs))
        cs, toffs = plan.encode_frame_pixels(fmt, torch.from_numpy(pix).to(plan.device), sop=True, eph=True, max_body_bytes=budget)
        plan.frame_status()
        old = [np.zeros_like(t) for t in tiles]
        for j, ((t, c, ys, xs), b) in enumerate(zip(wins, plan.blocks())):
            if ps[j] > 0:
                lo = plan_slot_offset(plan, j)
                old[t][c, ys, xs] = orc.t1_decode(slots[lo:lo + int(R[j, ps[j]])], ps[j], int(b["band"]), int(b["w"]), int(b["h"]))
        exp = mc.pixels(orc, mc.inverse_frame(orc, old, W, H, tile, prec, nres), prec)
        back = torch.zeros(exp.shape, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, int(toffs[-1].item()), back, sop=True, eph=True)
        plan.frame_status()
        assert np.array_equal(back.cpu().numpy(), exp)
    finally:
        plan.close()


def test_stage_calls_kept_and_floors(env):
    """the stage chain: encode_stream -> rate_allocate -> encode_tile_parts(kept, rate) gives the frame call's bytes; kept = numBPS gives
    encode_tile_parts' bytes; decode_tile_parts(floors) + decode_blocks(floors) + place_blocks give the coarsened coefficients"""
    torch, orc, ctx = env
    case = cc.FRAME_CASES[1]
    W, H, Cn, prec, tile, nres = case
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    pix, tiles = _frame(case, True, 0)
    plan = _plan(ctx, case, True, 0)
    try:
        d_pix = torch.from_numpy(pix).to(plan.device)
        coeff = plan.forward_pixels(fmt, d_pix)
        slots, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True)
        offs, stream = plan.compact(slots, lens)
        n = int(plan.info.blocks)
        total = int(lens[:n].to(torch.int64).sum().item())
        kept, chosen = plan.rate_allocate(rate, dist, nbs, total // 3)
        cs, toffs = plan.encode_tile_parts(stream, offs, lens, nbs, sop=True, eph=False, kept=kept, rate=rate)
        plan.frame_status()
        cs2, toffs2 = plan.encode_frame_pixels(fmt, d_pix, sop=True, eph=False, max_body_bytes=total // 3)
        plan.frame_status()
        length = int(toffs[-1].item())
        assert length == int(toffs2[-1].item()) and torch.equal(cs[:length], cs2[:length])
        full, ftoffs = plan.encode_tile_parts(stream, offs, lens, nbs, sop=True, eph=False, kept=nbs, rate=rate)
        ref_cs, rtoffs = plan.encode_tile_parts(stream, offs, lens, nbs, sop=True, eph=False)
        plan.frame_status()
        flen = int(rtoffs[-1].item())
        assert int(ftoffs[-1].item()) == flen and torch.equal(full[:flen], ref_cs[:flen])
        o2, l2, n2, f2 = plan.decode_tile_parts(cs, length, sop=True, eph=False, floors=True)
        placed = plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2, floors=f2))
        plan.frame_status()
        hp, rows = placed.cpu().numpy(), plan.planes()
        ks = (nbs[:n].to(torch.int64) - kept[:n].to(torch.int64)).cpu().numpy()
        wins = _windows(plan, tiles, Cn)
        cut = [t.copy() for t in tiles]
        for (t, c, ys, xs), k in zip(wins, ks):
            cut[t][c, ys, xs] = cc.coarse(tiles[t][c, ys, xs], int(k))
        for t_, c_, _x0, _y0, w_, h_, off in (tuple(int(v) for v in r) for r in rows):
            assert np.array_equal(hp[off:off + w_ * h_].reshape(h_, w_), cut[t_][c_]), (t_, c_)
    finally:
        plan.close()


def test_host_one_call_pair(env):
    torch, orc, ctx = env
    case = cc.FRAME_CASES[0]
    W, H, Cn, prec, tile, nres = case
    fmt = mc.PIX_FORMAT[(Cn, prec)]
    pix, tiles = _frame(case, True, 0)
    plan = _plan(ctx, case, True, 0)
    try:
        R, D, nbs, lens, slots, ws = _tables(torch, plan, case, pix)
        budget = int(lens.sum()) // 2
        ps, chosen = rc.allocate(R, D, nbs, ws, budget)
        got = plan.encode_pixels_host(fmt, pix, sop=True, eph=True, max_body_bytes=budget)
        cs, toffs = plan.encode_frame_pixels(fmt, torch.from_numpy(pix).to(plan.device), sop=True, eph=True, max_body_bytes=budget)
        plan.frame_status()
        assert bytes(got["bytes"]) == bytes(cs.cpu().numpy()[:int(toffs[-1].item())])
        assert np.array_equal(got["lens"].astype(np.int64), lens) and np.array_equal(got["numbps"].astype(np.int64), nbs)
        wins = _windows(plan, tiles, Cn)
        for r, k in ((0, 0), (1, 3)):
            exp = _expected_pixels(orc, case, True, 0, tiles, wins, [max(k, int(nb) - p) for nb, p in zip(nbs, ps)], r)
            host = plan.decode_pixels_host(got["bytes"], exp.shape, sop=True, eph=True, reduce=r, skip_planes=k, truncated=True)
            assert np.array_equal(host, exp), (r, k)
    finally:
        plan.close()


@pytest.mark.parametrize("why,kw", [
    ("ht", dict(coder=1)),
    ("batch", dict(frame_rows=35)),
    ("blocks_128", dict(cb=128)),
    ("no_closed_loop", dict(mallat=False)),
])
def test_frame_refusals(env, why, kw):
    torch, orc, ctx = env
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    from j2kgfx.codec import FramePlan
    kw = dict(kw)
    cb = kw.pop("cb", 64)
    plan = FramePlan(130, 70, 3, precision=8, lossless=True, num_resolutions=4, cb=(cb, cb), coder=kw.pop("coder", 0), ctx=ctx, mallat=kw.pop("mallat", True), **kw)
    try:
        pix = torch.zeros((70, 130 * 4), dtype=torch.uint8, device=plan.device)
        out = torch.full((1 << 16,), 0x77, dtype=torch.uint8, device=plan.device)
        for budget, status in ((1000, _lib.ERR_UNSUPPORTED),):
            with pytest.raises(J2KError) as e:
                plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, max_body_bytes=budget)
            assert e.value.status == status
        ctx.sync()
        assert bool((out == 0x77).all())                            # refused before any launch
    finally:
        plan.close()


def test_negative_budget(env):
    torch, orc, ctx = env
    from j2kgfx import _lib
    from j2kgfx._lib import J2KError
    plan = _plan(ctx, cc.FRAME_CASES[0], True, 0)
    try:
        pix = torch.zeros((70, 130 * 4), dtype=torch.uint8, device=plan.device)
        out = torch.full((1 << 16,), 0x77, dtype=torch.uint8, device=plan.device)
        with pytest.raises(J2KError) as e:
            plan.encode_frame_pixels(_lib.PIX_RGBA8, pix, out=out, max_body_bytes=-1)
        assert e.value.status == _lib.ERR_INVALID_ARG
        ctx.sync()
        assert bool((out == 0x77).all())
    finally:
        plan.close()
