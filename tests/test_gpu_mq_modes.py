"""GPU: the MQ block coder's own choice between its latency and its throughput setting (tests/mq_mode_cases.py), with nothing forced -- no
t1_dec_split / t1_lanes option, no J2K_T1_* variable: what FramePlan.mq_forms() reports is the restated rule, and whatever form runs, the bytes
and the decoded blocks are the oracle's.

(a) the life of a plan across the flip, and (e) graph capture across it, in child processes (tests/helpers_mq_modes.py: "alone" needs a process
    whose count of MQ contexts starts at 0);
(b) in company, in this process (the module makes its own company and holds it): every feature of the MQ codec once on the mid plan;
(c) two contexts with frames in flight, no synchronisation between them;
(d) the decoder's fall-back for a stream that is not 16-byte aligned is reported, and decodes the same."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mq_mode_cases as mc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_child_failed = []


# ---- (a), (e): child processes ----------------------------------------------------------------------------------------------------------------
STATES = ["alone", "company", "company_left", "two_in_company", "one_closed_under_its_plan", "alone_again", "ht_company"]
CAPTURE_STATES = ["alone_warm_up", "alone_graph_alone", "alone_graph_in_company", "capture_refused", "works_after_refusal", "company_graph"]


@pytest.mark.parametrize("family", ["mid", "big", "bigmid", "capture"])
def test_life_of_a_plan_across_the_flip(family):
    """alone -> company -> alone -> company of two, one closed under its plan -> alone -> HT company, the same plans and buffers throughout:
    encoder bytes, lengths, numBPS, decoder output on the encoder's stream and on arbitrary bytes against the oracle, mq_forms() against the rule
    and the number of live counted contexts in every state (family "capture": a graph captured alone replays after the flip; a capture right
    after the flip is refused, the context works afterwards and the capture then succeeds)"""
    assert not _child_failed, "not started: the child process of %s did not end in order" % _child_failed
    env = {k: v for k, v in os.environ.items() if not k.startswith("J2K_") or k == "J2K_LIB"}     # nothing forced: no tuning variable reaches the child
    try:
        out = subprocess.run([sys.executable, os.path.join(HERE, "helpers_mq_modes.py"), family], capture_output=True, text=True, env=env, timeout=300)
    except subprocess.TimeoutExpired:
        _child_failed.append(family)
        raise
    if out.returncode not in (0, 1):
        _child_failed.append(family)
    assert out.returncode in (0, 1), (out.returncode, out.stderr[-3000:])
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    assert res["family"] == family and res["failures"] == [], res["failures"]
    assert res["states"] == (CAPTURE_STATES if family == "capture" else STATES)
    assert out.returncode == 0
    if family != "capture":
        assert res["checks"] == len(STATES) * len(mc.FAMILIES[family]) * 9


# ---- in this process: company that the module holds -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    """(torch, oracle, t2ref, Context) with two more contexts alive that have each built an MQ plan: every context of a test is in company,
    whatever else the session holds"""
    import torch
    import oracle as orc
    import t2ref
    from j2kgfx.context import Context
    from j2kgfx.codec import FramePlan
    held = []
    for _ in range(2):
        ctx = Context(0)
        held.append((ctx, FramePlan(ctx=ctx, **mc.plan_kwargs(mc.PLANS["small"]))))
    yield torch, orc, t2ref, Context
    for ctx, plan in held:
        plan.close()
        ctx.close()


def _forms_in_company(got, n, max_dim, **kw):
    """mq_forms() against the rule, the count aside (other modules' contexts may be alive too): at least the module's two and the test's own"""
    got = [int(v) for v in got]
    assert got[0] >= 3, got
    assert got[1:] == mc.forms(n, max_dim, got[0], **kw)[1:], (got, mc.forms(n, max_dim, got[0], **kw))


class _Stage:
    """a plan of mq_mode_cases on a context of its own, its coefficient buffer on the device, the oracle's decodes of its blocks"""

    def __init__(self, env, name, seed=0, **plan_more):
        torch, orc, _, Context = env
        from j2kgfx.codec import FramePlan
        self.c = c = mc.case(name, seed)
        self.ctx = Context(0)
        self.plan = plan = FramePlan(ctx=self.ctx, **mc.plan_kwargs(c["plan"], **plan_more))
        self.n = int(plan.info.blocks)
        assert self.n == c["n"]
        self.coeff = torch.from_numpy(mc.coeff_buffer(c, plan.planes(), plan.info.coeff_elems)).to(plan.device)
        self.doffs = plan.decoded_offsets().astype(np.int64)
        self.sizes = np.array([int(b["w"]) * int(b["h"]) for _, b in c["jobs"]], np.int64)

    def blocks_of(self, decoded):
        hd = decoded.cpu().numpy()
        return [hd[self.doffs[j]:self.doffs[j] + self.sizes[j]].reshape(int(b["h"]), int(b["w"])) for j, (_, b) in enumerate(self.c["jobs"])]

    def close(self):
        self.plan.close()
        self.ctx.close()


def _plain_decodes(orc, c):
    """oracle.t1_decode of the oracle's encode of every job, with the encoder's own bit-plane counts"""
    offs = np.concatenate(([0], np.cumsum(c["lens"].astype(np.int64))))
    return [orc.t1_decode(c["bytes"][offs[j]:offs[j + 1]], int(c["numbps"][j]), int(b["band"]), int(b["w"]), int(b["h"])) for j, (_, b) in enumerate(c["jobs"])]


def _check_encode(s, stream, offs, lens, numbps):
    c, n = s.c, s.n
    ho = offs.cpu().numpy()
    assert np.array_equal(lens.cpu().numpy()[:n].astype(np.uint32), c["lens"])
    assert np.array_equal(numbps.cpu().numpy()[:n], c["numbps"])
    assert np.array_equal(ho[:n + 1], np.concatenate(([0], np.cumsum(c["lens"].astype(np.int64)))))
    assert np.array_equal(stream.cpu().numpy()[:int(ho[n])], c["bytes"])


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------
def test_company_skip_planes(env):
    """decode_blocks(skip_planes=k) of the mid plan in company: the plane-stepped path, K > 1 in the encode, coarse(oracle.t1_decode, k)"""
    import coarse_cases as cc
    torch, orc, _, _ = env
    s = _Stage(env, "mid")
    try:
        stream, offs, lens, numbps = s.plan.encode_stream(s.coeff)
        s.ctx.sync()
        _check_encode(s, stream, offs, lens, numbps)
        full = _plain_decodes(orc, s.c)
        for k in (0, 1, 3, 14):
            dec = s.plan.decode_blocks(stream, offs, lens, numbps, skip_planes=k)
            s.ctx.sync()
            forms = s.plan.mq_forms()
            _forms_in_company(forms, s.n, s.c["max_dim"])
            assert forms[1] > 1 and forms[3] == 1
            for j, got in enumerate(s.blocks_of(dec)):
                assert np.array_equal(got, cc.coarse(full[j], k)), (k, j)
    finally:
        s.close()


def test_company_host_call_takes_the_same_split_as_the_plan_call(env):
    """entropy.decode_blocks (j2k_decode_blocks: no plan) on the blocks of a mid plan just above the threshold (576), of the big + mid plan and of a
    big plan, in company: it reports the split the plan call reports on the same blocks, its big-block decoder stays one launch, and both equal
    oracle.t1_decode -- on the encoder's stream with deep blocks and on arbitrary bytes.  The host call takes any list of blocks, so the threshold
    itself is pinned there: the first 511 blocks decode on the one-launch kernels, the first 512 plane-stepped."""
    from j2kgfx import entropy
    torch, orc, _, _ = env
    for name in ("mid_576", "bigmid", "big128"):
        s = _Stage(env, name)
        try:
            c = s.c
            blocks = np.zeros(s.n, entropy.BLOCK_DTYPE)
            for j, (_, b) in enumerate(c["jobs"]):
                blocks[j] = (0, int(b["band"]), 0, 0, int(b["w"]), int(b["h"]))
            for label, by, offs, lens, nbv, want in mc.decode_streams(orc, c):
                got = entropy.decode_blocks(0, by, offs[:s.n], lens, nbv, blocks, ctx=s.ctx)
                host = s.ctx.mq_forms()
                _forms_in_company(host, s.n, c["max_dim"], host_call=True)
                pad = np.zeros(by.size + 64, np.uint8)
                pad[:by.size] = by
                dec = s.plan.decode_blocks(torch.from_numpy(pad).to(s.plan.device), torch.from_numpy(offs.astype(np.int64)).to(s.plan.device),
                                           torch.from_numpy(lens.astype(np.int32)).to(s.plan.device), torch.from_numpy(nbv).to(s.plan.device))
                s.ctx.sync()
                plan = s.plan.mq_forms()
                _forms_in_company(plan, s.n, c["max_dim"], encoded=False)
                assert (host[3], host[4], host[6]) == (plan[3], plan[4], plan[6]) and host[3] == (1 if s.n >= 512 else 0), (name, label, host, plan)
                via_plan = s.blocks_of(dec)
                for j in range(s.n):
                    assert np.array_equal(got[j], want[j]), (name, label, j)
                    assert np.array_equal(via_plan[j], want[j]), (name, label, j)
                if name == "mid_576":
                    for m in (mc.SPLIT_MIN_COMPANY - 1, mc.SPLIT_MIN_COMPANY):
                        got = entropy.decode_blocks(0, by, offs[:m], lens[:m], nbv[:m], blocks[:m], ctx=s.ctx)
                        _forms_in_company(s.ctx.mq_forms(), m, c["max_dim"], host_call=True)
                        assert s.ctx.mq_forms()[3] == (1 if m == mc.SPLIT_MIN_COMPANY else 0)
                        for j in range(m):
                            assert np.array_equal(got[j], want[j]), (name, label, m, j)
        finally:
            s.close()


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------------
def test_two_contexts_with_frames_in_flight(env):
    """Two contexts queue encode_stream + decode_blocks of different contents, three rounds into the same buffers, no synchronisation between the
    contexts or the rounds; a copy queued on each context's own stream keeps every round's outputs.  Every round of either context: the oracle's
    bytes, lengths, numBPS and decoded blocks."""
    torch, orc, _, _ = env
    rounds = 3
    sides = []
    for name in ("mid", "mid_tiled"):
        first = _Stage(env, name, 0)
        cases = [first.c] + [mc.case(name, r) for r in range(1, rounds)]
        coeffs = [first.coeff] + [torch.from_numpy(mc.coeff_buffer(c, first.plan.planes(), first.plan.info.coeff_elems)).to(first.plan.device) for c in cases[1:]]
        plan, n = first.plan, first.n
        bufs = dict(stream=torch.zeros(int(plan.info.bytes_cap) + 64, dtype=torch.uint8, device=plan.device), offs=torch.zeros(n + 1, dtype=torch.int64, device=plan.device),
                    lens=torch.zeros(n, dtype=torch.int32, device=plan.device), numbps=torch.zeros(n, dtype=torch.uint8, device=plan.device),
                    decoded=torch.zeros(max(int(plan.info.decoded_elems), 4), dtype=torch.int32, device=plan.device))
        room = max(int(c["bytes"].size) for c in cases) + 64
        keeps = [dict((k, torch.zeros_like(v[:room] if k == "stream" else v)) for k, v in bufs.items()) for _ in range(rounds)]
        sides.append(dict(stage=first, cases=cases, coeffs=coeffs, bufs=bufs, keeps=keeps))
    torch.cuda.synchronize()
    try:
        for r in range(rounds):
            for side in sides:
                plan, b = side["stage"].plan, side["bufs"]
                plan.encode_stream(side["coeffs"][r], b["stream"], b["offs"], b["lens"], b["numbps"])
                plan.decode_blocks(b["stream"], b["offs"], b["lens"], b["numbps"], b["decoded"])
                with torch.cuda.stream(plan._ext()):                  # on the context's own stream, behind the two calls: no synchronisation
                    for k, v in b.items():
                        side["keeps"][r][k].copy_(v[:side["keeps"][r][k].numel()])
        for side in sides:
            side["stage"].ctx.sync()
        for side in sides:
            s = side["stage"]
            forms = s.plan.mq_forms()
            _forms_in_company(forms, s.n, s.c["max_dim"])
            assert forms[1] > 1 and forms[3] == 1
            for r in range(rounds):
                s.c = side["cases"][r]
                k = side["keeps"][r]
                _check_encode(s, k["stream"], k["offs"], k["lens"], k["numbps"])
                want = _plain_decodes(orc, s.c)
                for j, got in enumerate(s.blocks_of(k["decoded"])):
                    assert np.array_equal(got, want[j]), (s.c["name"], r, j)
    finally:
        for side in sides:
            side["stage"].close()


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------------------
def test_unaligned_stream_falls_back_and_says_so(env):
    """a stream handed over at a 4-byte offset, in company, on the mid plan: the plane-stepped path is wanted and not taken (its 16-byte loads),
    mq_forms() says so, and the one-launch kernels decode what the oracle decodes"""
    torch, orc, _, _ = env
    s = _Stage(env, "mid")
    try:
        c = s.c
        for label, by, offs, lens, nbv, want in mc.decode_streams(orc, c):
            pad = np.zeros(by.size + 64, np.uint8)
            pad[4:4 + by.size] = by
            d = torch.from_numpy(pad).to(s.plan.device)
            assert d.data_ptr() % 16 == 0
            args = (torch.from_numpy(offs.astype(np.int64)).to(s.plan.device), torch.from_numpy(lens.astype(np.int32)).to(s.plan.device), torch.from_numpy(nbv).to(s.plan.device))
            dec = s.plan.decode_blocks(d[4:], *args)
            s.ctx.sync()
            forms = s.plan.mq_forms()
            _forms_in_company(forms, s.n, c["max_dim"], aligned=False, encoded=False)
            assert forms[6] == 1 and forms[3] == 0
            for j, got in enumerate(s.blocks_of(dec)):
                assert np.array_equal(got, want[j]), (label, j)
            d2 = torch.from_numpy(np.concatenate([by, np.zeros(64, np.uint8)])).to(s.plan.device)      # the same bytes aligned: the path is taken
            dec = s.plan.decode_blocks(d2, *args)
            s.ctx.sync()
            forms = s.plan.mq_forms()
            _forms_in_company(forms, s.n, c["max_dim"], encoded=False)
            assert forms[6] == 0 and forms[3] == 1
            for j, got in enumerate(s.blocks_of(dec)):
                assert np.array_equal(got, want[j]), (label, j)
    finally:
        s.close()


def test_company_raw_magref(env):
    """the raw-MagRef style on a plan of 600 blocks in company: the RAWMR instantiation of the lanes encoder with K > 1 and the style's plane-stepped
    decoder (16 KB more workspace per block) -- bodies, lengths, numBPS by raw_magref_cases.encode_tile_blocks, the decode by its decode_block on
    every fifth block and, for every block, the coefficients that went in (the style is lossless)"""
    import raw_magref_cases as rm
    torch, orc, _, _ = env
    s = _Stage(env, "mid_cb8", raw_magref=True)
    try:
        c, p = s.c, s.c["plan"]
        assert s.plan.raw_magref
        by, ln, nb = _raw_reference(orc)
        stream, offs, lens, numbps = s.plan.encode_stream(s.coeff)
        dec = s.plan.decode_blocks(stream, offs, lens, numbps)
        s.ctx.sync()
        forms = s.plan.mq_forms()
        _forms_in_company(forms, s.n, c["max_dim"])
        assert forms[1] > 1 and forms[3] == 1
        ho = offs.cpu().numpy()
        assert np.array_equal(lens.cpu().numpy()[:s.n].astype(np.uint32), ln) and np.array_equal(numbps.cpu().numpy()[:s.n], nb)
        assert np.array_equal(nb, c["numbps"])                      # (the style leaves the bit-plane counts alone)
        assert np.array_equal(stream.cpu().numpy()[:int(ho[s.n])], by)
        pos = np.concatenate(([0], np.cumsum(ln.astype(np.int64))))
        for j, got in enumerate(s.blocks_of(dec)):
            t, b = c["jobs"][j]
            _, _, x0, y0, _, _ = c["tiles"][t]
            win = c["coeff"][int(b["comp"]), y0 + int(b["y0"]):y0 + int(b["y0"]) + int(b["h"]), x0 + int(b["x0"]):x0 + int(b["x0"]) + int(b["w"])]
            assert np.array_equal(got, win), j
            if j % 5 == 1:
                assert np.array_equal(got, rm.decode_block(by[pos[j]:pos[j + 1]], int(nb[j]), int(b["band"]), int(b["w"]), int(b["h"]), orc)), j
    finally:
        s.close()


_RAW = {}


def _raw_reference(orc):
    import raw_magref_cases as rm
    if "mid_cb8" not in _RAW:
        c = mc.case("mid_cb8")
        p = c["plan"]
        _RAW["mid_cb8"] = rm.encode_tile_blocks(orc, [c["coeff"][k] for k in range(p["C"])], p["W"], p["H"], p["nres"], p["cb"], p["cb"], 1)
    return _RAW["mid_cb8"]


# the mid plan's geometry as pixels: 16-bit RGB (image.RGBA64), 272 x 200, three resolutions, 16 x 16 blocks -- 807 blocks
PIX_W, PIX_H, PIX_NRES, PIX_CB = mc.PLANS["mid"]["W"], mc.PLANS["mid"]["H"], mc.PLANS["mid"]["nres"], mc.PLANS["mid"]["cb"]
_PIX = {}


def _pixel_frames(orc, t2ref):
    """two frames of the geometry (noise with a flat left part: blocks without a plane) and the oracle's closed-loop tile-parts of each alone and of the
    batch of both -- made once, shared, never written"""
    import closed_loop_ref as ref
    from j2kgfx import _lib
    if not _PIX:
        frames = []
        for seed in (5, 6):
            pix, Cn, prec, planes = ref.pixel_frame(_lib.PIX_RGBA64, PIX_W, PIX_H, seed, orc, noise=1 << 11)
            row = pix.shape[1]
            flat = ref.pixel_frame(_lib.PIX_RGBA64, PIX_W, PIX_H, seed, orc, flat=True)[0]
            pix[:, : (row // 8 // 3) * 8] = flat[:, : (row // 8 // 3) * 8]                      # the left third: mid-grey
            planes = np.stack(orc.extract_image_data(pix, _lib.PIX_RGBA64, PIX_W, PIX_H))[:Cn]
            frames.append((pix, planes.astype(np.int32)))
        assert (Cn, prec) == (3, 16)
        _PIX["frames"] = frames
        _PIX["alone"] = [ref.oracle_frame(pl, PIX_W, PIX_H, PIX_W, PIX_H, PIX_NRES, PIX_CB, 0, True, False, orc, t2ref, precision=16) for _, pl in frames]
        _PIX["batch"] = ref.oracle_batch([pl for _, pl in frames], PIX_W, PIX_H, PIX_W, PIX_H, PIX_NRES, PIX_CB, 0, True, False, orc, t2ref, precision=16)
        _PIX["back"] = [orc.create_image([pl[k] for k in range(3)], 16) for _, pl in frames]    # what a lossless decode writes
        n = len(_PIX["alone"][0][0]["lens"])
        assert n == mc.case("mid")["n"] and (_PIX["alone"][0][0]["lens"] == 0).sum() > n // 8
    return _PIX


def _pixel_plan(env, frames=1):
    from j2kgfx.codec import FramePlan
    ctx = env[3](0)
    kw = dict(frame_rows=PIX_H) if frames > 1 else {}
    return ctx, FramePlan(PIX_W, PIX_H * frames, 3, precision=16, lossless=True, num_resolutions=PIX_NRES, cb=(PIX_CB, PIX_CB), tile=(0, 0), coder=0, ctx=ctx,
                          closed_loop=True, **kw)


def test_company_frame_calls_and_host_forms(env):
    """encode_frame_pixels / decode_frame_pixels and encode_pixels_host / decode_pixels_host of the mid geometry in company: the oracle's tile-parts
    (closed_loop_ref.oracle_frame) byte for byte, the pixels createImage makes of the samples that went in, K > 1 and the plane-stepped decoder"""
    from j2kgfx import _lib
    torch, orc, t2ref, _ = env
    P = _pixel_frames(orc, t2ref)
    ctx, plan = _pixel_plan(env)
    n = int(plan.info.blocks)
    try:
        for k, (pix, planes) in enumerate(P["frames"]):
            want = b"".join(P["alone"][k][t]["part"] for t in sorted(P["alone"][k]))
            d_pix = torch.from_numpy(pix).to(plan.device)
            cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA64, d_pix, sop=True, eph=False)
            plan.frame_status()
            forms = plan.mq_forms()
            assert forms[1] == mc.enc_k(n, True) > 1 and forms[2] == 0, forms
            total = int(toffs[-1].item())
            assert bytes(cs.cpu().numpy()[:total]) == want, k
            back = torch.full(pix.shape, 0x5A, dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, total, back, tile_offs=toffs if k else None, sop=True, eph=False)
            plan.frame_status()
            _forms_in_company(plan.mq_forms(), n, PIX_CB)
            assert plan.mq_forms()[3] == 1
            assert np.array_equal(back.cpu().numpy(), P["back"][k]), k
            # the host forms
            res = plan.encode_pixels_host(_lib.PIX_RGBA64, pix, sop=True, eph=False)
            assert bytes(res["bytes"]) == want, k
            assert np.array_equal(res["lens"], P["alone"][k][0]["lens"])
            coded = res["lens"] > 0
            assert np.array_equal(res["numbps"][coded], P["alone"][k][0]["numbps"][coded])
            assert plan.mq_forms()[1] == mc.enc_k(n, True)
            got = plan.decode_pixels_host(res["bytes"], pix.shape, sop=True, eph=False)
            _forms_in_company(plan.mq_forms(), n, PIX_CB)
            assert plan.mq_forms()[3] == 1
            assert np.array_equal(got, P["back"][k]), k
    finally:
        plan.close()
        ctx.close()


def test_company_batch_of_two_frames(env):
    """the mid geometry as a frame_rows batch of two frames (1614 blocks: K = 7): every frame's tile-part is the one it gets alone, renumbered
    (closed_loop_ref.oracle_batch), and every frame comes back as alone"""
    from j2kgfx import _lib
    torch, orc, t2ref, _ = env
    P = _pixel_frames(orc, t2ref)
    ctx, plan = _pixel_plan(env, frames=2)
    n = int(plan.info.blocks)
    try:
        assert n == mc.case("mid_batch")["n"]
        pix = np.concatenate([f[0] for f in P["frames"]], axis=0)
        d_pix = torch.from_numpy(pix).to(plan.device)
        cs, toffs = plan.encode_frame_pixels(_lib.PIX_RGBA64, d_pix, sop=True, eph=False)
        plan.frame_status()
        forms = plan.mq_forms()
        assert forms[1] == mc.enc_k(n, True) == 7, forms
        h_cs, h_t = cs.cpu().numpy(), toffs.cpu().numpy()
        assert len(P["batch"]) == len(h_t) - 1 == 2
        for k, wt in enumerate(P["batch"]):
            assert bytes(h_cs[int(h_t[k]):int(h_t[k + 1])]) == wt["part"], k
            assert wt["part"][14:] == P["alone"][k][0]["part"][14:]            # as alone, the tile-part header aside
        back = torch.full(pix.shape, 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, int(h_t[-1]), back, tile_offs=toffs, sop=True, eph=False)
        plan.frame_status()
        _forms_in_company(plan.mq_forms(), n, PIX_CB)
        assert plan.mq_forms()[3] == 1
        assert np.array_equal(back.cpu().numpy(), np.concatenate(P["back"], axis=0))
    finally:
        plan.close()
        ctx.close()


# ---- rate, layers, area: the Mallat variant of the mid geometry, 16-bit RGB pixels, with the frame tables test_gpu_layers.Frame holds -------------------
MALLAT_SPEC = ((PIX_W, PIX_H, 3, 16, (0, 0), PIX_NRES), True, 0, PIX_CB)
_MALLAT = {}


@pytest.fixture()
def mallat(env):
    """(plan, Frame): the plan is the test's own on a context of its own; the Frame -- the picture, the oracle's coefficient tiles, the device's
    rate tables -- is made once"""
    import mallat_cases as mal
    import test_gpu_layers as lyr
    import test_gpu_rate_frames as rf
    torch, orc, t2ref = env[:3]
    ctx = env[3](0)
    plan = lyr._plan(ctx, MALLAT_SPEC)
    try:
        if "F" not in _MALLAT:
            pix, planes = _pixel_frames(orc, t2ref)["frames"][0]     # Frame asks test_gpu_rate_frames._frame for its picture: this module's, with the flat part
            case, lossless, q, _ = MALLAT_SPEC
            own, rf._frame = rf._frame, lambda *a: (pix, mal.forward_frame(orc, planes, case[4], case[3], case[5], lossless, q))
            try:
                F = _MALLAT["F"] = lyr.Frame(torch, plan, MALLAT_SPEC)
            finally:
                rf._frame = own
            assert F.pix is pix
            jobs = mc.case("mid")["jobs"]                            # every block's weight from the ORACLE's block list (its resolution field)
            assert F.n == len(jobs)
            w = plan.rate_weights()
            F.ws = [float(w[int(b["comp"]), int(b["res"]), int(b["band"])]) for _, b in jobs]
        yield plan, _MALLAT["F"]
    finally:
        plan.close()
        ctx.close()


def test_company_rate_tables_allocation_and_truncated_decode(env, mallat):
    """encode_blocks(planes=True) in company (the PLANES instantiation of the lanes kernel, K = 4): bytes, numBPS and the rate / distortion tables
    against rate_cases for every block; rate_allocate against rate_cases.allocate; the frame cut to half its bytes decodes, truncated, to the inverse
    of coarse(coefficients, floors) (coarse_cases), through the frame call and through decode_tile_parts + decode_blocks(floors=) + place_blocks"""
    import coarse_cases as cc
    import rate_cases as rc
    import test_gpu_layers as lyr
    import test_gpu_rate_encode as gre
    import test_gpu_rate_frames as rf
    torch, orc, _, _ = env
    plan, F = mallat
    n, (case, lossless, q, cb) = F.n, MALLAT_SPEC
    coeff = plan.forward_pixels(F.fmt, F.d_pix)
    slots, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True)
    plan.ctx.sync()
    forms = plan.mq_forms()
    assert forms[0] >= 3 and forms[1] == mc.enc_k(n, True) == 4 and forms[2] == 0, forms
    R, D = rate.cpu().numpy().view(np.uint32)[:n], dist.cpu().numpy().view(np.uint64)[:n]
    assert np.array_equal(R.astype(np.int64), F.R) and np.array_equal(D, F.D)
    h_slots, so = slots.cpu().numpy(), lyr._slot_offsets(plan)
    h_lens, h_nb = lens.cpu().numpy().view(np.uint32)[:n], nbs.cpu().numpy()[:n]
    bl = plan.blocks()
    for j, (t, c, ys, xs) in enumerate(F.wins):
        v = np.ascontiguousarray(F.ctiles[t][c, ys, xs])
        band = int(bl[j]["band"])
        data, nb = orc.t1_encode(v, v.shape[1], v.shape[0], band)
        assert int(h_lens[j]) == len(data) and int(h_nb[j]) == nb and bytes(h_slots[so[j]:so[j] + len(data)]) == bytes(data), j
        gre._check_tables(orc, v, band, np.asarray(data, np.uint8), nb, R[j], D[j], None)
    assert (h_nb == 0).sum() > n // 8 and len(set(h_nb.tolist())) >= 5          # a picture: blocks without a plane, several depths
    cut_inside = dropped = False
    for budget in (F.U // 10, F.U // 2):
        ps, chosen = rc.allocate(F.R, F.D, F.nbs, F.ws, budget)
        kept, got_chosen = plan.rate_allocate(rate, dist, nbs, budget)
        plan.ctx.sync()
        assert [int(x) for x in kept.cpu().numpy()[:n]] == ps and int(got_chosen.cpu().numpy()[0]) == chosen <= budget
        cut_inside |= any(0 < p < nb for p, nb in zip(ps, F.nbs))
        dropped |= any(p == 0 < nb for p, nb in zip(ps, F.nbs))
    assert cut_inside and dropped                                    # otherwise the comparison is vacuous
    assert any(0 < p < nb for p, nb in zip(ps, F.nbs))               # the frame below: half the bytes, blocks cut inside
    floors = [nb - p for nb, p in zip(F.nbs, ps)]
    cs, toffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=True, eph=True, max_body_bytes=budget)
    plan.frame_status()
    assert plan.mq_forms()[1] == 4
    length = int(toffs[-1].item())
    exp = rf._expected_pixels(orc, case, lossless, q, F.ctiles, F.wins, floors, 0)
    back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
    plan.decode_frame_pixels(cs, length, back, tile_offs=toffs, sop=True, eph=True, truncated=True)
    plan.frame_status()
    _forms_in_company(plan.mq_forms(), n, cb)
    assert plan.mq_forms()[3] == 1
    assert np.array_equal(back.cpu().numpy(), exp)
    o2, l2, n2, f2 = plan.decode_tile_parts(cs, length, sop=True, eph=True, floors=True)
    placed = plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2, floors=f2))
    plan.frame_status()
    _forms_in_company(plan.mq_forms(), n, cb)
    assert plan.mq_forms()[3] == 1
    hp = placed.cpu().numpy()
    cut = [t.copy() for t in F.ctiles]
    for (t, c, ys, xs), k in zip(F.wins, floors):
        cut[t][c, ys, xs] = cc.coarse(F.ctiles[t][c, ys, xs], int(k))
    for t_, c_, _x0, _y0, w_, h_, off in (tuple(int(v) for v in r) for r in plan.planes()):
        assert np.array_equal(hp[off:off + w_ * h_].reshape(h_, w_), cut[t_][c_]), (t_, c_)


def test_company_two_quality_layers(env, mallat):
    """two quality layers ([a quarter of the bytes, everything]) in company: the stream is layer_cases.compose on the yardstick's cuts, and decoding
    one layer and two gives the inverse of the coefficients coarsened to each layer's floors"""
    import layer_cases as lc
    torch, orc, t2ref, _ = env
    plan, F = mallat
    n = F.n
    budgets = [F.U // 4, 1 << 62]
    kept, chosen = lc.allocate_layers(F.R, F.D, F.nbs, F.ws, budgets)
    Q = list(zip(*[lc.normalise(F.R[j], [kept[l][j] for l in range(2)]) for j in range(n)]))
    assert any(0 < q < nb for q, nb in zip(Q[0], F.nbs)) and list(Q[1]) == F.nbs
    want, wtoffs, wloffs = lc.compose(t2ref, F.tiles, F.datas, F.nbs, F.R, kept, True, False)
    cs, toffs, loffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=True, eph=False, layer_bytes=budgets)
    plan.frame_status()
    assert plan.mq_forms()[1] == mc.enc_k(n, True) == 4
    assert toffs.cpu().numpy().tolist() == wtoffs and loffs.cpu().numpy().tolist() == wloffs
    assert bytes(cs.cpu().numpy()[:wtoffs[-1]]) == want
    for k in (1, 2):
        exp = F.expected(orc, MALLAT_SPEC, Q[k - 1], 0, 0)
        back = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, wtoffs[-1], back, tile_offs=toffs if k == 1 else None, sop=True, eph=False, layers=k)
        plan.frame_status()
        _forms_in_company(plan.mq_forms(), n, PIX_CB)
        assert plan.mq_forms()[3] == 1
        assert np.array_equal(back.cpu().numpy(), exp), k
    assert np.array_equal(F.expected(orc, MALLAT_SPEC, Q[1], 0, 0), _pixel_frames(orc, t2ref)["back"][0])      # every layer: the lossless frame


def test_company_area_decode(env, mallat):
    """area= in company: a rectangle across the frame's middle with reduce = 1 -- the decoder is handed the jobs of the resolutions below the top one only,
    fewer than 512, so by the rule it is NOT the plane-stepped one -- and the same rectangle with reduce = 0, where every job goes to the decoder and it is.
    Either way the pixels are the crop of the yardstick's full decode (area_cases.crop)."""
    import area_cases as ac
    torch, orc, _, _ = env
    plan, F = mallat
    n = F.n
    cs, toffs = plan.encode_frame_pixels(F.fmt, F.d_pix, sop=False, eph=True)
    plan.frame_status()
    total = int(toffs[-1].item())
    bpp = ac.bytes_per_pixel(3, 16)
    area = (PIX_W // 2 - 37, PIX_H // 2 - 21, PIX_W // 2 + 50, PIX_H // 2 + 33)
    below_top = sum(1 for _, b in mc.case("mid")["jobs"] if int(b["res"]) < PIX_NRES - 1)
    assert 0 < below_top < 512 <= n
    for r, jobs in ((1, below_top), (0, n)):
        assert ac.area_ok(area, PIX_W, PIX_H, r)
        full = F.expected(orc, MALLAT_SPEC, F.nbs, 0, r)
        h, w = plan.area_shape(area, r)
        back = torch.full((h, w * bpp + 8), 0x5A, dtype=torch.uint8, device=plan.device)
        plan.decode_frame_pixels(cs, total, back, tile_offs=toffs, sop=False, eph=True, reduce=r, area=area)
        plan.frame_status()
        forms = [int(v) for v in plan.mq_forms()]
        assert forms[0] >= 3 and forms[1] == mc.enc_k(n, True)               # (the encode above: all n jobs)
        assert forms[3:] == mc.forms(jobs, PIX_CB, forms[0])[3:], forms      # the decode: `jobs` of them
        assert forms[3] == (1 if jobs >= 512 else 0)
        out = back.cpu().numpy()
        assert np.array_equal(out[:, :w * bpp], ac.crop(full, area, r, bpp)), r
        assert (out[:, w * bpp:] == 0x5A).all()
