"""GPU: HT block decode with byte-identical blocks decoded once (context option ht_dec_dedup: ht_vlcprep_dedup_kernel, ht_walk_kernel<true>,
ht_decode_lean_kernel<false, true>, csrc/ht.hip) against the same call with the option off and against the C oracle's HTDecoder.Decode of every
job's OWN bytes -- bit for bit over the whole `decoded` buffer, sentinel-prefilled, in both row modes, every call twice.

The plan's table only names candidates (tests/ht_dedup_cases.py is its definition); whether a job is skipped is decided from the bytes of the
call.  So every case below is a frame whose jobs carry chosen bodies: the plan's own stream (every list verifies), then one byte of a follower /
of a leader changed in each part of the block, a length changed, refused streams, streams with u >= 32 (the lean path's exit to the general
decoder: leader and followers then each decode themselves), and frames where only some lists verify."""
import numpy as np
import pytest

import ht_dedup_cases as dc
import ht_stream_cases as hc

pytestmark = pytest.mark.gpu

SENT = -123456789
GEOS = sorted(dc.GEOMETRIES)


class _Env:
    """per geometry: a plan per option value (and the inert combinations), the plan's own bodies, the rule"""

    def __init__(self, name):
        import torch
        from j2kgfx import CODER_HT, Context
        from j2kgfx.codec import FramePlan
        g = dc.GEOMETRIES[name]
        self.g, self.torch = g, torch
        self.plans, self.ctxs = {}, []
        for key, opts in (("off", dict(ht_dec_dedup=0)), ("on", dict(ht_dec_dedup=1)), ("on_front1", dict(ht_dec_dedup=1, ht_dec_front=1)),
                          ("on_lean0", dict(ht_dec_dedup=1, ht_dec_lean=0))):
            c = Context(0)
            for k, v in opts.items():
                c.set_option(k, v)
            self.ctxs.append(c)
            self.plans[key] = FramePlan(g["W"], g["H"], 1, precision=8, lossless=True, num_resolutions=g["nres"], cb=g["cb"], coder=CODER_HT, ctx=c)
        p = self.plans["on"]
        self.n = int(p.info.blocks)
        self.blocks = [dict(plane=int(b["plane"]), band=int(b["band"]), x0=int(b["x0"]), y0=int(b["y0"]), w=int(b["w"]), h=int(b["h"])) for b in p.blocks()]
        self.doffs = [int(x) for x in p.decoded_offsets()]
        self.elems = int(p.info.decoded_elems)
        self.rule = dc.leaders(self.blocks, self.doffs)
        rng = np.random.default_rng(0x9a01)
        frame = torch.from_numpy(rng.integers(0, 256, size=(1, g["H"], g["W"])).astype(np.int32)).to(p.device)
        stream, offs, lens, _ = p.encode_stream(p.forward(frame))
        p.ctx.sync()
        hs, ho, hl = stream.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()
        self.own = [bytes(hs[int(ho[j]):int(ho[j]) + int(hl[j])]) for j in range(self.n)]

    def close(self):
        for p in self.plans.values():
            p.close()


_ENVS = {}


@pytest.fixture(scope="module")
def envs():
    def get(name):
        if name not in _ENVS:
            _ENVS[name] = _Env(name)
        return _ENVS[name]
    yield get
    for e in _ENVS.values():
        e.close()
    _ENVS.clear()


_WANT = {}


def _want(oracle, w, h, data):
    key = (w, h, data)
    if key not in _WANT:
        _WANT[key] = oracle.ht_decode(np.frombuffer(data, np.uint8), w, h)
    return _WANT[key]


def _expected(env, oracle, bodies):
    """the whole buffer after a call into a sentinel-filled one: (every row written, coded rows only)"""
    full = np.full(env.elems, SENT, np.int32)
    coded = np.full(env.elems, SENT, np.int32)
    for j, b in enumerate(env.blocks):
        w, h, o = b["w"], b["h"], env.doffs[j]
        want = _want(oracle, w, h, bodies[j])
        full[o:o + w * h] = want.reshape(-1)
        coded[o:o + w * h].reshape(h, w)[0::4] = want[0::4]
        assert not want[1::4].any() and not want[2::4].any() and not want[3::4].any()
    return full, coded


def _run(env, oracle, bodies, what, keys=("off", "on")):
    torch = env.torch
    lens = np.array([len(b) for b in bodies], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    raw = np.frombuffer(b"".join(bodies) + b"\xff" * 64, np.uint8)
    full, coded = _expected(env, oracle, bodies)
    for key in keys:
        plan = env.plans[key]
        d_stream = torch.from_numpy(raw.copy()).to(plan.device)
        d_offs, d_lens = torch.from_numpy(offs).to(plan.device), torch.from_numpy(lens).to(plan.device)
        nb = torch.zeros(env.n, dtype=torch.uint8, device=plan.device)
        for rows, want in (("all", full), ("coded", coded)):
            plan.set_decode_coded_rows_only(rows == "coded")
            for rep in range(2):                                  # the second call starts on an idle device
                torch.cuda.synchronize()
                buf = torch.full((env.elems,), SENT, dtype=torch.int32, device=plan.device)
                plan.decode_blocks(d_stream, d_offs, d_lens, nb, decoded=buf)
                plan.ctx.sync()
                got = buf.cpu().numpy()
                if not np.array_equal(got, want):
                    bad = [j for j, b in enumerate(env.blocks) if not np.array_equal(got[env.doffs[j]:env.doffs[j] + b["w"] * b["h"]], want[env.doffs[j]:env.doffs[j] + b["w"] * b["h"]])]
                    raise AssertionError("%s, option %s, rows %s, run %d: %d elements differ; jobs %s (leaders %s)" % (
                        what, key, rows, rep, int((got != want).sum()), bad[:8], [env.rule.leaders[j] for j in bad[:8]]))
        plan.set_decode_coded_rows_only(False)


def _flip(data, pos):
    b = bytearray(data)
    b[pos] ^= 0x55
    return bytes(b)


def _parts(data, w, h):
    """positions inside the MagSgn segment, the MEL run's interior (or None), the VLC segment, the trailer of a block the encoder wrote"""
    n, scup = len(data), hc.scup_of(data)
    assert 2 <= scup <= n
    N = ((h + 3) // 4) * (((w + 3) // 4 + 1) // 2)
    nvlc = min(scup - 2, (46 * N + 7) // 8 + 8)
    mel_lo, mel_hi = n - scup + 4, n - 2 - nvlc                  # past the bytes init_mel_ok looks at, below the VLC bytes the prep takes
    return dict(magsgn=(n - scup) // 2 if n > scup else None, mel=(mel_lo + mel_hi) // 2 if mel_hi - mel_lo >= 1 else None, vlc=n - 3 if scup >= 3 else None, trailer=n - 1)


def _lists(env, least=1):
    return [(L, fs) for L, fs in sorted(env.rule.followers.items()) if len(fs) >= least]


# ---- the table ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOS)
def test_the_plans_table_is_the_python_rule(envs, name):
    env = envs(name)
    g = env.g
    mine = dc.block_list(g["W"], g["H"], g["nres"], g["cb"])
    assert [(b["band"], b["x0"], b["y0"], b["w"], b["h"]) for b in mine] == [(b["band"], b["x0"], b["y0"], b["w"], b["h"]) for b in env.blocks]
    assert env.doffs == dc.decoded_offsets(mine)
    for key, plan in env.plans.items():
        assert [int(x) for x in plan.ht_decode_leaders()] == env.rule.leaders, key
    if name == "136x136_cb16":
        assert max(len(fs) for fs in env.rule.followers.values()) == dc.MAX_FOLLOWERS and "cap" in env.rule.refused.values()


def test_a_closed_loop_plan_has_no_candidates_and_an_mq_plan_no_table(envs):
    from j2kgfx import CODER_HT, CODER_MQ, J2KError
    from j2kgfx.codec import FramePlan
    p = FramePlan(136, 136, 1, num_resolutions=5, cb=(16, 16), coder=CODER_HT, closed_loop=True)
    assert [int(x) for x in p.ht_decode_leaders()] == list(range(int(p.info.blocks)))
    p.close()
    p = FramePlan(136, 136, 1, num_resolutions=5, cb=(16, 16), coder=CODER_MQ)
    with pytest.raises(J2KError):
        p.ht_decode_leaders()
    p.close()


# ---- streams ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOS)
def test_the_plans_own_stream(envs, oracle, name):
    env = envs(name)
    for L, fs in env.rule.followers.items():
        assert all(env.own[f] == env.own[L] for f in fs) and len(env.own[L]) >= 4, "jobs of one window carry the same bytes"
    _run(env, oracle, env.own, "own stream", keys=("off", "on", "on_front1", "on_lean0"))


@pytest.mark.parametrize("name", GEOS)
@pytest.mark.parametrize("part", ["magsgn", "mel", "vlc", "trailer", "lens"])
def test_one_byte_of_a_follower_changed(envs, oracle, name, part):
    """in every list: its last follower differs from the leader in one byte of that part (or is one byte shorter); it decodes on its own bytes"""
    env = envs(name)
    bodies, hit = list(env.own), 0
    for L, fs in _lists(env):
        f = fs[-1]
        if part == "lens":
            bodies[f] = env.own[f][:-1]
            hit += 1
            continue
        pos = _parts(env.own[f], env.blocks[f]["w"], env.blocks[f]["h"])[part]
        if pos is not None:
            bodies[f] = _flip(env.own[f], pos)
            hit += 1
    assert hit >= 3
    _run(env, oracle, bodies, "follower: " + part)


@pytest.mark.parametrize("name", GEOS)
@pytest.mark.parametrize("part", ["magsgn", "vlc"])
def test_one_byte_of_a_leader_changed(envs, oracle, name, part):
    env = envs(name)
    bodies = list(env.own)
    for L, fs in _lists(env):
        pos = _parts(env.own[L], env.blocks[L]["w"], env.blocks[L]["h"])[part]
        if pos is not None:
            bodies[L] = _flip(env.own[L], pos)
    _run(env, oracle, bodies, "leader: " + part)


@pytest.mark.parametrize("name", GEOS)
def test_refused_streams_in_leader_and_followers(envs, oracle, name):
    """len < 2 in every job of one list, a SCUP field below 2 in every job of the next, SCUP > len in a third (the cases of ht_stream_cases group V's kinds)"""
    env = envs(name)
    bodies = list(env.own)
    lists = _lists(env)
    for k, (L, fs) in enumerate(lists[:3]):
        good = env.own[L]
        bad = (b"\x5a", hc.with_scup(good, 1), hc.with_scup(good[:40], len(good[:40]) + 1))[k]
        info = hc.classify(bad, env.blocks[L]["w"], env.blocks[L]["h"])
        assert info.reject == ("len<2", "scup<2", "scup>len")[k]
        for j in [L] + fs:
            bodies[j] = bad
    _run(env, oracle, bodies, "refused lists")


def test_streams_with_u_of_32_and_more_in_whole_lists(envs, oracle):
    """the lean path's exit: M("=32") and M(">=33") of the 16 x 16 shape in every job of a list (the list at the cap among them)"""
    env = envs("136x136_cb16")
    pool = {b: [c for c in hc.group_M() if (c.w, c.h) == (16, 16) and c.bucket == b and len(c.data) >= 4] for b in ("=32", ">=33")}
    assert all(len(v) >= 2 for v in pool.values())
    bodies = list(env.own)
    lists = [(L, fs) for L, fs in _lists(env) if (env.blocks[L]["w"], env.blocks[L]["h"]) == (16, 16)]
    assert len(lists) >= 4 and len(lists[0][1]) == dc.MAX_FOLLOWERS
    for k, (L, fs) in enumerate(lists[:4]):
        c = pool[("=32", ">=33")[k % 2]][k // 2]
        for j in [L] + fs:
            bodies[j] = c.data
    _run(env, oracle, bodies, "u >= 32 lists")


@pytest.mark.parametrize("name", GEOS)
def test_mixed_frames_where_only_some_lists_verify(envs, oracle, name):
    env = envs(name)
    rng = np.random.default_rng(0x9a02)
    bodies = list(env.own)
    for k, (L, fs) in enumerate(_lists(env)):
        if k % 2:
            continue
        for f in fs[::2]:                                         # every other follower of every other list: a fresh body of its shape
            bodies[f] = hc.encoder_output(rng, env.blocks[f]["w"], env.blocks[f]["h"], 300)
    _run(env, oracle, bodies, "mixed", keys=("off", "on", "on_front1", "on_lean0"))


def test_closed_loop_ht_round_trip_is_unchanged(oracle):
    """the closed-loop frame codec never sees the tables (its windows partition the plane; its decoder writes them in place): tile-parts and
    pixels with the option on == off, the frame call == the stage calls (parse, j2k_plan_decode_blocks, placement, inverse)"""
    import torch
    from closed_loop_ref import frame as make_frame
    from j2kgfx import Context, _lib
    from j2kgfx.codec import FramePlan
    geo = hc.PLANS[1]
    W, H = geo["W"], geo["H"]
    frm = make_frame(W, H, 31, noise=40)
    rgba = np.ascontiguousarray(np.concatenate([frm.transpose(1, 2, 0), np.full((H, W, 1), 255, np.uint8)], axis=2).reshape(H, W * 4))
    got = {}
    for on in (0, 1):
        c = Context(0)
        c.set_option("ht_dec_dedup", on)
        plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=geo["nres"], cb=(geo["cb"], geo["cb"]), tile=geo["tile"], coder=_lib.CODER_HT, closed_loop=True, ctx=c)
        assert [int(x) for x in plan.ht_decode_leaders()] == list(range(int(plan.info.blocks)))
        d_pix = torch.from_numpy(rgba).to(plan.device)
        stream, offs, lens, numbps = plan.encode_stream(plan.forward_pixels(_lib.PIX_RGBA8, d_pix))
        plan.frame_status()
        cs, toffs = plan.encode_tile_parts(stream, offs, lens, numbps, sop=True, eph=True)
        plan.frame_status()
        total = int(toffs[-1].item())
        o2, l2, n2 = plan.decode_tile_parts(cs, total, tile_offs=toffs, sop=True, eph=True)
        plan.frame_status()
        staged = plan.inverse_pixels(plan.place_blocks(plan.decode_blocks(cs, o2, l2, n2)), torch.zeros_like(d_pix))
        plan.frame_status()
        out = torch.zeros_like(d_pix)
        plan.decode_frame_pixels(cs, total, out, tile_offs=toffs, sop=True, eph=True)
        plan.frame_status()
        assert torch.equal(out, staged)
        got[on] = (cs.cpu().numpy()[:total].copy(), out.cpu().numpy())
        plan.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert got[1][1].reshape(H, W, 4)[:, :, :3].std() > 1        # (the reference's HT coder codes one row in four: no identity to compare with)
