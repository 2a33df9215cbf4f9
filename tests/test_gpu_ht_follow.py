"""GPU: what a verified follower costs under ht_dec_dedup (csrc/ht.hip) -- the prep's compare of the READ SET instead of the whole block, the walk in the
plan's slot order with follower-only workgroups that leave, and lists whose leader leaves the lean path (a u of 32 and more: leader and followers
then take the general decoder, the followers on their own bytes -- which may now differ from the leader's outside the read set).  The harness is
test_gpu_ht_dedup.py's: a sentinel-filled `decoded` buffer compared whole, both row modes, option on and off, every call twice (the second on an
idle device), expected values from the C oracle's HTDecoder.Decode of each job's OWN bytes -- never one kernel form against
another.  Cases and definitions: tests/ht_follow_cases.py (checked against the oracle alone in test_ht_follow_cases.py)."""
import numpy as np
import pytest

import ht_dedup_cases as dc
import ht_follow_cases as fc
import ht_stream_cases as hc

pytestmark = pytest.mark.gpu

SENT = -123456789


class _Env:
    """a one-component HT plan per option value, the plan's own bodies, the rule and the walk order"""

    def __init__(self, g):
        import torch
        from j2kgfx import CODER_HT, Context
        from j2kgfx.codec import FramePlan
        self.g, self.torch = g, torch
        self.plans = {}
        for key, on in (("off", 0), ("on", 1)):
            c = Context(0)
            c.set_option("ht_dec_dedup", on)
            self.plans[key] = FramePlan(g["W"], g["H"], 1, precision=8, lossless=True, num_resolutions=g["nres"], cb=g["cb"], coder=CODER_HT, ctx=c)
        p = self.plans["on"]
        self.n = int(p.info.blocks)
        self.blocks = [dict(plane=int(b["plane"]), band=int(b["band"]), x0=int(b["x0"]), y0=int(b["y0"]), w=int(b["w"]), h=int(b["h"])) for b in p.blocks()]
        self.doffs = [int(x) for x in p.decoded_offsets()]
        self.elems = int(p.info.decoded_elems)
        self.rule = dc.leaders(self.blocks, self.doffs)
        self.order, self.nlead = fc.walk_order(self.rule.leaders)
        rng = np.random.default_rng(0xF012)
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
            _ENVS[name] = _Env(dc.GEOMETRIES[name] if name in dc.GEOMETRIES else fc.BIG_PLAN if name == "big" else fc.WALK_PLANS[name])
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


def _run(env, oracle, bodies, what):
    """decode `bodies` (one per job) with the option off and on, both row modes, twice each, into a sentinel-filled buffer; the whole buffer against the
    oracle's decode of every job's own bytes -- so nothing may be written outside the blocks' own elements either"""
    torch = env.torch
    full = np.full(env.elems, SENT, np.int32)
    coded = np.full(env.elems, SENT, np.int32)
    for j, b in enumerate(env.blocks):
        w, h, o = b["w"], b["h"], env.doffs[j]
        want = _want(oracle, w, h, bodies[j])
        full[o:o + w * h] = want.reshape(-1)
        coded[o:o + w * h].reshape(h, w)[0::4] = want[0::4]
        assert not want[1::4].any() and not want[2::4].any() and not want[3::4].any()
    lens = np.array([len(b) for b in bodies], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    raw = np.frombuffer(b"".join(bodies) + b"\xff" * 64, np.uint8)
    for key in ("off", "on"):
        plan = env.plans[key]
        d_stream = torch.from_numpy(raw.copy()).to(plan.device)
        d_offs, d_lens = torch.from_numpy(offs).to(plan.device), torch.from_numpy(lens).to(plan.device)
        nb = torch.zeros(env.n, dtype=torch.uint8, device=plan.device)
        for rows, want in (("all", full), ("coded", coded)):
            plan.set_decode_coded_rows_only(rows == "coded")
            for rep in range(2):
                torch.cuda.synchronize()
                buf = torch.full((env.elems,), SENT, dtype=torch.int32, device=plan.device)
                plan.decode_blocks(d_stream, d_offs, d_lens, nb, decoded=buf)
                plan.ctx.sync()
                got = buf.cpu().numpy()
                if not np.array_equal(got, want):
                    bad = [j for j, b in enumerate(env.blocks) if not np.array_equal(got[env.doffs[j]:env.doffs[j] + b["w"] * b["h"]], want[env.doffs[j]:env.doffs[j] + b["w"] * b["h"]])]
                    raise AssertionError("%s, option %s, rows %s, run %d: %d elements differ; jobs %s (leaders %s, slots %s)" % (
                        what, key, rows, rep, int((got != want).sum()), bad[:8], [env.rule.leaders[j] for j in bad[:8]], [env.order.index(j) for j in bad[:8]]))
        plan.set_decode_coded_rows_only(False)


def _lists(env, shape=None, least=1):
    return [(L, fs) for L, fs in sorted(env.rule.followers.items())
            if len(fs) >= least and (shape is None or (env.blocks[L]["w"], env.blocks[L]["h"]) == shape)]


# ---- the read set ---------------------------------------------------------------------------------------------------------------------------
def test_read_set_edges_in_followers_and_leaders(envs, oracle):
    """every case of ht_follow_cases.edge_cases() in a list of its own, as many per frame as the plan has 16 x 16 lists: the list's last follower (or
    its leader) differs from the others by the case's flip -- inside the read set it decodes on its own bytes, outside it it verifies and its leader's
    rows are its own; either way the buffer is the oracle's"""
    env = envs("136x136_cb16")
    lists = _lists(env, fc.EDGE_SHAPE)
    assert len(lists) >= 12
    cases = fc.edge_cases()
    for k0 in range(0, len(cases), len(lists)):
        bodies = list(env.own)
        for (L, fs), c in zip(lists, cases[k0:k0 + len(lists)]):
            for j in [L] + fs:
                bodies[j] = c.base
            if c.who == "follower":
                bodies[fs[-1]] = c.other
            elif c.who == "leader":
                bodies[L] = c.other
        _run(env, oracle, bodies, "edges %d..: %s" % (k0, "; ".join(c.label for c in cases[k0:k0 + len(lists)])[:400]))


def test_read_set_edges_of_a_block_that_reads_its_magsgn_past_the_first_kilobyte(envs, oracle):
    """ht_follow_cases.big_edge_cases(): a 64 x 64 list (leader and three followers) whose decode reads 1 493 bytes of MagSgn -- flips in the compare's
    second batch and at the piece pulled back to the segment's end decide results here; one frame per case"""
    env = envs("big")
    (L, fs), = _lists(env, fc.BIG_SHAPE)
    assert len(fs) == 3 and env.n == 4
    for c in fc.big_edge_cases():
        bodies = [c.base] * 4
        if c.who == "follower":
            bodies[fs[-1]] = c.other
        elif c.who == "leader":
            bodies[L] = c.other
        _run(env, oracle, bodies, c.label)


# ---- the walk order -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", sorted(fc.WALK_PLANS))
def test_the_plans_walk_order_is_the_python_rule(envs, count):
    env = envs(count)
    mine, rule = fc.plan_rule(env.g)
    assert [(b["band"], b["x0"], b["y0"], b["w"], b["h"]) for b in mine] == [(b["band"], b["x0"], b["y0"], b["w"], b["h"]) for b in env.blocks]
    assert rule.leaders == env.rule.leaders and env.nlead == count
    for key, plan in env.plans.items():
        order, nlead = plan.ht_decode_walk_order()
        assert [int(x) for x in order] == env.order and nlead == count, key
        assert [int(x) for x in plan.ht_decode_leaders()] == env.rule.leaders, key


@pytest.mark.parametrize("count", sorted(fc.WALK_PLANS))
def test_walk_order_with_the_plans_own_stream(envs, oracle, count):
    """every follower verifies: the follower-only workgroups leave at once"""
    env = envs(count)
    for L, fs in env.rule.followers.items():
        assert all(env.own[f] == env.own[L] for f in fs) and len(env.own[L]) >= 4
    _run(env, oracle, env.own, "own stream, %d leaders" % count)


def _failed(env, j):
    """job j's body with its first VLC byte flipped (inside the read set of any block): the prep's compare fails and the job walks"""
    return fc.flip(env.own[j], len(env.own[j]) - 3)


@pytest.mark.parametrize("count", [63, 64, 65, 129])
@pytest.mark.parametrize("kind", ["first_lane", "last_lane", "all"])
def test_follower_only_workgroups_with_followers_that_fail(envs, oracle, count, kind):
    """in every follower-only workgroup (the partial last one included): exactly one follower fails the compare, in the workgroup's first lane / in
    its last lane, or all of them do -- the workgroup then stages and walks like any other"""
    env = envs(count)
    groups = fc.follower_only_groups(env.order, env.nlead)
    assert groups and any(len(jobs) < fc.WALK_BLOCKS for _, jobs in groups) == (count in (63, 65))
    bodies = list(env.own)
    for g, jobs in groups:
        assert all(env.rule.leaders[j] != j for j in jobs)
        for j in {"first_lane": jobs[:1], "last_lane": jobs[-1:], "all": jobs}[kind]:
            bodies[j] = _failed(env, j)
            assert bodies[j] != env.own[env.rule.leaders[j]]
    _run(env, oracle, bodies, "%s of every follower-only workgroup fails, %d leaders" % (kind, count))


def test_a_single_follower_only_workgroup_among_several_has_a_failure(envs, oracle):
    """three follower-only workgroups: the middle one has one failure in its last lane, the others leave"""
    env = envs(64)
    groups = fc.follower_only_groups(env.order, env.nlead)
    assert len(groups) == 3
    bodies = list(env.own)
    j = groups[1][1][-1]
    bodies[j] = _failed(env, j)
    _run(env, oracle, bodies, "one failure in workgroup %d" % groups[1][0])


# ---- a leader off the lean path -------------------------------------------------------------------------------------------------------------
# (plan, block shape, followers of its longest list, whether the plan has a job of that shape that neither leads nor follows anybody -- the rule on
# the CPU: the 16- and the 8-wide plan have a list at the cap of seven and the job the cap turned away; the 32- and 64-wide plans have neither)
BIG_U = [("136x136_cb16", (16, 16), 7, True), ("132x132_cb32", (32, 32), 5, False), ("264x72_cb64x16", (64, 16), 5, False), (63, (8, 8), 7, True)]


@pytest.mark.parametrize("name,shape,longest,has_alone", BIG_U, ids=["w16", "w32", "w64", "w8"])
@pytest.mark.parametrize("changed", ["none", "some"])
@pytest.mark.parametrize("first", ["=32", ">=33"])
def test_leaders_with_u_of_32_and_more(envs, oracle, name, shape, longest, has_alone, changed, first):
    """a u of 32 / of 33 and more in every job of a list: the leader leaves the lean path and the followers the prep verified follow it to the general
    decoder.  The longest list first (at the cap of seven followers in the 16- and 8-wide plans) and the buckets by turns beginning with `first`, so the
    list at the cap runs with both; a job without followers too, where the plan has one; `some`: every other follower carries a byte flipped in its
    MagSgn segment or VLC bytes and decodes on its own, and in the first list with two followers exactly one stays verified (a list of one)."""
    env = envs(name)
    w, h = shape
    sufs = fc.big_u_suffixes(w, h)
    buckets = ("=32", ">=33") if first == "=32" else (">=33", "=32")
    rng = np.random.default_rng(0xF013)
    lists = sorted(_lists(env, shape), key=lambda t: -len(t[1]))
    assert len(lists) >= 4 and len(lists[0][1]) == longest and (longest == dc.MAX_FOLLOWERS) == has_alone
    bodies = list(env.own)
    for k, (L, fs) in enumerate(lists[:6]):
        body = hc.splice(hc._rand(rng, (0, 5, 300, 1100)[k % 4]), sufs[buckets[k % 2]])
        assert hc.bucket_of(hc.classify(body, w, h).max_u) == buckets[k % 2]
        for j in [L] + fs:
            bodies[j] = body
        if changed == "some":
            for f in fs[1::2]:
                bodies[f] = fc.flip(body, len(body) - 3 if len(fs) % 2 else 0)
            assert sum(1 for f in fs if bodies[f] == body) >= 1
    two = [(L, fs) for L, fs in lists[:6] if len(fs) == 2]
    assert two, "a list with two followers among those that carry the streams"
    assert sum(1 for f in two[0][1] if bodies[f] == bodies[two[0][0]]) == (1 if changed == "some" else 2)
    alone = [j for j, b in enumerate(env.blocks) if (b["w"], b["h"]) == shape and env.rule.leaders[j] == j and j not in env.rule.followers]
    assert bool(alone) == has_alone
    if has_alone:
        bodies[alone[0]] = hc.splice(b"", sufs[buckets[1]])
    _run(env, oracle, bodies, "u >= 32 in %d lists of %dx%d, changed: %s, first: %s" % (min(len(lists), 6), w, h, changed, first))
