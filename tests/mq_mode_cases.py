"""The MQ block coder's own choice between its latency and its throughput setting, restated, and the plans that make every part of the
choice move -- importable without a GPU: tests/test_mq_mode_cases.py checks this module with the oracle alone, tests/test_gpu_mq_modes.py
and its child process tests/helpers_mq_modes.py hold the device to it.

The library counts the live contexts of the process that have built an MQ-coder plan (a context once, whatever it builds afterwards; an
HT plan does not count).  "alone" = that count is below 2, "in company" = 2 or more.  What hangs on it, with n the jobs of the call:

    block encode, blocks <= 64 x 64    K blocks per wavefront of the MQ chains: ceil(n / 2048) alone, min(64, ceil(n / 256)) in company
    block encode, blocks above 64      one fused kernel alone, two kernels through symbol lists in company
    block decode                       the plane-stepped path from 12 000 blocks alone, from 512 in company -- if the stream is 16-byte
                                       aligned (a plan call; the host call copies the bytes to an aligned buffer) and its workspace can be had
    block decode, blocks above 64      one launch alone, two (two sizes of block state) in company; the host call j2k_decode_blocks always one

FramePlan.mq_forms() / Context.mq_forms() report what a call took; forms() below is what they must say with nothing forced.

Contents are COEFFICIENTS (int32 planes handed to the block coder, no transform in front), so that every reference is the oracle's block
coder and nothing else: oracle.encode_tile_blocks per tile for the encoder, oracle.t1_decode per block for the decoder."""
import functools

import numpy as np

SPLIT_MIN_ALONE, SPLIT_MIN_COMPANY = 12000, 512
DEC_LANES = 2                                   # the plane-stepped decoder's default form (context option t1_dec_lanes)


def in_company(live):
    return live >= 2


def enc_k(n, company):
    k = min(64, -(-n // 256)) if company else -(-n // 2048)
    return min(64, max(1, k))


def dec_split(n, company):
    return n >= (SPLIT_MIN_COMPANY if company else SPLIT_MIN_ALONE)


def forms(n, max_dim, live, aligned=True, host_call=False, encoded=True, decoded=True):
    """what mq_forms() must report after a block encode and a block decode of n jobs whose largest block side is max_dim, with `live` counted
    contexts alive; host_call: Context.mq_forms() after entropy.decode_blocks (no encode record, the big-block decoder as one launch)"""
    company = in_company(live)
    big = max_dim > 64
    want = dec_split(n, company)
    took = want and aligned
    return [live,
            enc_k(n, company) if encoded and not host_call else 0,
            1 if encoded and not host_call and big and company else 0,
            1 if decoded and took else 0,
            DEC_LANES if decoded and took else 0,
            (0 if not big else 2 if company and not host_call else 1) if decoded else 0,
            1 if decoded and want and not took else 0,
            0]


# ---- the plans: closed-loop MQ plans (the windows partition every tile-component), chosen by block count ------------------------------------
# name: W, H, components, resolutions, code-block side, tile, frames (> 1: a frame_rows batch of that many frames of H rows), and the bracket its
# block count must lie in
PLANS = {
    "small":     dict(W=96, H=80, C=3, nres=3, cb=32, tile=(0, 0), frames=1, bracket=(1, 255)),
    "mid":       dict(W=272, H=200, C=3, nres=3, cb=16, tile=(0, 0), frames=1, bracket=(600, 1100)),
    "mid_tiled": dict(W=264, H=200, C=3, nres=4, cb=16, tile=(112, 96), frames=1, bracket=(600, 1100)),       # 3 x 3 tiles, the last column 40 wide, the last row 8 high
    "mid_576":   dict(W=256, H=192, C=3, nres=3, cb=16, tile=(0, 0), frames=1, bracket=(512, 599)),           # just above the decoder's threshold in company
    "mid_cb8":   dict(W=136, H=100, C=3, nres=3, cb=8, tile=(0, 0), frames=1, bracket=(512, 1100)),          # a quarter of mid's samples (the raw-MagRef style's reference is Python)
    "mid_batch": dict(W=272, H=200, C=3, nres=3, cb=16, tile=(0, 0), frames=2, bracket=(1200, 2200)),
    "big128":    dict(W=384, H=200, C=3, nres=5, cb=128, tile=(0, 0), frames=1, bracket=(1, 511)),            # test_gpu_t1_big's mixed geometry, two more resolutions for small blocks
    "big256":    dict(W=520, H=330, C=1, nres=5, cb=256, tile=(0, 0), frames=1, bracket=(1, 511)),
    "bigmid":    dict(W=616, H=458, C=3, nres=5, cb=128, tile=(144, 136), frames=1, bracket=(512, 1100)),     # 5 x 4 tiles: the 72 x 68 bands of the full tiles are one block each
}
FAMILIES = {"mid": ("mid", "mid_tiled"), "big": ("big128", "big256"), "bigmid": ("bigmid",)}     # one child process each (tests/helpers_mq_modes.py)
PRECISION = 12


def tiles_of(p):
    """[(frame, tile of the frame, x0, y0 in the batch, w, h)] in the plan's tile order (frame 0's tiles first)"""
    tw, th = p["tile"][0] or p["W"], p["tile"][1] or p["H"]
    tx, ty = -(-p["W"] // tw), -(-p["H"] // th)
    out = []
    for f in range(p["frames"]):
        for t in range(tx * ty):
            x0, y0 = (t % tx) * tw, (t // tx) * th
            out.append((f, t, x0, f * p["H"] + y0, min(tw, p["W"] - x0), min(th, p["H"] - y0)))
    return out


def jobs_of(oracle, p):
    """the plan's job list by the oracle: [(tile index, oracle block record)] in job order"""
    out = []
    for i, (_, _, _, _, w, h) in enumerate(tiles_of(p)):
        out += [(i, b) for b in oracle.enumerate_blocks(p["C"], w, h, p["nres"], p["cb"], p["cb"], 1)]
    return out


def coefficients(p, seed, tiles, jobs):
    """int32 [C, frames * H, W] coefficient planes, filled window by window of the job list so that blocks of every size get every kind of content:
    job j is flat zero for j % 8 in (0, 3) (a quarter of the blocks have no plane at all), sparse for j % 8 == 5 (one sample in fifty set, magnitudes
    up to 2^20), and noise of 1 + (5 j) % 13 bits otherwise (a spread of bit-plane counts among neighbours in the job order)"""
    rng = np.random.default_rng(seed)
    x = np.zeros((p["C"], p["frames"] * p["H"], p["W"]), np.int64)
    for j, (t, b) in enumerate(jobs):
        _, _, x0, y0, _, _ = tiles[t]
        w, h = int(b["w"]), int(b["h"])
        if j % 8 in (0, 3):
            continue
        if j % 8 == 5:
            v = np.where(rng.random((h, w)) < 0.02, rng.integers(-(1 << 20), 1 << 20, (h, w)), 0)
            v.reshape(-1)[int(rng.integers(0, w * h))] = 1 << 19
        else:
            bits = 1 + (5 * j) % 13
            v = rng.integers(-(1 << bits) + 1, 1 << bits, (h, w))
            v.reshape(-1)[int(rng.integers(0, w * h))] = (1 << bits) - 1
        x[int(b["comp"]), y0 + int(b["y0"]):y0 + int(b["y0"]) + h, x0 + int(b["x0"]):x0 + int(b["x0"]) + w] = v
    return x.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(name, seed):
    import oracle
    oracle.lib()
    p = PLANS[name]
    tiles = tiles_of(p)
    jobs = jobs_of(oracle, p)
    coeff = coefficients(p, seed, tiles, jobs)
    data, lens, nbs = [], [], []
    for (_, _, x0, y0, w, h) in tiles:
        by, ln, nb = oracle.encode_tile_blocks([np.ascontiguousarray(coeff[c, y0:y0 + h, x0:x0 + w]) for c in range(p["C"])], w, h, p["nres"], p["cb"], p["cb"], 0, windows=1)
        data.append(by); lens.append(ln); nbs.append(nb)
    lens, nbs = np.concatenate(lens).astype(np.uint32), np.concatenate(nbs).astype(np.uint8)
    assert len(jobs) == lens.size
    return dict(name=name, plan=p, coeff=coeff, tiles=tiles, jobs=jobs, bytes=np.concatenate(data), lens=lens, numbps=nbs,
                n=len(jobs), max_dim=max(max(int(b["w"]), int(b["h"])) for _, b in jobs))


def case(name, seed=0):
    """The plan `name` with contents: dict(plan, coeff, tiles, jobs, bytes, lens, numbps, n, max_dim) -- bytes / lens / numbps are the oracle's
    encode of every job in job order (computed once per process; do not write into them)."""
    return _case(name, 20261 + 7 * seed + sum(map(ord, name)))


def decode_streams(oracle, c, seed=0):
    """The decoder's inputs for the jobs of a case, and what the oracle decodes from them: [(label, bytes uint8, offs uint64 [n + 1], lens uint32,
    numbps uint8, [expected block (h, w) int32])].
      "encoded":   the oracle's encode, with the bit-plane count of every 37th coded block of at most 64 x 64 raised by 16 -- 32 planes and more, which
                   the plane-stepped decoder must leave to the one-launch kernel (coarse_cases.deep's recipe; deep_jobs() says which);
      "arbitrary": bytes no encoder wrote -- random lengths from 0 (every fifth job has no bytes at all), every seventh job 0xFF-rich, bit-plane
                   counts 0 ... 14 and 33 on every 41st job."""
    n = c["n"]
    out = []
    nb = c["numbps"].copy()
    deep = deep_jobs(c)
    nb[deep] += 16
    offs = np.concatenate(([0], np.cumsum(c["lens"].astype(np.uint64)))).astype(np.uint64)
    out.append(("encoded", c["bytes"], offs, c["lens"], nb))
    rng = np.random.default_rng(977 + seed + n)
    ln = np.zeros(n, np.uint32)
    chunks = []
    nb2 = np.zeros(n, np.uint8)
    for j, (_, b) in enumerate(c["jobs"]):
        w, h = int(b["w"]), int(b["h"])
        k = 0 if j % 5 == 0 else int(rng.integers(1, min(2 * w * h, 1200) + 8))
        g = rng.integers(0, 256, k).astype(np.uint8)
        if j % 7 == 0 and k:
            g[rng.integers(0, k, k // 3 + 1)] = 0xFF
        chunks.append(g)
        ln[j] = k
        nb2[j] = 33 if j % 41 == 40 and max(w, h) <= 64 else j % 15
    offs2 = np.concatenate(([0], np.cumsum(ln.astype(np.uint64)))).astype(np.uint64)
    out.append(("arbitrary", np.concatenate(chunks), offs2, ln, nb2))
    res = []
    for label, by, of, l, nbv in out:
        want = [oracle.t1_decode(by[int(of[j]):int(of[j]) + int(l[j])], int(nbv[j]), int(b["band"]), int(b["w"]), int(b["h"]))
                for j, (_, b) in enumerate(c["jobs"])]
        res.append((label, by, of, l, nbv, want))
    return res


def deep_jobs(c):
    """the jobs whose bit-plane count decode_streams() raises by 16: every 37th of the coded jobs of at most 64 x 64 with 16 planes or more"""
    ok = [j for j, (_, b) in enumerate(c["jobs"]) if c["lens"][j] > 0 and c["numbps"][j] >= 16 and max(int(b["w"]), int(b["h"])) <= 64]
    return np.array(ok[::37], dtype=np.int64)


def plan_kwargs(p, **more):
    """FramePlan(**plan_kwargs(PLANS[name])) is the plan (coder 0 = MQ)"""
    kw = dict(width=p["W"], height=p["H"] * p["frames"], ncomp=p["C"], precision=PRECISION, lossless=True, num_resolutions=p["nres"],
              cb=(p["cb"], p["cb"]), tile=p["tile"], coder=0, closed_loop=True)
    if p["frames"] > 1:
        kw["frame_rows"] = p["H"]
    kw.update(more)
    return kw


def coeff_buffer(c, planes, elems):
    """the plan's coefficient buffer (int32 [elems]) holding the case's planes: planes = FramePlan.planes(), rows (tile, comp, x0, y0, w, h, offset)"""
    buf = np.zeros(int(elems), np.int32)
    for row in planes:
        t, comp, off = int(row[0]), int(row[1]), int(row[6])
        _, _, x0, y0, w, h = c["tiles"][t]
        assert (int(row[4]), int(row[5])) == (w, h), (row, c["tiles"][t])
        buf[off:off + w * h] = c["coeff"][comp, y0:y0 + h, x0:x0 + w].reshape(-1)
    return buf
