"""GPU: the four-wave workgroup form of the HT block encoder (ht_encode_wg_kernel, option ht_enc_waves = 4) against the oracle
encoder and against the one-wave form (ht_enc_waves = 1), through j2k_plan_encode_stream -- the only caller that has the alias
tables the form needs.

A plane of 2w x 2h samples with two resolutions has ONE distinct window, w x h at the top left, shared by the LL block and the
three bands above it (the reference addresses every band from the top left of the plane), so a plan of such planes puts
blocks of a chosen size and content in front of the kernel; every component is another window.  Compared per job: the bytes
of the dense stream (the slot's MagSgn bytes, the MEL zeros the gather inserts where the kernel's MagSgn length says, the VLC
bytes and the trailer -- a wrong MagSgn length moves the zeros, so it shows as wrong bytes), `lens`, `numbps`, the offsets, and
the fault raised at the next synchronisation.  Every case runs a second time after a device synchronisation, on an idle device.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MININT = -2147483648


@pytest.fixture(scope="module")
def ctxs():
    """(one-wave context, four-wave context)"""
    from j2kgfx import Context
    out = []
    for waves in (1, 4):
        c = Context(0)
        c.set_option("ht_enc_waves", waves)
        out.append(c)
    return out


def _encode(ctx, planes, nres, cb):
    """two runs of encode_stream on planes [(H, W) int32] taken as coefficients: [(per-job bytes, lens, numbps, offs, fault)] * 2"""
    import torch
    from j2kgfx import J2KError
    from j2kgfx.codec import FramePlan
    H, W = planes[0].shape
    plan = FramePlan(W, H, len(planes), precision=8, lossless=True, num_resolutions=nres, cb=(cb, cb), coder=1, ctx=ctx)
    host = np.zeros(int(plan.info.coeff_elems), np.int32)
    for tile, comp, x0, y0, w, h, off in plan.planes():
        assert (tile, x0, y0, w, h) == (0, 0, 0, W, H)
        host[off:off + w * h] = planes[comp].reshape(-1)
    coeff = plan.alloc_coeff()
    coeff[:host.size].copy_(torch.from_numpy(host))
    n = int(plan.info.blocks)
    runs = []
    for rep in range(2):
        torch.cuda.synchronize()                                   # the second run starts on an idle device
        stream, offs, lens, nb = plan.encode_stream(coeff)
        fault = False
        try:
            ctx.sync()
        except J2KError:
            fault = True
        o, l = offs.cpu().numpy()[:n + 1].astype(np.int64), lens.cpu().numpy()[:n].astype(np.uint32)
        s = stream.cpu().numpy()
        runs.append(([bytes(s[o[j]:o[j] + int(l[j])]) for j in range(n)], l, nb.cpu().numpy()[:n].copy(), o, fault))
    plan.close()
    return runs


def _want(oracle, planes, nres, cb):
    """the oracle's coder on every job's window: (per-job bytes, lens, numbps or None, fault); a job in the reference's panic domain
    (MinInt32 in a coded position) has no bytes, and the tile coder then has no bit-plane counts either"""
    H, W = planes[0].shape
    jobs = oracle.enumerate_blocks(len(planes), W, H, nres, cb, cb)
    want, fault = [], False
    for b in jobs:
        x0, y0, w, h = int(b["x0"]), int(b["y0"]), int(b["w"]), int(b["h"])
        win = np.ascontiguousarray(planes[int(b["comp"])][y0:y0 + h, x0:x0 + w])
        try:
            want.append(bytes(oracle.ht_encode(win, w, h)))
        except ValueError:
            want.append(b""); fault = True
    nb = None
    if not fault:
        by, ln, nb = oracle.encode_tile_blocks(planes, W, H, nres, cb, cb, 1)
        assert bytes(by) == b"".join(want) and [int(x) for x in ln] == [len(x) for x in want]
        # The reference's tile encoder keeps no bit-plane count for this coder; the oracle's helper takes the bit length of the
        # largest UNSIGNED magnitude, the coder itself (ht.go:947-966) and both kernel forms compare int32, where -MinInt32
        # stays negative and never wins.  They differ only for a coded block that holds MinInt32: the coder's rule there.
        for j, b in enumerate(jobs):
            x0, y0, w, h = int(b["x0"]), int(b["y0"]), int(b["w"]), int(b["h"])
            win = planes[int(b["comp"])][y0:y0 + h, x0:x0 + w]
            if want[j] and (win == MININT).any():
                nb[j] = int(np.abs(win[win != MININT]).max()).bit_length()
    return jobs, want, np.array([len(x) for x in want], np.uint32), nb, fault


def _check(oracle, ctxs, planes, nres=2, cb=64):
    planes = [np.ascontiguousarray(p, dtype=np.int32) for p in planes]
    jobs, want, wl, wnb, wfault = _want(oracle, planes, nres, cb)
    one = _encode(ctxs[0], planes, nres, cb)
    four = _encode(ctxs[1], planes, nres, cb)
    for rep, (got, ref) in enumerate(zip(four, one)):
        by, ln, nb, offs, fault = got
        assert fault == wfault == ref[4], rep
        assert np.array_equal(ln, ref[1]) and np.array_equal(nb, ref[2]) and np.array_equal(offs, ref[3]), rep
        assert by == ref[0], rep
        assert np.array_equal(np.diff(offs), ln.astype(np.int64)), rep
        for j in range(len(jobs)):                                 # (a faulted block has length 0; the others are the oracle's as ever)
            assert by[j] == want[j], (rep, j, tuple(jobs[j]))
        assert np.array_equal(ln, wl), rep
        if wnb is not None:
            assert np.array_equal(nb, wnb), rep
    return jobs, want


def _window(w, h, block):
    """block (h, w) at the top left of a 2w x 2h plane; the rest is noise that no job reads"""
    p = np.random.default_rng(w * 64 + h).integers(-5, 6, (2 * h, 2 * w)).astype(np.int32)
    p[:h, :w] = block
    return p


@pytest.mark.parametrize("w", [4, 8, 60, 64])
@pytest.mark.parametrize("h", [1, 3, 4, 5, 61, 64])
def test_block_sizes(oracle, ctxs, w, h):
    """every width x height of the four-wave path's edges (one quad per row ... sixteen; one coded row ... sixteen, a last stripe of
    1, 3 or 4 rows): noise of ~9 bits with holes, +-1 magnitudes and magnitudes of 30 bits, three windows per plan"""
    rng = np.random.default_rng(1000 * w + h)
    a = rng.integers(-300, 301, (h, w)); a[rng.random((h, w)) < 0.3] = 0
    b = rng.choice([-1, 1], (h, w))
    c = rng.integers(-(1 << 30), 1 << 30, (h, w))
    _check(oracle, ctxs, [_window(w, h, x) for x in (a, b, c)])


def test_block_contents(oracle, ctxs):
    """64 x 64 windows: all zero (nil); the only non-zero sample in an uncoded row (numbps from the whole block, all coded quads empty);
    +-1 (1-bit MagSgn fields: runs of 0xFF candidates), all -1 (every MagSgn byte 0xFF or its 7-bit successor); magnitudes with u
    near 31; MinInt32 in an uncoded row beside coded samples (no fault: it never wins the int32 maximum and is never coded)"""
    rng = np.random.default_rng(5)
    w = h = 64
    zero = np.zeros((h, w), np.int64)
    lone = zero.copy(); lone[5, 17] = -77
    pm1 = rng.choice([-1, 1], (h, w))
    neg1 = np.full((h, w), -1)
    big = rng.integers((1 << 30) - 4096, 1 << 30, (h, w)) * rng.choice([-1, 1], (h, w))
    big[0, 0] = 2147483647; big[4, 9] = -2147483647
    quiet = rng.integers(-40, 41, (h, w)); quiet[2, 3] = MININT
    jobs, want = _check(oracle, ctxs, [_window(w, h, x) for x in (zero, lone, pm1, neg1, big, quiet)])
    comp = [int(b["comp"]) for b in jobs]
    assert all((len(want[j]) == 0) == (comp[j] == 0) for j in range(len(jobs)))


def test_minint32_fault(oracle, ctxs):
    """MinInt32 in a coded row beside other samples is the reference's panic domain: the fault is reported at the next
    synchronisation by both forms, the block has length 0, the other windows of the plan are coded as ever; alone in its block
    it is an all-zero block (its int32 magnitude is negative) and no fault"""
    rng = np.random.default_rng(6)
    w = h = 64
    bad = rng.integers(-40, 41, (h, w)); bad[8, 30] = MININT
    good = rng.integers(-40, 41, (h, w))
    jobs, want = _check(oracle, ctxs, [_window(w, h, bad), _window(w, h, good)])
    assert [len(want[j]) == 0 for j in range(len(jobs))] == [int(b["comp"]) == 0 for b in jobs]
    alone = np.zeros((h, w), np.int64); alone[8, 30] = MININT
    jobs, want = _check(oracle, ctxs, [_window(w, h, alone), _window(w, h, good)])
    assert [len(want[j]) == 0 for j in range(len(jobs))] == [int(b["comp"]) == 0 for b in jobs]


def test_emit_seams(oracle, ctxs):
    """blocks found by a search with the oracle on the CPU (tests/golden/ht_encode_wg_seams.npz): a 0xFF byte at MagSgn byte 255,
    256, 257, 1023 and 1024 -- the seams of the 256-byte steps the four waves share and of a round of four steps -- and a VLC byte
    stuffed to 7 bits (0x7F behind a byte above 0x8F) at VLC byte 255 and 256.  The property is checked in the oracle's bytes."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ht_encode_wg_seams.npz"))
    names = ["ms255", "ms256", "ms257", "ms1023", "ms1024", "vlc255", "vlc256"]
    w = h = 64
    mel = 2 * w * h // 4
    for nm in names:
        by = oracle.ht_encode(g[nm].astype(np.int32), w, h)
        scup = int(by[-2]) << 8 | int(by[-1])
        ms, vlc = by[:by.size - scup], by[by.size - scup + mel:by.size - 2]
        k = int(nm.lstrip("msvlc"))
        if nm.startswith("ms"):
            assert ms.size > k + 1 and ms[k] == 0xFF, nm
        else:
            assert vlc.size > k + 1 and vlc[k] == 0x7F and vlc[k - 1] > 0x8F, nm
    _check(oracle, ctxs, [_window(w, h, g[nm]) for nm in names])


@pytest.mark.parametrize("W,H,Cn,nres,cb", [(26, 18, 2, 2, 64), (121, 123, 1, 2, 64), (256, 128, 1, 2, 128), (200, 150, 3, 4, 32)])
def test_blocks_off_the_four_wave_path(oracle, ctxs, W, H, Cn, nres, cb):
    """the same launch codes what the four waves do not share, on wave 0 alone: widths that are no multiple of 4 (13 x 9), windows
    on odd strides (61 / 60 wide in a plane of 121), more than 1024 coded samples (128 x 64: the bit-serial path) -- and a small
    frame of several resolutions that mixes all of them with four-wave blocks"""
    rng = np.random.default_rng(W + H)
    planes = []
    for c in range(Cn):
        p = rng.integers(-200, 201, (H, W)); p[rng.random((H, W)) < 0.4] = 0
        planes.append(p)
    _check(oracle, ctxs, planes, nres, cb)


def test_alias_list_longer_than_64(oracle, ctxs):
    """An alias list grows past 64 jobs only where the band sizes of successive resolutions stop shrinking, at 1 x 1: an 8 x 8 plane
    with 28 resolutions has a 1 x 1 window shared by 76 jobs (no small geometry gives a window whose width is a multiple of 4 --
    the four-wave path -- more than the four jobs of one resolution: widths halve from one resolution to the next).  The workgroup
    kernel publishes that list from wave 0; the 4 x 4 windows of the same plan take the four-wave path."""
    planes = [np.random.default_rng(9).integers(-90, 91, (8, 8))]
    planes[0][0, 0] = -23
    jobs, want = _check(oracle, ctxs, planes, nres=28)
    ones = [j for j in range(len(jobs)) if (int(jobs[j]["w"]), int(jobs[j]["h"])) == (1, 1)]
    assert len(ones) > 64 and all(len(want[j]) > 0 for j in ones)
