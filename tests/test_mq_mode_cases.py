"""CPU: tests/mq_mode_cases.py is what it says it is, by the oracle alone -- every plan's block count lies in its bracket, the restated
selection rule gives what the table in that module says for both settings, the contents have blocks without a plane and a spread of
bit-plane counts, and the deep blocks exist where claimed.  The device is held to this module by tests/test_gpu_mq_modes.py."""
import numpy as np
import pytest

import mq_mode_cases as mc


@pytest.mark.parametrize("name", sorted(mc.PLANS))
def test_block_counts_lie_in_their_brackets(oracle, name):
    p = mc.PLANS[name]
    jobs = mc.jobs_of(oracle, p)
    lo, hi = p["bracket"]
    assert lo <= len(jobs) <= hi, (name, len(jobs))
    sides = np.array([max(int(b["w"]), int(b["h"])) for _, b in jobs])
    if name.startswith("mid") or name == "small":
        assert sides.max() <= 32
    if name == "small":
        assert len(jobs) < 256
    if name == "big128":
        assert sides.max() == 128 and (sides <= 64).sum() >= 10 and (sides > 64).sum() >= 10 and len(jobs) < 512
    if name == "big256":
        assert sides.max() == 256 and (sides <= 64).sum() >= 4 and ((sides > 128).sum() >= 2) and len(jobs) < 512
    if name == "bigmid":
        assert len(jobs) >= 512 and 0 < (sides > 64).sum() < len(jobs) // 4 and sides.max() <= 256
    if name == "mid_batch":
        assert len(jobs) == 2 * len(mc.jobs_of(oracle, mc.PLANS["mid"]))
    if name == "mid_tiled":
        tiles = mc.tiles_of(p)
        assert len(tiles) == 9 and len({(w, h) for *_, w, h in tiles}) == 4            # ragged: four tile shapes
    # the windows partition every tile-component
    for i, (_, _, _, _, w, h) in enumerate(mc.tiles_of(p)):
        for comp in range(p["C"]):
            cover = np.zeros((h, w), np.int32)
            for t, b in jobs:
                if t == i and int(b["comp"]) == comp:
                    cover[int(b["y0"]):int(b["y0"]) + int(b["h"]), int(b["x0"]):int(b["x0"]) + int(b["w"])] += 1
            assert (cover == 1).all(), (name, i, comp)


def test_restated_rule_is_the_table(oracle):
    n = {name: len(mc.jobs_of(oracle, mc.PLANS[name])) for name in mc.PLANS}
    # K: 1 alone for every plan here, ceil(n / 256) in company
    for name in mc.PLANS:
        assert mc.enc_k(n[name], False) == 1
    assert mc.enc_k(n["small"], True) == 1
    for name in ("mid", "mid_tiled", "mid_576", "mid_cb8", "bigmid"):
        assert 3 <= mc.enc_k(n[name], True) <= 5 and mc.enc_k(n[name], True) == -(-n[name] // 256)
    assert mc.enc_k(n["mid_batch"], True) == -(-n["mid_batch"] // 256) > mc.enc_k(n["mid"], True)
    assert [mc.enc_k(k, True) for k in (1, 256, 257, 512, 513, 64 * 256, 64 * 256 + 1, 10 ** 6)] == [1, 1, 2, 2, 3, 64, 64, 64]
    assert [mc.enc_k(k, False) for k in (1, 2048, 2049, 4096, 4097, 10 ** 6)] == [1, 1, 2, 2, 3, 64]
    # the split: in company only, from 512 blocks
    for name in mc.PLANS:
        assert not mc.dec_split(n[name], False)
        assert mc.dec_split(n[name], True) == (name in ("mid", "mid_tiled", "mid_576", "mid_cb8", "mid_batch", "bigmid"))
    assert [mc.dec_split(k, True) for k in (511, 512)] == [False, True] and [mc.dec_split(k, False) for k in (11999, 12000)] == [False, True]
    assert not mc.in_company(0) and not mc.in_company(1) and mc.in_company(2) and mc.in_company(3)
    # the whole record, both settings
    assert mc.forms(807, 16, 1) == [1, 1, 0, 0, 0, 0, 0, 0]
    assert mc.forms(807, 16, 2) == [2, 4, 0, 1, 2, 0, 0, 0]
    assert mc.forms(807, 16, 3, aligned=False) == [3, 4, 0, 0, 0, 0, 1, 0]
    assert mc.forms(100, 128, 1) == [1, 1, 0, 0, 0, 1, 0, 0]
    assert mc.forms(100, 128, 2) == [2, 1, 1, 0, 0, 2, 0, 0]
    assert mc.forms(780, 72, 1) == [1, 1, 0, 0, 0, 1, 0, 0]
    assert mc.forms(780, 72, 2) == [2, 4, 1, 1, 2, 2, 0, 0]
    assert mc.forms(780, 72, 2, host_call=True) == [2, 0, 0, 1, 2, 1, 0, 0]
    assert mc.forms(807, 16, 2, decoded=False) == [2, 4, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("name", sorted(mc.PLANS))
def test_contents_are_what_they_claim(oracle, name):
    c = mc.case(name)
    assert c["n"] == len(c["jobs"]) == c["lens"].size == c["numbps"].size and int(c["lens"].sum()) == c["bytes"].size
    coded = c["lens"] > 0
    j = np.arange(c["n"])
    flat = np.isin(j % 8, (0, 3))
    assert np.array_equal(~coded, flat) and (c["numbps"][flat] == 0).all() and flat.sum() >= c["n"] // 5      # blocks without a plane
    nb = c["numbps"][coded]
    assert int(nb.max()) - int(nb.min()) >= 8, (int(nb.min()), int(nb.max()))           # a spread of bit-plane counts
    assert int(nb.max()) <= 31
    noise = coded & (j % 8 != 5)
    assert np.array_equal(c["numbps"][noise], (1 + (5 * j) % 13)[noise])
    big = np.array([max(int(b["w"]), int(b["h"])) > 64 for _, b in c["jobs"]])
    if big.any():                                                                       # ... among the big blocks and among the small ones
        assert (big & flat).any() and (~big & flat).any() and (~big & noise).any()
        assert int(c["numbps"][big & coded].max()) - int(c["numbps"][big & coded].min()) >= 8
    # the sparse blocks: one sample in fifty set (in a window of 16 x 16 that is 5 +- 2: at most 6 % + 8 samples here)
    sparse = 0
    for k, (t, b) in enumerate(c["jobs"]):
        if k % 8 == 5:
            _, _, x0, y0, _, _ = c["tiles"][t]
            win = c["coeff"][int(b["comp"]), y0 + int(b["y0"]):y0 + int(b["y0"]) + int(b["h"]), x0 + int(b["x0"]):x0 + int(b["x0"]) + int(b["w"])]
            assert 0 < np.count_nonzero(win) <= 0.06 * win.size + 8 and c["numbps"][k] == 20
            sparse += 1
    assert sparse >= c["n"] // 9
    # the deep blocks exist where claimed: 32 planes and more after the raise, blocks the plane-stepped decoder could otherwise take
    deep = mc.deep_jobs(c)
    streams = mc.decode_streams(oracle, c)
    assert [s[0] for s in streams] == ["encoded", "arbitrary"]
    _, by, offs, lens, nbv, want = streams[0]
    if c["plan"]["bracket"][0] >= 512:
        assert deep.size >= 2
    for j in deep:
        b = c["jobs"][j][1]
        assert nbv[j] >= 32 and nbv[j] == c["numbps"][j] + 16 and max(int(b["w"]), int(b["h"])) <= 64 and lens[j] > 0
    assert (np.delete(nbv, deep) == np.delete(c["numbps"], deep)).all()
    # the encoder's stream decodes to the coefficients (the deep blocks: shifted up by the 16 planes they claim)
    for j, (t, b) in enumerate(c["jobs"]):
        _, _, x0, y0, _, _ = c["tiles"][t]
        win = c["coeff"][int(b["comp"]), y0 + int(b["y0"]):y0 + int(b["y0"]) + int(b["h"]), x0 + int(b["x0"]):x0 + int(b["x0"]) + int(b["w"])]
        if j not in set(deep.tolist()):
            assert np.array_equal(want[j], win), (name, j)
    # the arbitrary streams: jobs without a byte, 0xFF-rich jobs, 33 planes
    _, by2, offs2, lens2, nb2, _ = streams[1]
    assert (lens2 == 0).sum() >= c["n"] // 5 and (nb2 == 33).sum() >= (1 if c["n"] > 100 and c["max_dim"] <= 64 else 0)
    ff = [j for j in range(c["n"]) if lens2[j] >= 30 and (by2[int(offs2[j]):int(offs2[j]) + int(lens2[j])] == 0xFF).mean() > 0.2]
    assert len(ff) >= 1
    assert int(offs2[-1]) == by2.size and int(offs[-1]) == by.size
