"""CPU: the case lists of tests/ht_follow_cases.py against the C oracle alone -- no kernel.  A GPU check that passes vacuously would hide a wrong
HT_PAIR_DUP, so: every flip outside the read set leaves HTDecoder.Decode's output unchanged (a follower verified in spite of it is right to be), and
in every position class of the read set at least one case changes the output (a follower verified in spite of THAT would be caught)."""
import numpy as np

import ht_dedup_cases as dc
import ht_follow_cases as fc
import ht_stream_cases as hc


def test_interior_flips_leave_the_oracles_output_unchanged():
    w, h = fc.EDGE_SHAPE
    seen = 0
    for c in fc.edge_cases():
        if c.cls not in fc.INTERIOR_CLASSES:
            continue
        a_end, b_start = fc.read_set(c.base, w, h)
        diff = [i for i in range(len(c.base)) if c.base[i] != c.other[i]]
        assert len(c.base) == len(c.other) and len(diff) == 1 and a_end <= diff[0] < b_start, c.label
        assert np.array_equal(fc.decode(c.base, w, h), fc.decode(c.other, w, h)), c.label
        seen += 1
    assert seen >= 14                                                 # first and last interior byte of the encoder's block, the one-byte interior, the refused blocks'; x 2 roles


def test_every_read_set_class_has_a_case_that_changes_the_output():
    """... in a block that HAS an interior: where A reaches B the kernel compares the whole block, as the parent did, and such a case says nothing about
    where the narrower compare ends.  The one exception is b_first: B's first byte is what 46 bits for every pair would reach, no stream on 8 pairs
    gets there with an interior in front of it (the encoder's block: B starts at byte 176, the deepest byte used is 224), so that class is pinned from the inside
    by vlc_deepest -- the deepest VLC byte that changes the output, in a block with an interior -- and itself only where B starts the suffix."""
    w, h = fc.EDGE_SHAPE
    changes = {cls: 0 for cls in fc.POSITION_CLASSES}
    with_interior = {cls: 0 for cls in fc.POSITION_CLASSES}
    for c in fc.edge_cases():
        if c.cls in changes and c.who == "follower":
            diff = [i for i in range(len(c.base)) if c.base[i] != c.other[i]]
            a_end, b_start = fc.read_set(c.base, w, h)
            assert len(diff) == 1 and (diff[0] < a_end or diff[0] >= b_start), c.label      # inside the read set
            if not np.array_equal(fc.decode(c.base, w, h), fc.decode(c.other, w, h)):
                changes[c.cls] += 1
                with_interior[c.cls] += a_end < b_start
    assert all(changes.values()), changes
    assert all(n for cls, n in with_interior.items() if cls != "b_first"), with_interior
    assert with_interior["mel0"] >= 2 and with_interior["mel1"] >= 2 and with_interior["mel2"] >= 2 and with_interior["mel3"] >= 2   # behind 0 and 4 MagSgn bytes


def test_the_big_block_reads_its_magsgn_segment_past_the_first_kilobyte():
    """the 64 x 64 cases: every flip below byte 1 493 of the segment -- the last byte of the first 1 KB batch, the first of the second, inside it, the
    last byte read, the last byte of a segment cut to 1 023 / 1 024 / 1 025 / 1 300 bytes -- changes the oracle's output, in a block with an interior;
    the flips behind it and in the interior change nothing"""
    w, h = fc.BIG_SHAPE
    changes = {cls: 0 for cls in fc.BIG_CLASSES}
    cut = set()
    for c in fc.big_edge_cases():
        if c.who != "follower":
            continue
        diff = [i for i in range(len(c.base)) if c.base[i] != c.other[i]]
        a_end, b_start = fc.read_set(c.base, w, h)
        assert len(diff) == 1 and a_end < b_start, c.label
        same = np.array_equal(fc.decode(c.base, w, h), fc.decode(c.other, w, h))
        if c.cls in changes:
            assert not same and diff[0] < a_end, c.label
            changes[c.cls] += 1
            if c.cls == "cut_last":
                cut.add(diff[0] + 1)
        else:
            assert same, c.label
            assert diff[0] >= fc.BIG_READS
    assert all(changes.values()), changes
    assert cut == {1023, 1024, 1025, 1300}
    assert any(c.cls == "" and c.who == "follower" and 2048 <= [i for i in range(len(c.base)) if c.base[i] != c.other[i]][0] < 2500 for c in fc.big_edge_cases())


def test_the_mel_start_cases_are_refusals_that_one_flip_lifts():
    w, h = fc.EDGE_SHAPE
    n = 0
    for c in fc.edge_cases():
        if c.cls.startswith("mel") and c.who == "follower":
            assert hc.classify(c.base, w, h).reject == "mel" and hc.classify(c.other, w, h).reject == "none", c.label
            assert (len(c.base) - hc.scup_of(c.base)) % 4 == 0     # an empty or four-byte MagSgn segment: the MEL reader looks at four bytes
            n += 1
    assert n == 12                                                   # the whole-block recipe, and with an interior behind 0 and 4 MagSgn bytes


def test_the_lengths_and_forms_the_cases_cover():
    w, h = fc.EDGE_SHAPE
    cases = fc.edge_cases()
    assert {len(c.base) for c in cases} >= set(range(4, 9))
    seg = {len(c.base) - hc.scup_of(c.base) for c in cases}
    assert seg >= {0, 1, 3, 1023, 1024, 1025} and max(seg) > 2048
    gaps = set()
    for c in cases:
        n, scup = len(c.base), hc.scup_of(c.base)
        gaps.add((n - 2 - fc.vlc_reach(scup, w, h)) - (n - scup + 4))
    assert gaps >= {0, -1, 1}                                       # A and B touch, overlap by one byte, leave one byte between them
    assert all(c.who == "none" or len(c.other) == len(c.base) for c in cases)
    for c in cases:                                                  # every body is a block the prep would take: not refused before the compare (or refused alike)
        assert len(c.base) >= 4


def test_the_walk_plans_have_the_counts_they_are_named_for():
    for count, g in fc.WALK_PLANS.items():
        blocks, rule = fc.plan_rule(g)
        order, nlead = fc.walk_order(rule.leaders)
        assert nlead == count == sum(1 for j, L in enumerate(rule.leaders) if L == j), g
        assert sorted(order) == list(range(len(blocks))) and order[:nlead] == sorted(order[:nlead]) and order[nlead:] == sorted(order[nlead:])
        assert all(rule.leaders[j] == j for j in order[:nlead]) and all(rule.leaders[j] != j for j in order[nlead:])
        assert max(b["w"] for b in blocks) * max(b["h"] for b in blocks) <= 64 * 64 and g["W"] * g["H"] <= 140 * 140
    groups = {k: fc.follower_only_groups(*fc.walk_order(fc.plan_rule(g)[1].leaders)) for k, g in fc.WALK_PLANS.items()}
    assert groups[1] == [] and [g for g, _ in groups[64]] == [1, 2, 3] and [g for g, _ in groups[65]] == [2] and [g for g, _ in groups[129]] == [3]
    assert [g for g, _ in groups[63]] == [1, 2] and len(groups[63][1][1]) == 5       # a full follower-only workgroup and a partial last one
    assert len(groups[65][0][1]) < fc.WALK_BLOCKS                                     # (partial as well)


def test_big_u_suffixes_exist_for_every_lean_width():
    for w, h in ((8, 8), (16, 16), (32, 32), (64, 16)):
        sufs = fc.big_u_suffixes(w, h)
        assert hc.classify(sufs["=32"], w, h).max_u == 32 and hc.classify(sufs[">=33"], w, h).max_u >= 33
        assert all(len(s) >= 4 for s in sufs.values())
