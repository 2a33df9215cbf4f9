"""CPU: the leader / follower rule of tests/ht_dedup_cases.py on the geometries tests/test_gpu_ht_dedup.py decodes -- each has what those tests need."""
import pytest

import ht_dedup_cases as dc


@pytest.mark.parametrize("name", sorted(dc.GEOMETRIES))
def test_every_geometry_has_a_long_list_a_lone_job_and_a_refused_candidate(name):
    g = dc.GEOMETRIES[name]
    blocks = dc.block_list(g["W"], g["H"], g["nres"], g["cb"])
    rule = dc.leaders(blocks)
    n = len(blocks)
    print(name, n, "jobs;", {k: len(v) for k, v in rule.followers.items()}, "refused:", sorted(set(rule.refused.values())))
    assert g["W"] * g["H"] <= 20000
    assert max(len(v) for v in rule.followers.values()) >= 3
    lone = [j for j in range(n) if rule.leaders[j] == j and j not in rule.followers]
    assert lone
    assert any(why in ("width", "alignment") for why in rule.refused.values())
    # the table's invariants: a leader is its own leader and lower than its followers, nobody follows a follower, lists within the cap
    for L, fs in rule.followers.items():
        assert rule.leaders[L] == L and all(f > L and rule.leaders[f] == L for f in fs) and len(fs) <= dc.MAX_FOLLOWERS
        for f in fs:
            assert (blocks[f]["w"], blocks[f]["h"]) == (blocks[L]["w"], blocks[L]["h"]) and blocks[f]["w"] in dc.LEAN_WIDTHS
    assert all(rule.leaders[rule.leaders[j]] == rule.leaders[j] for j in range(n))
    assert all(f != 0 for fs in rule.followers.values() for f in fs)


def test_the_cap_geometry_fills_a_list_and_leaves_a_job_beyond_it():
    g = dc.GEOMETRIES["136x136_cb16"]
    rule = dc.leaders(dc.block_list(g["W"], g["H"], g["nres"], g["cb"]))
    assert len(rule.followers[min(rule.followers)]) == dc.MAX_FOLLOWERS or max(len(v) for v in rule.followers.values()) == dc.MAX_FOLLOWERS
    beyond = [j for j, why in rule.refused.items() if why == "cap"]
    assert beyond and all(rule.leaders[j] == j for j in beyond)


def test_store_shapes_of_the_lean_path_are_both_present():
    widths = set()
    for g in dc.GEOMETRIES.values():
        blocks = dc.block_list(g["W"], g["H"], g["nres"], g["cb"])
        widths |= {blocks[f]["w"] for fs in dc.leaders(blocks).followers.values() for f in fs}
    assert {16, 32, 64} <= widths
