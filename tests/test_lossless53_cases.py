"""CPU: the case lists of tests/lossless53_cases.py before the GPU sees them (tests/test_gpu_lossless53_oracle.py).

* The constants are the code's: context defaults from csrc/j2k_plan.h, accepted option values from the ctx_options() table.
* The lists are deterministic, the ids unique, and every route the restated plan builder knows -- kernel form x direction x {int32 frame,
  host unit call, each packed format whose pixels that form reads or writes} -- is reached by three cases at least.
* Every seam column and row of every case's job tables carries an impulse of that case's `impulse` content, and the `step` content has an
  edge on it.
* The C oracle and oracle/pyref.py -- two independent restatements of the reference -- agree on preprocess (the `noise` frame, every tile),
  decompose53 and reconstruct53 (`fullrange`, one component) of every case of PYREF_CAP samples and fewer.
* Each `pixelrange` set has two rows at least that leave 0 ... 2^prec - 1 and two that do not, by the oracle alone.

Counts (printed by the tests; -s shows them):
  784 cases (marching planes 134, marching RGB 85, plane workgroup 88, tail and deep 100, RGBA8 level 0 271, packed formats 106) and 190 unit-call
      shapes x 2 level counts reach 122 routes; the thinnest routes have 3 cases (packed-format forms of the plane kernels, the RGBA8 kernels and
      the pixel-writing marching kernel under NRGBA, the mid job without the compact layout), `tail` has 337
  22 974 seam columns and rows carry an impulse; of the marching tables' band seams 6 827 are linked through LDS and 2 280 are not
  pyref confirms 413 of the 784 cases (401 of 16 000 samples and fewer, 12 larger ones -- 16 384 ... 72 360 samples -- for the routes those do
      not reach; 371 left out); every route keeps a confirmed case
  485 `pixelrange` sets (61 cases below 6 rows have none): 3 ... 10 rows leave the range, 2 ... 112 stay inside it"""
import collections

import numpy as np

import lossless53_cases as lc
import pyref

PYREF_CAP = 16000            # samples of a frame (W * H * C): pyref is a scalar walk of about 4 us per sample and call


def test_constants_follow_the_code():
    d = lc.defaults()
    assert d == {"band_prows": 5, "band_prows_pix": 3, "plane_wg": 4, "l0_wg": 8, "l0_wg_invw": 4, "deep_min_planes": 12}, d      # what the shapes below were laid out for
    v = lc.option_values()
    assert {k: v[k] for k in lc.OPTIONS_53} == {
        "plane_wg": (0, 4, 8), "l0_wg": (0, 4, 8), "l0_wg_invw": (0, 4, 8), "l0_fuse": (0, 8, 10, 16), "l0_inv_wpe": (5, 6, 7), "l0_store": (0, 1, 2, 4),
        "deep": (0, 1), "deep_mid": (0, 1), "deep_mid_inv": (0, 1, 2), "mega": (0, 1, 2), "plane_wg3": (0, 1), "pix_fuse": (0, 1, 2), "l0_wg_inv": (0, 1)}
    # every accepted value of every option is some case's context (the defaults through the cases that do not name the option)
    seen = collections.defaultdict(set)
    for c in lc.all_cases():
        for k, val in c.env:
            seen[k[4:].lower()].add(val)
    a = lc.all_defaults()
    for k in lc.OPTIONS_53:
        assert set(v[k]) <= seen[k] | {a[lc.OPTION_FIELD.get(k, k)]}, (k, seen[k])
    ws = lc.march_widths()
    for b in lc.STRIP_BASES:
        assert {b + e for e in lc.STRIP_DELTAS} <= set(ws)
    assert set(range(190, 197)) | set(range(380, 389)) | set(range(1, 10)) <= set(ws)
    assert {w for w, _ in lc.march_shapes()} == set(ws)
    hs = lc.march_heights()
    assert {1, 2, 3} | {2 * b * k + e for b in (5, 3) for k in (1, 2, 4) for e in (-1, 0, 1)} == set(hs)
    for h in hs:
        assert sum(1 for _, hh in lc.march_shapes() if hh == h) >= 3
    for nr in (3, 7):
        halves = collections.defaultdict(set)
        for h in lc.wg_heights(nr):
            halves[(h + 1) // 2].add(h & 1)
        assert set(halves) == {nr - 1, nr, nr + 1, 2 * nr, 2 * nr + 1} and all(p == {0, 1} for p in halves.values())
    for nr2 in (5, 7, 13):
        assert {((h + 1) // 2 + 1) // 2 for h in lc.fuse_heights(nr2)} == {nr2 - 1, nr2, nr2 + 1, 2 * nr2, 2 * nr2 + 1}
        assert {h & 1 for h in lc.fuse_heights(nr2)} == {0, 1}
    for c in lc.all_cases():
        assert c.W * c.H * c.C <= 600000 and all(w <= 1100 and (h <= 64 or w <= 520) or w <= 16 for _, _, w, h in lc.tiles_of(c.W, c.H, c.tile)), c.id


def test_lists_are_deterministic_and_ids_unique():
    ids = [c.id for c in lc.all_cases()]
    assert len(ids) == len(set(ids))
    for f in (lc.marching_plane_cases, lc.marching_rgb_cases, lc.plane_wg_cases, lc.tail_deep_cases, lc.rgba8_cases, lc.packed_cases):
        a = f()
        f.cache_clear()
        assert a == f()
    assert np.array_equal(lc.int_frame("fullrange", 24, 12, 3, 12, 5), lc.int_frame("fullrange", 24, 12, 3, 12, 5))
    assert np.array_equal(lc.coeff_plane("noise", 24, 12, 5), lc.coeff_plane("noise", 24, 12, 5))
    assert np.array_equal(lc.pixelrange_set(24, 12, 3, 8, 3, 1), lc.pixelrange_set(24, 12, 3, 8, 3, 1))


def test_restated_routing_on_known_plans():
    """the restatement on geometries whose plan the code's comments and the older tests spell out"""
    R = lc.route(3840, 2160, 3, (512, 512), 6)                                   # the benchmark's 4K frame: 40 tiles, 120 planes
    assert R["deep_l0"] == 1 and R["tail_l0"] == 2 and R["nlaunch"] == 1 and len(R["deep"]) == 120
    assert R["tabs"][(0, 1)].cpl == 8 and R["tabs"][(0, 1)].vec and R["rgba8"]["fwd_wg"]["nw"] == 8 and R["rgba8"]["inv_wg"]["nw"] == 4
    assert lc.pick_cpl(191) == 2 and lc.pick_cpl(192) == 4 and lc.pick_cpl(383) == 4 and lc.pick_cpl(384) == 8
    assert [j[1] for j in lc.make_jobs(0, 1016, 1, 8, 5)] == [0, 504, 1000] and [j[1] for j in lc.make_jobs(0, 512, 1, 8, 5)] == [0]
    assert [j[1] for j in lc.make_jobs(0, 513, 1, 8, 5)] == [0, 504] and [j[1] for j in lc.make_jobs(0, 129, 1, 2, 5)] == [0, 126]
    R = lc.route(518, 21, 1, (512, 0), 2, (("J2K_PLANE_WG", 0),))                # a ragged column of 6: the whole table falls to cpl 2 scalar
    assert (R["tabs"][(0, 0)].cpl, R["tabs"][(0, 0)].vec) == (2, False)
    R = lc.route(260, 40, 3, (0, 0), 6, (("J2K_DEEP_MIN_PLANES", 1),))           # level 1 is 130 wide: not a multiple of 4, the tail takes over
    assert R["deep_l0"] == -1 and R["tail_l0"] == 2
    R = lc.route(264, 40, 3, (0, 0), 6, (("J2K_DEEP_MIN_PLANES", 1),))
    assert R["deep_l0"] == 1 and not R["deep"][0]["has_mid"]
    R = lc.route(512, 66, 3, (0, 0), 6, (("J2K_DEEP_MIN_PLANES", 1),))
    assert R["deep_l0"] == 1 and R["deep"][0]["has_mid"] and R["deep"][0]["compact"]
    R = lc.route(16, 8194, 1, (0, 0), 3)
    assert R["tabs"][(0, 0)].pwg is None and lc.route(16, 8192, 1, (0, 0), 3)["tabs"][(0, 0)].pwg is not None      # 4096 pair-rows
    linked, unlinked = lc.seam_kinds(lc.route(128, 41, 1, (0, 0), 2, (("J2K_PLANE_WG", 0),)))
    assert linked == 3 and unlinked == 1                                         # five bands of five pair-rows: the fifth starts a workgroup


def test_every_route_has_three_cases():
    """Counts per route (kernel form, direction, int32 frame / unit call / packed format), printed with -s."""
    R = lc.all_routes()
    lines = ["%4d  %-36s %s %s" % (len(v), k[0], k[1], k[2]) for k, v in sorted(R.items())]
    print("\n".join(lines))
    print("routes %d, cases %d (+ %d unit shapes x %d level counts), thinnest route %d cases"
          % (len(R), len(lc.all_cases()), sum(len(lc.unit_shapes(n)) for n in lc.UNIT_WAVES), len(lc.UNIT_LEVELS), min(len(v) for v in R.values())))
    thin = {k: len(v) for k, v in R.items() if len(v) < 3}
    assert not thin, thin
    forms = {k[0] for k in R}
    # every template instantiation the launchers can reach has a route
    for want in ["march<cpl%d,nc%d,vec>" % (c, n) for c in (2, 4, 8) for n in (1, 3)] + ["march<cpl2,nc1,scalar>", "march<cpl2,nc3,scalar>",
                 "march<cpl8,nc1,vec,pix>", "march<cpl8,nc3,vec,pix>", "tail", "deep_fwd<mid>", "deep_fwd<nomid>", "deep_flat", "deep_inv<nomid>",
                 "deep_inv<mid0>", "deep_inv<mid1>", "deep_inv<mid1,compact>", "deep_inv<mid2>", "mega_fwd<order1>", "mega_fwd<order2>",
                 "mega_inv<order1>", "mega_inv<order2>", "rgba8_fuse<nw8,store1>", "rgba8_fuse<nw8,store0>", "rgba8_fuse<nw10,store1>", "rgba8_fuse<nw16,store1>"] + \
                ["plane_wg<nw%d,nc%d,io0,%s>" % (nw, n, m) for nw in (4, 8) for n in (1, 3) for m in ("single", "multi")] + \
                ["plane_wg<nw4,nc1,io%d,%s>" % (s, m) for s in (1, 2, 3, 4) for m in ("single", "multi")] + \
                ["plane_wg<nw4,nc3,io4,%s>" % m for m in ("single", "multi")] + ["plane_wg<nw8,nc1,io1,%s>" % m for m in ("single", "multi")] + \
                ["rgba8_wg_fwd<nw%d,store1>" % nw for nw in (4, 8)] + ["rgba8_wg_fwd<nw8,store%d>" % s for s in (0, 2, 4)] + \
                ["rgba8_wg_inv<nw%d,wpe%d>" % (nw, w) for nw in (4, 8) for w in (5, 6, 7)]:
        assert want in forms, want


def test_every_seam_carries_an_edge():
    """every seam column / row of every case's job tables: an impulse of the `impulse` frame on it, an edge of the `step` frame at it; both
    kinds of band seam (linked through LDS, not linked) occur"""
    nseam = linked = unlinked = 0
    for c in lc.all_cases():
        R = c.route
        seam = lc.seams(R)
        lk, ul = lc.seam_kinds(R)
        linked += lk
        unlinked += ul
        pts = set(lc.impulse_points(c.W, c.H, c.tile, seam))
        big = c.W * c.H > 100000
        if not big:
            imp = lc.int_frame("impulse", c.W, c.H, c.C, c.prec, 1, c.tile, seam)
            assert {tuple(p) for p in np.argwhere((imp != (1 << (c.prec - 1))).any(axis=0))} == pts, c.id
            ecols, erows = lc.step_edges(lc.int_frame("step", c.W, c.H, c.C, c.prec, 1, c.tile, seam))
        for x0, y0, w, h in lc.tiles_of(c.W, c.H, c.tile):
            cols, rows = seam.get((x0, y0), (set(), set()))
            assert (y0 + h - 1 in {y for y, _ in pts}) and (x0 + w - 1 in {x for _, x in pts})            # last row, last column
            for col in cols:
                if col < w:
                    nseam += 1
                    assert any(x == x0 + col and y0 <= y < y0 + h for y, x in pts), (c.id, "column", col)
                    if not big and col + 1 in cols and col + 1 < w:
                        assert x0 + col in ecols, (c.id, "step column", col)
            for row in rows:
                if row < h:
                    nseam += 1
                    assert any(y == y0 + row and x0 <= x < x0 + w for y, x in pts), (c.id, "row", row)
                    if not big and row + 1 in rows and row + 1 < h and c.C > 1:
                        assert y0 + row in erows, (c.id, "step row", row)
    print("seam columns and rows with an impulse: %d; band seams of the marching tables linked through LDS %d, not linked %d" % (nseam, linked, unlinked))
    assert linked >= 100 and unlinked >= 100


def test_oracle_agrees_with_pyref(oracle):
    """oracle.preprocess (every tile of the `noise` frame), decompose53 and reconstruct53 (`fullrange`, component 0 of the first tile) ==
    pyref's on every case of PYREF_CAP samples and fewer and on the smallest case of every route those do not reach; at most half of the
    cases are left out and every route keeps a confirmed case"""
    cases = lc.all_cases()
    done, routes = 0, set()
    small = [c for c in cases if c.W * c.H * c.C <= PYREF_CAP]
    for c in small:
        routes |= c.forms("fwd") | c.forms("inv")
    extra = {}                                   # the smallest case of every route that no case under the cap reaches
    for c in sorted(cases, key=lambda c: c.W * c.H * c.C):
        if (c.forms("fwd") | c.forms("inv")) - routes:
            extra[c.id] = c
            routes |= c.forms("fwd") | c.forms("inv")
    for c in small + list(extra.values()):
        done += 1
        frame = lc.int_frame("noise", c.W, c.H, c.C, c.prec, 1)
        for x0, y0, w, h in lc.tiles_of(c.W, c.H, c.tile):
            crop = frame[:, y0:y0 + h, x0:x0 + w]
            want = lc.expect_forward(oracle, crop, c.prec, c.nres)
            py = pyref.preprocess([crop[k].reshape(-1).tolist() for k in range(c.C)], w, h, c.prec, True, c.nres)
            assert np.array_equal(np.array(py, np.int64).reshape(c.C, h, w), want), (c.id, "preprocess")
        x0, y0, w, h = lc.tiles_of(c.W, c.H, c.tile)[0]
        x = lc.coeff_plane("fullrange", w, h, 1)
        lv = lc.levels_of(c.nres)
        d = x.reshape(-1).tolist()
        pyref.decompose53(d, w, h, lv)
        assert np.array_equal(np.array(d, np.int64).reshape(h, w), oracle.decompose53(x, w, h, lv)), (c.id, "decompose53")
        d = x.reshape(-1).tolist()
        pyref.reconstruct53(d, w, h, lv)
        assert np.array_equal(np.array(d, np.int64).reshape(h, w), oracle.reconstruct53(x, w, h, lv)), (c.id, "reconstruct53")
        assert np.array_equal(oracle.tcd_inverse_dwt(x, w, h, lv, 1), oracle.reconstruct53(x, w, h, lv))
    unit = {r for r in lc.all_routes() if r[2] == "unit"}
    missing = set(lc.all_routes()) - routes - unit
    print("pyref confirms %d of %d cases (%d of %d samples and fewer, %d larger ones for the routes those do not reach: %d ... %d samples; %d left out); "
          "routes without a confirmed case: %s" % (done, len(cases), len(small), PYREF_CAP, len(extra), min(c.W * c.H * c.C for c in extra.values()),
                                                   max(c.W * c.H * c.C for c in extra.values()), len(cases) - done, sorted(missing)))
    assert 2 * done >= len(cases)
    assert not missing


def test_pixelrange_sets_leave_and_keep_the_range(oracle):
    """every `pixelrange` set the GPU tests use: rows that leave 0 ... 2^prec - 1 and rows that do not, two of each at least, by the oracle"""
    out, keep, n = [], [], 0
    for c in lc.rgba8_cases() + lc.packed_cases():
        if not c.pixelrange:
            continue
        for x0, y0, w, h in lc.tiles_of(c.W, c.H, c.tile):
            co = lc.pixelrange_set(w, h, c.C, c.prec, c.nres, x0 + y0)
            bad = lc.out_of_range_rows(lc.expect_inverse(oracle, co, c.prec, c.nres), c.prec)
            assert bad.sum() >= 2 and (~bad).sum() >= 2, (c.id, x0, y0)
            n += 1
            out.append(int(bad.sum()))
            keep.append(int((~bad).sum()))
    small = sum(1 for c in lc.rgba8_cases() + lc.packed_cases() if not c.pixelrange)
    print("pixelrange sets %d (cases below %d rows without one: %d): rows that leave the range %d ... %d, rows that stay inside %d ... %d"
          % (n, lc.PIXELRANGE_MIN_H, small, min(out), max(out), min(keep), max(keep)))
    assert n >= 200
