"""The yardstick of rate control on batch plans (j2k_plan_set_rate_per_frame, FramePlan(rate_per_frame=True), the *_frames calls), importable
without a GPU: tests/test_frame_rate_cases.py checks it on the CPU, tests/test_gpu_frame_rate.py holds the device against it bit for bit.

A batch plan (frame_rows) holds F = height / frame_rows frames; every frame is coded exactly as it would be alone.  Rate control on it has one
meaning: FRAME f GETS THE CUTS IT WOULD GET ALONE UNDER ITS OWN BUDGET.  With tpf = tiles / F tiles per frame, frame f owns the contiguous job
range J_f = the blocks whose tile is in [f tpf, (f + 1) tpf) -- the plan lists its blocks tile by tile -- and every function below is the
existing definition (rate_cases.allocate, layer_cases.allocate_layers, quality_cases.allocate_quality / allocate_quality_layers,
pass_cases.allocate_quality) called on the tables, point counts and weights of J_f with frame f's budget(s) or target(s).  Nothing else is
new: the order of the float64 sum of quality_cases starts again at the first block of every frame.

Layouts: kept [L][n] as before; chosen and achieved [L][F].  A scalar budget / target (or a ladder of L of them) applies to every frame
separately; the *_frames forms of the device take one value per frame (one layer) -- here: `per_frame=True`, budgets[f] / targets[f]."""
import numpy as np

import layer_cases as lc
import pass_cases as pc
import quality_cases as qc
import rate_cases as rc


# ---- ranges -----------------------------------------------------------------------------------------------------------------------------------
def frame_ranges(block_tiles, tiles_per_frame, nframes=None):
    """the tile of every block (job order), tiles per frame -> [(first job, job count)] per frame.  Frames are contiguous (asserted); a frame
    whose tiles have no blocks has count 0 and starts where the next one does.  nframes: the plan's frame count (default: as many as the last
    block's tile needs)"""
    bt = [int(t) for t in block_tiles]
    tpf = int(tiles_per_frame)
    assert tpf >= 1 and all(a <= b for a, b in zip(bt, bt[1:])), "blocks are listed tile by tile"
    ntiles = (max(bt) + 1) if bt else tpf
    F = int(nframes) if nframes is not None else (ntiles + tpf - 1) // tpf
    assert F * tpf >= ntiles
    out = []
    j = 0
    for f in range(F):
        first = j
        while j < len(bt) and bt[j] // tpf == f:
            j += 1
        out.append((first, j - first))
    assert j == len(bt)
    return out


def _slices(ranges, *tabs):
    for a, c in ranges:
        yield tuple(t[a:a + c] for t in tabs)


def _per_frame(values, F, per_frame):
    """what frame f is given: values[f] alone (per_frame) or the whole ladder"""
    if per_frame:
        assert len(values) == F, "one value per frame"
        return [[v] for v in values]
    return [list(values)] * F


# ---- byte budgets -----------------------------------------------------------------------------------------------------------------------------
def allocate_layers_frames(Rs, Ds, nbs, ws, ranges, budgets, per_frame=False):
    """-> (kept [L][n], chosen [L][F]); L = 1 with per_frame.  nbs: the point count of every block (numBPS on plane tables, pass_cases.points
    on pass tables)"""
    F = len(ranges)
    mine = _per_frame(budgets, F, per_frame)
    L = len(mine[0]) if F else len(budgets)
    n = len(Rs)
    kept = [[0] * n for _ in range(L)]
    chosen = [[0] * F for _ in range(L)]
    for f, ((a, c), (R, D, nb, w)) in enumerate(zip(ranges, _slices(ranges, Rs, Ds, nbs, ws))):
        k, ch = lc.allocate_layers(R, D, nb, w, mine[f])
        for l in range(L):
            kept[l][a:a + c] = k[l]
            chosen[l][f] = ch[l]
    return kept, chosen


def allocate_frames(Rs, Ds, nbs, ws, ranges, budget):
    """one budget for every frame (an int) or one per frame (a sequence) -> (kept [n], chosen [F]): rate_cases.allocate per range"""
    per = not isinstance(budget, (int, np.integer))
    kept, chosen = allocate_layers_frames(Rs, Ds, nbs, ws, ranges, list(budget) if per else [int(budget)], per_frame=per)
    return kept[0], chosen[0]


# ---- distortion targets -----------------------------------------------------------------------------------------------------------------------
def allocate_quality_layers_frames(Rs, Ds, nbs, ws, ranges, targets, per_frame=False, passes=False):
    """-> (kept [L][n], chosen [L][F], achieved [L][F]); passes: the tables are pass tables (pass_cases.allocate_quality: the wider hull arrays)"""
    F = len(ranges)
    mine = _per_frame(targets, F, per_frame)
    L = len(mine[0]) if F else len(targets)
    n = len(Rs)
    kept = [[0] * n for _ in range(L)]
    chosen = [[0] * F for _ in range(L)]
    achieved = [[0.0] * F for _ in range(L)]
    for f, ((a, c), (R, D, nb, w)) in enumerate(zip(ranges, _slices(ranges, Rs, Ds, nbs, ws))):
        if passes:
            assert L == 1, "pass cuts take one target"
            ps, b, s = pc.allocate_quality(R, D, nb, w, mine[f][0])
            k, ch, ac = [ps], [b], [s]
        else:
            k, ch, ac = qc.allocate_quality_layers(R, D, nb, w, mine[f])
        for l in range(L):
            kept[l][a:a + c] = k[l]
            chosen[l][f] = ch[l]
            achieved[l][f] = ac[l]
    return kept, chosen, achieved


def allocate_quality_frames(Rs, Ds, nbs, ws, ranges, target, passes=False):
    """one target for every frame (a float) or one per frame (a sequence) -> (kept [n], chosen [F], achieved [F])"""
    per = not isinstance(target, (int, float, np.integer, np.floating))
    kept, chosen, achieved = allocate_quality_layers_frames(Rs, Ds, nbs, ws, ranges, list(target) if per else [float(target)], per_frame=per, passes=passes)
    return kept[0], chosen[0], achieved[0]


# ---- pass tables ------------------------------------------------------------------------------------------------------------------------------
def allocate_frames_passes(Rs, Ds, nbs, ws, ranges, budget):
    """allocate_frames on the 96-entry tables: the point count of a block is pass_cases.points(numBPS)"""
    return allocate_frames(Rs, Ds, [pc.points(nb) for nb in nbs], ws, ranges, budget)


def allocate_quality_frames_passes(Rs, Ds, nbs, ws, ranges, target):
    return allocate_quality_frames(Rs, Ds, [pc.points(nb) for nb in nbs], ws, ranges, target, passes=True)


def psnr_distortion(W, frame_rows, ncomp, precision, lossless, quality, db):
    """the target of ONE frame of the batch"""
    return qc.psnr_distortion(W, frame_rows, ncomp, precision, lossless, quality, db)


# ---- geometries and frames of the device tests ------------------------------------------------------------------------------------------------
INF = 1 << 62
# name: (W, frame rows, frames, components, resolutions, code-block side, tile)
GEOMETRIES = {
    "thin": (130, 70, 3, 3, 4, 64, (0, 0)),
    "tiled": (260, 44, 2, 3, 4, 64, (128, 32)),
    "strided": (200, 150, 2, 3, 3, 8, (0, 0)),
}
# frame f of a batch: (seed offset, noise as a fraction of the range; 0 = flat, one colour).  They differ so that the frames' lambdas differ: a
# kernel that searched once and applied frame 0's lambda everywhere passes on equal frames.
FRAME_NOISE = ((0, 1.0 / 16), (1, 0.0), (2, 1.0 / 2))
# the frame-range program's geometries (tests/frame_ranges_main.cpp prints them in this order): W, H, frame_rows, ncomp, resolutions, cb, tile
RANGE_GEOMETRIES = (
    ("untiled_batch3", 130, 210, 70, 3, 4, 64, (0, 0)),
    ("tiled_batch2_partial_rows", 260, 88, 44, 3, 4, 64, (128, 32)),
    ("single_frame", 130, 70, 0, 3, 4, 64, (0, 0)),
    ("one_sample_high", 40, 3, 1, 1, 3, 8, (0, 0)),
)


def tiles_of_geometry(W, H, frame_rows, tile):
    """(tiles in all, tiles per frame) of a batch as the plan lays it out: the tile grid starts again at every frame"""
    fh = frame_rows if frame_rows > 0 else H
    tw, th = (tile[0] or W), (tile[1] or fh)
    tpf = ((W + tw - 1) // tw) * ((fh + th - 1) // th)
    return tpf * (H // fh), tpf


def expected_block_tiles(orc, W, H, frame_rows, ncomp, nres, cb, tile):
    """the tile of every block of the batch plan, from the oracle's enumeration of every tile (closed-loop windows)"""
    fh = frame_rows if frame_rows > 0 else H
    tw, th = (tile[0] or W), (tile[1] or fh)
    out, t = [], 0
    for _f in range(H // fh):
        for y0 in range(0, fh, th):
            for x0 in range(0, W, tw):
                w, h = min(tw, W - x0), min(th, fh - y0)
                out += [t] * len(orc.enumerate_blocks(ncomp, w, h, nres, cb, cb, 1))
                t += 1
    return out
