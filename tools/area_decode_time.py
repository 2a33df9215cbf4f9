"""What a region decode buys on the device (docs/KERNEL_NOTES.md 4y): 3840x2160 RGB8, 5-3, Mallat closed loop, MQ coder, 64x64 blocks, SOP + EPH,
untiled and with 512x512 tiles.  decode_frame_pixels with no `area`, and with windows of 512^2, 1024^2 and 2048^2 at the frame's centre, at
reduce 0 and 1, in two modes:

  alone      one context, one frame at a time: HIP events around the call, mean / min of REP frames after WARM, ms (latency)
  in flight  CONTEXTS contexts, each decoding its own stream, every call queued before any is waited for -- the way bench_host.py's closed-loop
             record runs: wall time over a run of at least half a second -> calls per second

Per row also the blocks needed / total (area_blocks) and the time of the area_blocks launch alone (events around FramePlan.area_blocks).  The only
assertions: reduce 0 without `area` gives back the source, and every window equals the crop of the call without `area`.

A package without the area calls is measured through the calls it has (the no-area rows only), so the same script gives the baseline of an older
checkout: --pkg DIR names the directory that holds that checkout's j2kgfx package and libj2kgfx.so.
      python tools/area_decode_time.py [--pkg DIR] [--tiles 0|512] [--contexts 12] [--short] [--json FILE]"""
import json
import os
import sys
import time

import numpy as np
import torch


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


sys.path.insert(0, _arg("--pkg", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-jpeg2000_amd")))
from j2kgfx import _lib                    # noqa: E402
from j2kgfx.codec import FramePlan         # noqa: E402
from j2kgfx.context import Context         # noqa: E402

SHORT = "--short" in sys.argv
WARM, REP = (1, 2) if SHORT else (2, 10)
CONTEXTS = int(_arg("--contexts", "12"))
TILES = [int(_arg("--tiles", "-1"))] if "--tiles" in sys.argv else [512, 0]
W, H = 3840, 2160


def frame(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.clip(np.stack([xx * 255 // W, yy * 255 // H, (xx + yy) * 127 // W]) + rng.integers(-16, 17, (3, H, W)), 0, 255).astype(np.uint8)
    pix = np.full((H, W, 4), 255, np.uint8)
    pix[..., :3] = f.transpose(1, 2, 0)
    return pix.reshape(H, W * 4)


def centre(side):
    x0, y0 = (W - side) // 2, max((H - side) // 2, 0)
    return (x0, y0, x0 + side, min(y0 + side, H))


def lane(tile, seed):
    ctx = Context(0)
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=6, cb=(64, 64), tile=(tile, tile), coder=0, ctx=ctx, mallat=True, track_streams=False)
    pix = frame(seed)
    d_pix = torch.from_numpy(pix).to(plan.device)
    nt = int(plan.info.tiles)
    cs = plan.empty(plan.frame_bound(), torch.uint8)
    toffs = plan.empty(nt + 1, torch.int64)[:nt + 1]
    plan.encode_frame_pixels(_lib.PIX_RGBA8, d_pix, True, True, cs, toffs)
    plan.frame_status()
    return dict(ctx=ctx, plan=plan, pix=pix, cs=cs, toffs=toffs, total=int(toffs[-1].item()), ext=torch.cuda.ExternalStream(ctx.stream), bufs={})


def call(ln, r, area):
    plan = ln["plan"]
    key = (r, area)
    if key not in ln["bufs"]:
        h, w = plan.area_shape(area, r) if area else (plan.reduced_shape(r) if r else (H, W))
        ln["bufs"][key] = torch.zeros((h, w * 4), dtype=torch.uint8, device=plan.device)
    kw = dict(area=area) if area else {}
    plan.decode_frame_pixels(ln["cs"], ln["total"], ln["bufs"][key], ln["toffs"], True, True, reduce=r, **kw)
    return ln["bufs"][key]


def timed(ln, f):
    ms = []
    for i in range(WARM + REP):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ln["ext"]); f(); e1.record(ln["ext"])
        ln["ctx"].sync()
        if i >= WARM:
            ms.append(e0.elapsed_time(e1))
    return float(np.mean(ms)), float(np.min(ms))


def in_flight(lanes, r, area):
    def sweep():
        for ln in lanes:
            call(ln, r, area)

    def barrier():
        for ln in lanes:
            ln["ctx"].sync()
    sweep(); barrier()
    t0 = time.perf_counter()
    sweep(); barrier()
    steps = 2 if SHORT else max(3, int(np.ceil(0.5 / max(time.perf_counter() - t0, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(steps):
        sweep()
    barrier()
    return steps * len(lanes) / (time.perf_counter() - t0)


out = {}
for tile in TILES:
    lanes = [lane(tile, 1 + f) for f in range(CONTEXTS)]          # (made first: with two or more MQ contexts the decoders take their throughput settings in both modes)
    first = lanes[0]
    have = hasattr(first["ctx"].L, "j2k_plan_decode_frame_pixels_area")
    n = int(first["plan"].info.blocks)
    print("4K RGB8 Mallat closed loop, MQ, SOP + EPH, %s, %d blocks, %d bytes of tile-parts; %s; %d contexts; alone: ms, mean / min of %d after %d" %
          ("512 x 512 tiles" if tile else "untiled", n, first["total"], "area calls" if have else "no area calls in this package", CONTEXTS, REP, WARM), flush=True)
    print("reduce  window            blocks needed    alone mean / min ms    in flight calls/s    area_blocks launch ms", flush=True)
    rows = []
    for r in (0, 1):
        full = None
        for side in (0, 512, 1024, 2048):
            area = centre(side) if side else None
            if area and not have:
                continue
            alone = timed(first, lambda: call(first, r, area))
            first["plan"].frame_status()
            got = call(first, r, area).cpu().numpy()
            first["plan"].frame_status()
            needed, ab = n, None
            if area is None:
                full = got
                if r == 0:
                    assert np.array_equal(got, first["pix"]), "the call without area does not give back the source"
            else:
                m = (1 << r) - 1
                x0, y0, x1, y1 = ((v + m) >> r for v in area)
                assert np.array_equal(got, full[y0:y1, 4 * x0:4 * x1]), "window differs from the crop of the full decode"
                need = first["plan"].area_blocks(area, r)
                first["ctx"].sync()
                needed = int(need.sum().item())
                ab = timed(first, lambda: first["plan"].area_blocks(area, r))
            rate = in_flight(lanes, r, area)
            rows.append(dict(reduce=r, window=side, needed=needed, total=n, alone_ms_mean=alone[0], alone_ms_min=alone[1], in_flight_per_s=rate,
                             area_blocks_ms_mean=ab and ab[0], area_blocks_ms_min=ab and ab[1]))
            print("%6d  %-16s %7d / %-7d %9.2f / %-9.2f %14.1f           %s" % (r, "%d^2" % side if side else "whole frame", needed, n, alone[0], alone[1], rate,
                                                                              "%.3f / %.3f" % ab if ab else "-"), flush=True)
    out["tile%d" % tile] = dict(area_calls=have, blocks=n, bytes=first["total"], contexts=CONTEXTS, rows=rows)
    for ln in lanes:
        ln["plan"].close()
        ln["ctx"].close()
if "--json" in sys.argv:
    with open(_arg("--json", ""), "w") as f:
        json.dump(out, f)
