"""What rate control on a batch plan (FramePlan(frame_rows=..., rate_per_frame=True)) costs and buys on the device, on the 4K RGB8 frame of
bench.py --config cl as a closed-loop Mallat plan: 3840x2160, lossless 5-3, 512x512 tiles, 64x64 blocks, six resolutions, MQ coder, SOP + EPH --
a batch of --frames (4) such frames on ONE context, against the same frames one by one on a single-frame plan of the same context.

  encode   (a) the plain batch encode; (b) the batch encode with max_body_bytes at 10 % and at 40 % of one frame's uncut bodies (every frame
           under that budget); (c) --frames single-frame-plan calls with the same budgets.  The three are measured --rounds (3) times in turn,
           each time --warm + --reps calls; HIP events around the call(s), ms per BATCH, mean / min of the reps
  decode   decode_frame_pixels(truncated=True) of (b)'s stream against --frames single-frame decodes of (c)'s streams, the same way
  check    (b)'s tile-parts equal (c)'s from byte 14 of every tile-part on (what the timing compares computes the same thing)
[--json FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "go-jpeg2000_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from j2kgfx import _lib                    # noqa: E402
from j2kgfx.codec import FramePlan         # noqa: E402
from j2kgfx.context import Context         # noqa: E402
import bench_host                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
W, H, C, TILE, NRES, CB, PREC = bench_host.W, bench_host.H, bench_host.C, bench_host.TILE, bench_host.NRES, bench_host.CB, bench_host.PREC
F = args.frames
out = dict(frames=F, rows=[])

ctx = Context(0)
kw = dict(precision=PREC, lossless=True, num_resolutions=NRES, cb=(CB, CB), tile=(TILE, TILE), coder=0, ctx=ctx, track_streams=False, mallat=True)
batch = FramePlan(W, H * F, C, frame_rows=H, rate_per_frame=True, **kw)
single = FramePlan(W, H, C, **kw)
host = [torch.from_numpy(bench_host._rgba_host(np, f)) for f in range(F)]
pix1 = [h.to(single.device) for h in host]
pixb = torch.cat(pix1, dim=0).contiguous()
ntb, nt1 = int(batch.info.tiles), int(single.info.tiles)
csb, toffsb = batch.empty(batch.frame_bound(), torch.uint8), batch.empty(ntb + 1, torch.int64)[:ntb + 1]
cs1 = [single.empty(single.frame_bound(), torch.uint8) for _ in range(F)]
toffs1 = [single.empty(nt1 + 1, torch.int64)[:nt1 + 1] for _ in range(F)]
backb, back1 = torch.zeros_like(pixb), [torch.zeros_like(p) for p in pix1]
ext = torch.cuda.ExternalStream(ctx.stream)


def timed(f):
    ms = []
    for i in range(args.warm + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext); f(); e1.record(ext)
        ctx.sync()
        if i >= args.warm:
            ms.append(e0.elapsed_time(e1))
    batch.frame_status(); single.frame_status()
    return float(np.mean(ms)), float(np.min(ms))


def enc_batch(budget):
    kws = {} if budget is None else dict(max_body_bytes=budget)
    batch.encode_frame_pixels(_lib.PIX_RGBA8, pixb, sop=True, eph=True, out=csb, tile_offs=toffsb, **kws)


def enc_singles(budget):
    kws = {} if budget is None else dict(max_body_bytes=budget)
    for f in range(F):
        single.encode_frame_pixels(_lib.PIX_RGBA8, pix1[f], sop=True, eph=True, out=cs1[f], tile_offs=toffs1[f], **kws)


def dec_batch():
    batch.decode_frame_pixels(csb, csb.numel(), backb, tile_offs=toffsb, sop=True, eph=True, truncated=True)


def dec_singles():
    for f in range(F):
        single.decode_frame_pixels(cs1[f], cs1[f].numel(), back1[f], tile_offs=toffs1[f], sop=True, eph=True, truncated=True)


def row(**kws):
    out["rows"].append(kws)
    print("  ".join("%s=%s" % (k, ("%.3f" % v) if isinstance(v, float) else v) for k, v in kws.items()), flush=True)


coeff = single.forward_pixels(_lib.PIX_RGBA8, pix1[0])
lens = single.encode_blocks(coeff)[1]
ctx.sync()
total = int(lens[:int(single.info.blocks)].to(torch.int64).sum().item())
print("uncut code-block bodies of frame 0: %d bytes; %d frames per batch, %d blocks per frame" % (total, F, int(single.info.blocks)))
out["total"] = total

for pct in (10, 40):                        # what is timed computes the same thing
    b = total * pct // 100
    enc_batch(b); enc_singles(b)
    ctx.sync(); batch.frame_status(); single.frame_status()
    hb, tb = csb.cpu().numpy(), toffsb.cpu().numpy()
    for f in range(F):
        h1, t1 = cs1[f].cpu().numpy(), toffs1[f].cpu().numpy()
        for t in range(nt1):
            a, e = int(tb[f * nt1 + t]), int(tb[f * nt1 + t + 1])
            assert bytes(hb[a + 14:e]) == bytes(h1[int(t1[t]) + 14:int(t1[t + 1])]), (pct, f, t)
    dec_batch(); dec_singles()
    ctx.sync(); batch.frame_status(); single.frame_status()
    assert all(torch.equal(backb[f * H:(f + 1) * H], back1[f]) for f in range(F)), pct
print("batch tile-parts and pixels equal the single-frame plan's at 10 % and 40 %")

for rnd in range(args.rounds):
    mean, best = timed(lambda: enc_batch(None))
    row(what="encode", round=rnd, form="(a) batch, plain", ms_mean=mean, ms_min=best, bytes=int(toffsb[-1].item()))
    for pct in (10, 40):
        b = total * pct // 100
        mean, best = timed(lambda: enc_batch(b))
        row(what="encode", round=rnd, form="(b) batch, max_body_bytes %d %%" % pct, ms_mean=mean, ms_min=best, bytes=int(toffsb[-1].item()))
        mean, best = timed(lambda: enc_singles(b))
        row(what="encode", round=rnd, form="(c) %d single-frame calls, %d %%" % (F, pct), ms_mean=mean, ms_min=best, bytes=sum(int(t[-1].item()) for t in toffs1))
        mean, best = timed(dec_batch)
        row(what="decode", round=rnd, form="batch, truncated, %d %%" % pct, ms_mean=mean, ms_min=best)
        mean, best = timed(dec_singles)
        row(what="decode", round=rnd, form="%d single-frame decodes, %d %%" % (F, pct), ms_mean=mean, ms_min=best)

batch.close(); single.close(); ctx.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
