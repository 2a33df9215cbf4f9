"""What pass-level rate control (pass_cuts=True) costs and buys on the device, on the 4K RGB8 frame of bench.py --config cl as a closed-loop Mallat
plan: 3840x2160, lossless 5-3, 512x512 tiles, 64x64 blocks, six resolutions, MQ coder, SOP + EPH -- plane cuts and pass cuts in the same process.

  encode   encode_frame_pixels(max_body_bytes = 35 % of the uncut bodies): plane cuts against pass cuts, under the two-kernel and the one-kernel
           block encoder form (t1_split 1 / 0); HIP events around the call, ms, mean / min of --reps frames
  decode   decode_frame_pixels of the 35 % streams: truncated=True on the plane-cut stream against pass_cuts=True on the pass-cut stream (and
           truncated=True on the pass-cut stream, which reads its whole planes), with the plane-stepped path forced on (t1_dec_split 1) and off (0)
           and as the context chooses
  quality  at the budgets 5, 10, 20, 40 and 60 % of the uncut bodies: pixels.psnr of the decoded frame and the body + header bytes the frame took,
           plane cuts against pass cuts
--pkg DIR: import j2kgfx from DIR (with its libj2kgfx.so beside the package) instead of this checkout's -- an older checkout's build measures its
plane-cut rows with the same script (the pass rows are left out where the package has no pass_cuts).  [--json FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(sys.argv[sys.argv.index("--pkg") + 1]) if "--pkg" in sys.argv else os.path.join(ROOT, "go-jpeg2000_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from j2kgfx import _lib, pixels            # noqa: E402  (before bench_host, which puts this checkout's package first on the path)
from j2kgfx.codec import FramePlan         # noqa: E402
from j2kgfx.context import Context         # noqa: E402
import bench_host                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--json", default=None)
ap.add_argument("--pkg", default=None)
ap.add_argument("--only", choices=["all", "encode", "decode", "quality"], default="all")
args = ap.parse_args()
W, H, C, TILE, NRES, CB, PREC = bench_host.W, bench_host.H, bench_host.C, bench_host.TILE, bench_host.NRES, bench_host.CB, bench_host.PREC
HAVE_PASSES = "j2k_plan_encode_frame_pixels_passes" in _lib.SYMBOLS
out = dict(package=PKG, have_passes=HAVE_PASSES, rows=[])
base = torch.from_numpy(bench_host._rgba_host(np, 0))


def lane(**opts):
    ctx = Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    p = FramePlan(W, H, C, precision=PREC, lossless=True, num_resolutions=NRES, cb=(CB, CB), tile=(TILE, TILE), coder=0, ctx=ctx, track_streams=False, mallat=True)
    pix = base.to(p.device)
    nt = int(p.info.tiles)
    return dict(ctx=ctx, p=p, pix=pix, back=torch.zeros_like(pix), cs=p.empty(p.frame_bound(), torch.uint8), toffs=p.empty(nt + 1, torch.int64)[:nt + 1])


def close(ln):
    ln["p"].close()
    ln["ctx"].close()


def timed(ln, f):
    ext = torch.cuda.ExternalStream(ln["ctx"].stream)
    ms = []
    for i in range(args.warm + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext); f(); e1.record(ext)
        ln["ctx"].sync()
        if i >= args.warm:
            ms.append(e0.elapsed_time(e1))
    ln["p"].frame_status()
    return float(np.mean(ms)), float(np.min(ms))


def encode(ln, budget, passes):
    kw = dict(pass_cuts=True) if passes else {}
    ln["p"].encode_frame_pixels(_lib.PIX_RGBA8, ln["pix"], sop=True, eph=True, out=ln["cs"], tile_offs=ln["toffs"], max_body_bytes=budget, **kw)


def decode(ln, passes):
    kw = dict(pass_cuts=True) if passes else dict(truncated=True)
    ln["p"].decode_frame_pixels(ln["cs"], ln["cs"].numel(), ln["back"], tile_offs=ln["toffs"], sop=True, eph=True, **kw)


def uncut_bodies(ln):
    p = ln["p"]
    coeff = p.forward_pixels(_lib.PIX_RGBA8, ln["pix"])
    lens = p.encode_blocks(coeff)[1]
    ln["ctx"].sync()
    return int(lens[:int(p.info.blocks)].to(torch.int64).sum().item())


def row(**kw):
    out["rows"].append(kw)
    print("  ".join("%s=%s" % (k, ("%.3f" % v) if isinstance(v, float) else v) for k, v in kw.items()), flush=True)


forms = [("planes", False)] + ([("passes", True)] if HAVE_PASSES else [])
ln = lane()
total = uncut_bodies(ln)
close(ln)
print("uncut code-block bodies: %d bytes" % total)
out["total"] = total
B35 = total * 35 // 100

if args.only in ("all", "encode"):
    for split in (1, 0):
        ln = lane(t1_split=split)
        for name, passes in forms:
            mean, best = timed(ln, lambda: encode(ln, B35, passes))
            row(what="encode", encoder="two-kernel" if split else "one-kernel", cuts=name, ms_mean=mean, ms_min=best, frame_bytes=int(ln["toffs"][-1].item()))
        close(ln)

if args.only in ("all", "decode"):
    for dsplit in (None, 1, 0):
        ln = lane(**({} if dsplit is None else dict(t1_dec_split=dsplit)))
        for stream, spasses in forms:
            encode(ln, B35, spasses)
            ln["p"].frame_status()
            for reader, rpasses in forms:
                if rpasses and not spasses:
                    continue                                         # (the pass reader on a plane-cut stream is the truncated reader's job)
                mean, best = timed(ln, lambda: decode(ln, rpasses))
                forms_ = ln["p"].mq_forms() if hasattr(ln["p"], "mq_forms") else None
                row(what="decode", plane_stepped={None: "default", 1: "forced on", 0: "off"}[dsplit], stream=stream, reader="pass_cuts" if rpasses else "truncated",
                    ms_mean=mean, ms_min=best, forms=str(forms_))
        close(ln)

if args.only in ("all", "quality"):
    ln = lane()
    for pct in (5, 10, 20, 40, 60):
        for name, passes in forms:
            encode(ln, total * pct // 100, passes)
            ln["p"].frame_status()
            decode(ln, passes)
            ln["p"].frame_status()
            db = pixels.psnr(_lib.PIX_RGBA8, ln["pix"], ln["back"], W, H, ctx=ln["ctx"])
            row(what="quality", budget_pct=pct, budget=total * pct // 100, cuts=name, frame_bytes=int(ln["toffs"][-1].item()), psnr_db=float(db))
    close(ln)

if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
