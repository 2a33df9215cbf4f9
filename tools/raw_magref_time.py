"""What the raw-MagRef coding style (j2k_plan_set_raw_magref) costs and buys on the device, on bench.py --config cl's geometry: 3840x2160 RGB8,
lossless, 512x512 tiles, 64x64 blocks, six resolutions, closed loop, MQ coder, SOP + EPH -- style off and on in the same process.

  --mode alone   one context, one frame at a time: HIP events around encode_frame_pixels and decode_frame_pixels, ms, mean / min of --reps frames
  --mode batch   bench.py's batch shape, 12 contexts x 4 frames per plan (frame_rows): wall time of a step of all contexts, Gpixel/s
  --style 0|1|both   (both: off first, then on)

GPU_MAX_HW_QUEUES: 32 unless the environment already sets it (bench.py --config cl asks for the same); the value in force is printed, and the
batch row depends on it.  --only encode|decode (batch): one direction per step.
Prints the stream sizes both ways and, with --share, the MagRef share of the MQ symbols of the frame (CPU: tests/raw_magref_cases.py on every
16th block).  Every decoded frame is compared with the source.  For per-kernel times run one style per process under
rocprofv3 --kernel-trace --stats -- python tools/raw_magref_time.py --mode alone --style 1     [--json FILE]

--pkg DIR: import j2kgfx from DIR (with its libj2kgfx.so beside the package) instead of this checkout's -- an older checkout's build measures its
plain mode with the same script (--style 0; the setter is not called where the package has none)."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")      # as bench.py --config cl: a hardware queue per context of the batch shape (read when HIP initialises)

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(sys.argv[sys.argv.index("--pkg") + 1]) if "--pkg" in sys.argv else os.path.join(ROOT, "go-jpeg2000_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from j2kgfx import _lib                    # noqa: E402  (before bench_host, which puts this checkout's package first on the path)
from j2kgfx.codec import FramePlan         # noqa: E402
from j2kgfx.context import Context         # noqa: E402
import bench_host                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["alone", "batch"], default="alone")
ap.add_argument("--style", choices=["0", "1", "both"], default="both")
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--share", action="store_true")
ap.add_argument("--json", default=None)
ap.add_argument("--pkg", default=None)
ap.add_argument("--only", choices=["both", "encode", "decode"], default="both", help="--mode batch: the direction(s) a step runs (decode: of streams encoded once)")
args = ap.parse_args()
W, H, C, TILE, NRES, CB, PREC = bench_host.W, bench_host.H, bench_host.C, bench_host.TILE, bench_host.NRES, bench_host.CB, bench_host.PREC
styles = [0, 1] if args.style == "both" else [int(args.style)]
out = dict(mode=args.mode, rows=[], hw_queues=os.environ["GPU_MAX_HW_QUEUES"])
print("GPU_MAX_HW_QUEUES=%s" % os.environ["GPU_MAX_HW_QUEUES"])


def lane(index, batch):
    ctx = Context(0)
    p = FramePlan(W, H * batch, C, precision=PREC, lossless=True, num_resolutions=NRES, cb=(CB, CB), tile=(TILE, TILE), coder=0, ctx=ctx, track_streams=False,
                  closed_loop=True, frame_rows=H if batch > 1 else 0)
    base = bench_host._rgba_host(np, index)
    pix = torch.from_numpy(np.concatenate([base if b == 0 else np.roll(base, (41 * b, 388 * b), axis=(0, 1)) for b in range(batch)], axis=0)).to(p.device)
    nt = int(p.info.tiles)
    return dict(ctx=ctx, p=p, pix=pix, back=torch.zeros_like(pix), cs=p.empty(p.frame_bound(), torch.uint8), toffs=p.empty(nt + 1, torch.int64)[:nt + 1])


def code(ln, enc=True, dec=True):
    p = ln["p"]
    if enc:
        p.encode_frame_pixels(_lib.PIX_RGBA8, ln["pix"], sop=True, eph=True, out=ln["cs"], tile_offs=ln["toffs"])
    if dec:
        p.decode_frame_pixels(ln["cs"], ln["cs"].numel(), ln["back"], tile_offs=ln["toffs"], sop=True, eph=True)


if args.mode == "alone":
    ln = lane(0, 1)
    ext = torch.cuda.ExternalStream(ln["ctx"].stream)

    def timed(f):
        ms = []
        for i in range(args.warm + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext); f(); e1.record(ext)
            ln["ctx"].sync()
            if i >= args.warm:
                ms.append(e0.elapsed_time(e1))
        return float(np.mean(ms)), float(np.min(ms))

    print("4K RGB8 lossless closed loop, MQ, SOP + EPH, %d blocks, one frame alone; ms, mean / min of %d frames after %d" % (int(ln["p"].info.blocks), args.reps, args.warm))
    print("style   encode_frame_pixels     decode_frame_pixels    tile-part bytes", flush=True)
    for s in styles:
        if hasattr(ln["p"], "set_raw_magref"):
            ln["p"].set_raw_magref(bool(s))
        else:
            assert s == 0, "this package has no raw-MagRef style"
        enc = timed(lambda: code(ln, dec=False))
        dec = timed(lambda: code(ln, enc=False))
        ln["p"].frame_status()
        total = int(ln["toffs"][-1].item())
        assert torch.equal(ln["back"], ln["pix"]), "the frame did not come back"
        out["rows"].append(dict(style=s, encode_ms_mean=enc[0], encode_ms_min=enc[1], decode_ms_mean=dec[0], decode_ms_min=dec[1], bytes=total))
        print("%5d   %9.2f / %-9.2f   %9.2f / %-9.2f   %d" % (s, enc[0], enc[1], dec[0], dec[1], total), flush=True)
else:
    F, B = 12, 4
    lanes = [lane(f, B) for f in range(F)]
    torch.cuda.synchronize()

    def barrier():
        for ln in lanes:
            ln["ctx"].sync()
        torch.cuda.synchronize()

    print("4K RGB8 lossless closed loop, MQ, SOP + EPH: %d contexts x %d frames per plan; encode + decode of every frame per step" % (F, B))
    print("style   ms per step    Gpixel/s (%s)   tile-part bytes of context 0" % ("both directions" if args.only == "both" else args.only), flush=True)
    for s in styles:
        for ln in lanes:
            if hasattr(ln["p"], "set_raw_magref"):
                ln["p"].set_raw_magref(bool(s))
            else:
                assert s == 0, "this package has no raw-MagRef style"
        kw = dict(enc=args.only != "decode", dec=args.only != "encode")
        for ln in lanes:
            code(ln)                                   # (a decode-only step needs streams of this style)
        for _ in range(max(args.warm, 1)):
            for ln in lanes:
                code(ln, **kw)
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            for ln in lanes:
                code(ln, **kw)
        barrier()
        dt = (time.perf_counter() - t0) / args.reps
        for ln in lanes:
            ln["p"].frame_status()
            assert torch.equal(ln["back"], ln["pix"]), "a frame did not come back"
        total = int(lanes[0]["toffs"][-1].item())
        gp = (2.0 if args.only == "both" else 1.0) * F * B * W * H / dt / 1e9
        out["rows"].append(dict(style=s, step_ms=dt * 1e3, gpixel_s=gp, bytes=total))
        print("%5d   %10.1f   %10.2f   %d" % (s, dt * 1e3, gp, total), flush=True)

if args.share:
    import oracle as orc
    import pyref
    import raw_magref_cases as rm
    frame = bench_host._rgba_host(np, 0).reshape(H, W, 4)[..., :3].transpose(2, 0, 1).astype(np.int32)
    tile = np.ascontiguousarray(frame[:, :TILE, :TILE])
    coeff = orc.preprocess([tile[c] for c in range(C)], TILE, TILE, PREC, True, NRES)
    jobs = orc.enumerate_blocks(C, TILE, TILE, NRES, CB, CB, 1)
    mag = allsym = 0
    for j in jobs[::16]:
        counts = [0, 0]

        class Enc(pyref.MQEncoder):
            def encode(self, ctx, decision):
                counts[ctx in rm.MAG_CTXS] += 1
                super().encode(ctx, decision)
        t = pyref.T1(int(j["w"]), int(j["h"]))
        t.set_data([int(v) for v in rm.extract(coeff[int(j["comp"])], TILE, TILE, j).reshape(-1)])
        with rm._coders(enc=Enc):
            t.encode(int(j["band"]))
        mag += counts[1]; allsym += counts[0] + counts[1]
    out["magref_share"] = mag / max(allsym, 1)
    print("MagRef share of the MQ symbols (tile 0, every 16th block, %d symbols): %.1f %%" % (allsym, 100.0 * mag / max(allsym, 1)))

if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f)
