"""A/B of the closed loop over the prefix layout (j2k_params.closed_loop = 1) and over the Mallat decomposition (= 2), and of the
reduced-resolution decode, on the C2 geometry of bench.py: 3840 x 2160 RGB8, 512 x 512 tiles, 6 resolutions, 64 x 64 blocks, one frame resident on
the device, one context.  Every figure is the time between two events on the context's stream around ONE call (encode_frame_pixels /
decode_frame_pixels), after --warmup calls, over --steps calls: median, min and max in microseconds.  One JSON line per mode.

  python tools/mallat_ab.py --coder mq --mode prefix          # what the parent commit computes (run it on a parent build too: J2K_LIB=...)
  python tools/mallat_ab.py --coder mq --mode mallat --reduce 0 1 2 3

decode at reduce r: `decode_us` the whole call; `inverse_us` the 5-3 inverse dispatches' own time (j2k_ctx_profile_read_tag 2 + 3, profile
mode 2, measured in a second pass so that the stamps do not sit in the first; the 9-7 launches carry no stamps, the tool is lossless only);
`parse_us` the tile-part + packet parse alone (decode_tile_parts, the same at every r); `blocks_us` the stage calls decode_blocks +
place_blocks on ALL jobs, timed directly (the block decoder has no profile tag; at reduce > 0 its subset has no stage call, so there the
block-decode share is decode_us - parse_us - inverse_us, launch gaps included -- a remainder, not a measurement)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-jpeg2000_amd"))
sys.path.insert(0, ROOT)

W, H, C, TILE, NRES, CB, PREC = 3840, 2160, 3, 512, 6, 64, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coder", choices=["mq", "ht"], default="mq")
    ap.add_argument("--mode", choices=["prefix", "mallat"], default="mallat")
    ap.add_argument("--reduce", type=int, nargs="*", default=[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench_host
    from j2kgfx import CODER_HT, CODER_MQ, Context, _lib
    from j2kgfx.codec import FramePlan
    if not torch.cuda.is_available():
        raise SystemExit("tools/mallat_ab.py needs a HIP device")
    torch.cuda.set_device(0)
    ctx = Context(0)
    kw = dict(mallat=True) if args.mode == "mallat" else dict(closed_loop=True)
    p = FramePlan(W, H, C, precision=PREC, lossless=True, num_resolutions=NRES, cb=(CB, CB), tile=(TILE, TILE),
                  coder=CODER_HT if args.coder == "ht" else CODER_MQ, ctx=ctx, track_streams=False, **kw)
    pix = torch.from_numpy(bench_host._rgba_host(np, 0)).to(p.device)        # frame 0 of bench.py --config cl / clht
    cs = p.empty(p.frame_bound(), torch.uint8)
    toffs = p.empty(int(p.info.tiles) + 1, torch.int64)[:int(p.info.tiles) + 1]
    ext = torch.cuda.ExternalStream(ctx.stream, device=p.device)
    torch.cuda.synchronize()

    def timed(fn):
        for _ in range(max(args.warmup, 1)):
            fn()
        ctx.sync()
        us = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext)
            fn()
            e1.record(ext)
            ctx.sync()
            us.append(e0.elapsed_time(e1) * 1e3)
        return dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1))

    out = dict(coder=args.coder, mode=args.mode, steps=args.steps, warmup=args.warmup, lib=os.path.basename(os.path.dirname(_lib.LIB_PATH)) or _lib.LIB_PATH)
    out["encode_us"] = timed(lambda: p.encode_frame_pixels(_lib.PIX_RGBA8, pix, sop=True, eph=True, out=cs, tile_offs=toffs))
    p.frame_status()
    out["stream_bytes"] = int(toffs[-1].item())
    n = int(p.info.blocks)
    o2, l2, n2 = p.empty(n + 1, torch.int64), p.empty(n, torch.int32), p.empty(n, torch.uint8)
    out["parse_us"] = timed(lambda: p.decode_tile_parts(cs, cs.numel(), tile_offs=toffs, sop=True, eph=True, offs=o2, lens=l2, numbps=n2))
    decoded, coeff = p.empty(p.info.decoded_elems, torch.int32), p.alloc_coeff()
    out["blocks_us"] = timed(lambda: p.place_blocks(p.decode_blocks(cs, o2, l2, n2, decoded), coeff))
    out["decode"] = {}
    full = None
    for r in args.reduce:
        Hr, Wr = p.reduced_shape(r) if r else (H, W)
        back = torch.zeros((Hr, Wr * 4), dtype=torch.uint8, device=p.device)
        call = lambda: p.decode_frame_pixels(cs, cs.numel(), back, tile_offs=toffs, sop=True, eph=True, reduce=r)      # noqa: E731
        rec = dict(size="%dx%d" % (Wr, Hr), decode_us=timed(call))
        p.frame_status()
        ctx.profile_enable(2)
        ctx.profile_read()
        for _ in range(args.steps):
            call()
        ctx.sync()
        inv = sum(ctx.profile_read_tag(t)[1] for t in (2, 3)) * 1e3 / args.steps
        ctx.profile_enable(False)
        rec["inverse_us"] = round(inv, 1)
        if r == 0:
            full = back
            if args.coder == "mq":
                assert torch.equal(back, pix), "closed-loop round trip is not bit-exact"
        out["decode"][str(r)] = rec
    print(json.dumps(out))
    del full
    p.close()
    ctx.close()


if __name__ == "__main__":
    main()
