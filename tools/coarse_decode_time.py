"""What a skipped bit plane buys on the device: 3840x2160 RGB8, 512x512 tiles, 64x64 blocks, Mallat closed loop, MQ coder, SOP + EPH, one frame
alone.  HIP events around the whole decode call (decode_frame_pixels) and around decode_blocks, for skip_planes 0 ... 4 at reduce 0 and 1:
mean and min of 10 frames after 2 warm-up frames, in ms.  Every decoded frame is compared with the skip_planes = 0 pixels of its reduce
(reported: PSNR and the largest difference); the only assertion is that reduce 0, skip_planes 0 gives back the source.

A library without the j2k_*_coarse entries is measured through the old calls, skip_planes = 0 only: the same script gives the row of an
older checkout when it is put beside that checkout's package.      python tools/coarse_decode_time.py [--json FILE]"""
import json
import os
import sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-jpeg2000_amd"))
from j2kgfx import _lib                    # noqa: E402
from j2kgfx.codec import FramePlan         # noqa: E402
from j2kgfx.context import Context         # noqa: E402

WARM, REP = 2, 10
ctx = Context(0)
have = hasattr(ctx.L, "j2k_plan_decode_frame_pixels_coarse") and hasattr(ctx.L, "j2k_plan_decode_blocks_coarse")
W, H = 3840, 2160
rng = np.random.default_rng(1)
yy, xx = np.mgrid[0:H, 0:W]
frame = np.clip(np.stack([xx * 255 // W, yy * 255 // H, (xx + yy) * 127 // W]) + rng.integers(-16, 17, (3, H, W)), 0, 255).astype(np.uint8)
pix = np.full((H, W, 4), 255, np.uint8); pix[..., :3] = frame.transpose(1, 2, 0)
plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=6, cb=(64, 64), tile=(512, 512), coder=0, ctx=ctx, mallat=True, track_streams=False)
d_pix = torch.from_numpy(pix.reshape(H, W * 4)).to(plan.device)
ext = torch.cuda.ExternalStream(ctx.stream)
n = int(plan.info.blocks)
cs = plan.empty(plan.frame_bound(), torch.uint8); toffs = plan.empty(int(plan.info.tiles) + 1, torch.int64)[:int(plan.info.tiles) + 1]
plan.encode_frame_pixels(_lib.PIX_RGBA8, d_pix, True, True, cs, toffs)
plan.frame_status()
total = int(toffs[-1].item())
o2 = plan.empty(n + 1, torch.int64); l2 = plan.empty(n, torch.int32); n2 = plan.empty(n, torch.uint8)
plan.decode_tile_parts(cs, total, toffs, True, True, o2, l2, n2)
plan.frame_status()
decoded = plan.empty(plan.info.decoded_elems, torch.int32)


def timed(f):
    ms = []
    for i in range(WARM + REP):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext); f(); e1.record(ext)
        ctx.sync()
        if i >= WARM:
            ms.append(e0.elapsed_time(e1))
    return float(np.mean(ms)), float(np.min(ms))


rows = []
print("4K RGB8 Mallat closed loop, MQ, SOP + EPH, %d blocks, %d bytes of tile-parts; %s; ms, mean / min of %d frames after %d" %
      (n, total, "j2k_*_coarse entries" if have else "old entries (skip_planes = 0 only)", REP, WARM), flush=True)
print("reduce skip_planes   decode_frame_pixels      decode_blocks     PSNR vs skip 0   max |diff|", flush=True)
for r in (0, 1):
    Hr, Wr = plan.reduced_shape(r)
    base = None
    for k in (range(5) if have else (0,)):
        back = torch.zeros((Hr, Wr * 4), dtype=torch.uint8, device=plan.device)
        kw = dict(skip_planes=k) if have else {}
        whole = timed(lambda: plan.decode_frame_pixels(cs, total, back, toffs, True, True, reduce=r, **kw))
        plan.frame_status()
        got = back.cpu().numpy()
        if k == 0:
            base = got
            if r == 0:
                assert np.array_equal(got, pix.reshape(H, W * 4)), "skip_planes = 0 does not give back the source"
        d = got.astype(np.int32) - base.astype(np.int32)
        mse = float((d.astype(np.float64) ** 2).mean())
        psnr = float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
        blk = timed(lambda: plan.decode_blocks(cs, o2, l2, n2, decoded, **kw)) if r == 0 else None
        rows.append(dict(reduce=r, skip_planes=k, frame_ms_mean=whole[0], frame_ms_min=whole[1], blocks_ms_mean=blk and blk[0], blocks_ms_min=blk and blk[1],
                         psnr=psnr, max_diff=int(np.abs(d).max())))
        print("%6d %11d   %9.2f / %-9.2f  %s   %12.2f   %10d" % (r, k, whole[0], whole[1], "%7.2f / %-7.2f" % blk if blk else "      -          ", psnr, int(np.abs(d).max())),
              flush=True)
plan.frame_status()
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(dict(coarse_entries=have, blocks=n, bytes=total, rows=rows), f)
