"""What a region of interest costs the rate-limited encode (docs/KERNEL_NOTES.md 4z): 3840x2160 RGB8, 5-3, Mallat closed loop, MQ coder, 64x64
blocks, 6 resolutions, 512x512 tiles; the frame is tools/area_decode_time.py's gradient with +-16 of noise.  One context, one frame at a time, HIP
events around the call, mean / min of REP calls after WARM, ms:

  frame    encode_frame_pixels(max_body_bytes = a quarter of the uncut body bytes) without roi -- twice, for the run-to-run spread --, with
           roi = the 512^2 at the frame's centre, and with roi = the whole frame (every block multiplied); the same with three layers
  blocks   encode_blocks(planes=True) without and with those rectangles (the MQ coder and the distortion launch; the kernels' own times come
           from a run of this tool under `rocprofv3 --kernel-trace --stats`, which names rate_distortion_kernel and rate_distortion_roi_kernel)

Per rectangle also the blocks with a footprint, wholly / partly inside (roi_windows).  The only assertion: roi_gain = 1 gives the bytes of the
call without roi.
      python tools/roi_encode_time.py [--short] [--json FILE]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-jpeg2000_amd"))
from j2kgfx.codec import FramePlan         # noqa: E402
from j2kgfx.context import Context         # noqa: E402

SHORT = "--short" in sys.argv
WARM, REP = (1, 3) if SHORT else (2, 10)
W, H = 3840, 2160
PIX_RGBA8 = 2


def frame(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.clip(np.stack([xx * 255 // W, yy * 255 // H, (xx + yy) * 127 // W]) + rng.integers(-16, 17, (3, H, W)), 0, 255).astype(np.uint8)
    pix = np.full((H, W, 4), 255, np.uint8)
    pix[..., :3] = f.transpose(1, 2, 0)
    return pix.reshape(H, W * 4)


def timed(plan, fn):
    ms = []
    for i in range(WARM + REP):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s = plan._ext()
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        if i >= WARM:
            ms.append(e0.elapsed_time(e1))
    return dict(mean=round(float(np.mean(ms)), 4), min=round(float(np.min(ms)), 4))


def main():
    ctx = Context(0)
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=6, cb=(64, 64), tile=(512, 512), coder=0, ctx=ctx, mallat=True)
    d_pix = torch.from_numpy(frame(5)).to(plan.device)
    n, nt = int(plan.info.blocks), int(plan.info.tiles)
    coeff = plan.forward_pixels(PIX_RGBA8, d_pix)
    slots, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True)
    ctx.sync()
    U = int(lens[:n].to(torch.int64).sum().item())
    B, LB = U // 4, [U // 10, U // 4, U // 2]
    centre = ((W - 512) // 2, (H - 512) // 2, (W + 512) // 2, (H + 512) // 2)
    rects = {"none": None, "none again": None, "centre 512^2": centre, "whole frame": (0, 0, W, H)}
    out = plan.empty(plan.frame_bound_layers(3), torch.uint8)
    toffs = plan.empty(nt + 1, torch.int64)[:nt + 1]
    res = dict(blocks=n, body_bytes=U, budget=B, rows=[])
    bl = plan.blocks()
    for name, q in rects.items():
        kw = dict(roi=q, roi_gain=16) if q else {}
        row = dict(roi=name)
        if q:
            win = plan.roi_windows(q).cpu().numpy()
            inside = sum(1 for F, b in zip(win, bl) if (F[2], F[3]) == (int(b["w"]), int(b["h"])))
            row.update(footprint_blocks=int((win[:, 2] > 0).sum()), whole_blocks=inside)
        row["frame_rate"] = timed(plan, lambda: plan.encode_frame_pixels(PIX_RGBA8, d_pix, sop=True, eph=True, out=out, tile_offs=toffs, max_body_bytes=B, **kw))
        plan.frame_status()
        row["frame_bytes"] = int(toffs[-1].item())
        row["frame_layers"] = timed(plan, lambda: plan.encode_frame_pixels(PIX_RGBA8, d_pix, sop=True, eph=True, out=out, tile_offs=toffs, layer_bytes=LB, **kw))
        plan.frame_status()
        row["blocks_planes"] = timed(plan, lambda: plan.encode_blocks(coeff, slots=slots, lens=lens, numbps=nbs, planes=True, **kw))
        ctx.sync()
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    a, ta = plan.encode_frame_pixels(PIX_RGBA8, d_pix, max_body_bytes=B, roi=centre, roi_gain=1)
    plan.frame_status()
    la = int(ta[-1].item())
    a = a[:la].clone()
    b, tb = plan.encode_frame_pixels(PIX_RGBA8, d_pix, max_body_bytes=B)
    plan.frame_status()
    assert la == int(tb[-1].item()) and torch.equal(a, b[:la]), "roi_gain = 1 is not the call without roi"
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(res, f, indent=1)
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
