"""What a quality target costs and what it gives (docs/KERNEL_NOTES.md, "Quality-targeted encode").  Information: nothing is asserted but that
the byte budget used for the comparison gives the quality call's cuts.

1. Time, with tools/rate_encode_time.py's method (its 3840x2160 RGB 12-bit frame, 64x64 blocks, Mallat closed loop, MQ, one context; HIP events
   on the context's stream, mean and min of 10 calls after 2, in ms): encode_frame_pixels(min_psnr=dB) against encode_frame_pixels(max_body_bytes=B)
   with B = the body bytes the quality call chose (the same cuts: checked through the stage calls), the two alternating; and the allocation
   launches alone on that frame's tables: rate_allocate_layers against rate_allocate_quality for 1 and 3 layers.
2. The image-domain result on the frames of tests/test_gpu_quality_encode.py (64x48 and 192x128 8-bit RGB, 8x8 blocks, 5-3 and 9-7 at quality
   20) at min_psnr = 30 / 40 / 50 dB: the PSNR pixels.psnr reports for the decoded frame, the same figure from the oracle's composition on the
   CPU for the definition's cuts, the estimate 10 log10(N peak^2 q^2 / achieved), and the body bytes.

    python tools/quality_encode_time.py [--json FILE] [--skip-4k]"""
import json
import os
import sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "go-jpeg2000_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
from j2kgfx import _lib, pixels            # noqa: E402
from j2kgfx.codec import FramePlan         # noqa: E402
from j2kgfx.context import Context         # noqa: E402

WARM, REP = 2, 10
ctx = Context(0)
ext = torch.cuda.ExternalStream(ctx.stream)
out = {}


def timed_pair(f, g):
    """two calls alternating: ((mean, min) of f, (mean, min) of g)"""
    ms = ([], [])
    for i in range(WARM + REP):
        for k, fn in enumerate((f, g)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext); fn(); e1.record(ext)
            ctx.sync()
            if i >= WARM:
                ms[k].append(e0.elapsed_time(e1))
    return tuple((float(np.mean(m)), float(np.min(m))) for m in ms)


# ---- 1. time ------------------------------------------------------------------------------------------------------------------------------------
if "--skip-4k" not in sys.argv:
    W, H, PREC = 3840, 2160, 12
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:H, 0:W]
    top = (1 << PREC) - 1
    frame = np.clip(np.stack([xx * top // W, yy * top // H, (xx + yy) * (top // 2) // W]) + rng.integers(-64, 65, (3, H, W)), 0, top).astype(np.int32)
    plan = FramePlan(W, H, 3, precision=PREC, lossless=True, num_resolutions=6, cb=(64, 64), coder=0, ctx=ctx, mallat=True, track_streams=False)
    n, nt = int(plan.info.blocks), int(plan.info.tiles)
    p16 = np.full((H, W, 4), 0xFFFF, np.uint16); p16[..., :3] = (frame.transpose(1, 2, 0) << 4).astype(np.uint16)
    d_pix = torch.from_numpy(p16.astype(">u2").view(np.uint8).reshape(H, W * 8)).to(plan.device)
    coeff = plan.forward_pixels(_lib.PIX_RGBA64, d_pix)
    slots, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True)
    ctx.sync()
    total = int(lens[:n].to(torch.int64).sum().item())
    cs = plan.empty(plan.frame_bound(), torch.uint8); toffs = plan.empty(nt + 1, torch.int64)[:nt + 1]
    cs2 = plan.empty(plan.frame_bound(), torch.uint8); toffs2 = plan.empty(nt + 1, torch.int64)[:nt + 1]
    print("4K RGB 12 bit Mallat closed loop, MQ, %d blocks, %d body bytes; ms, mean / min of %d calls after %d, the two calls alternating" % (n, total, REP, WARM), flush=True)
    print("  dB   encode_frame_pixels(min_psnr)   encode_frame_pixels(max_body_bytes=B)   B = body bytes   frame bytes", flush=True)
    out["frame_rows"] = []
    for db in (40.0, 50.0, 60.0):
        T = plan.psnr_distortion(db)
        kq, cq, aq = plan.rate_allocate_quality(rate, dist, nbs, [T])
        ctx.sync()
        B = int(cq[0].item())
        kb, cb_ = plan.rate_allocate(rate, dist, nbs, B)
        ctx.sync()
        assert torch.equal(kq[0], kb[:n]) and int(cb_.item()) == B, "the byte budget does not give the quality call's cuts"
        tq, tb = timed_pair(lambda: plan.encode_frame_pixels(_lib.PIX_RGBA64, d_pix, False, False, cs, toffs, min_psnr=db),
                            lambda: plan.encode_frame_pixels(_lib.PIX_RGBA64, d_pix, False, False, cs2, toffs2, max_body_bytes=B))
        plan.frame_status()
        fb = int(toffs[-1].item())
        assert fb == int(toffs2[-1].item()) and torch.equal(cs[:fb], cs2[:fb])
        out["frame_rows"].append(dict(db=db, quality_ms=tq, budget_ms=tb, body_bytes=B, frame_bytes=fb))
        print("%4.0f   %12.3f / %-12.3f   %14.3f / %-14.3f   %14d   %11d" % (db, tq[0], tq[1], tb[0], tb[1], B, fb), flush=True)
    print("  layers   rate_allocate_layers     rate_allocate_quality   (the allocation launch alone, the same tables, budgets = the quality choices' bytes)", flush=True)
    out["alloc_rows"] = []
    for dbs in ((50.0,), (40.0, 50.0, 60.0)):
        Ts = [plan.psnr_distortion(d) for d in dbs]
        kq, cq, aq = plan.rate_allocate_quality(rate, dist, nbs, Ts)
        ctx.sync()
        Bs = [int(x) for x in cq.cpu().numpy()]
        tb, tq = timed_pair(lambda: plan.rate_allocate_layers(rate, dist, nbs, Bs), lambda: plan.rate_allocate_quality(rate, dist, nbs, Ts))
        out["alloc_rows"].append(dict(layers=len(dbs), layers_ms=tb, quality_ms=tq))
        print("%8d   %8.3f / %-8.3f      %8.3f / %-8.3f" % (len(dbs), tb[0], tb[1], tq[0], tq[1]), flush=True)
    plan.close()

# ---- 2. what came out -------------------------------------------------------------------------------------------------------------------------------
import oracle as orc                       # noqa: E402
import quality_cases as qc                 # noqa: E402
import test_gpu_layers as tl               # noqa: E402
import test_gpu_rate_frames as rf          # noqa: E402

print("frame, wavelet      min_psnr   pixels.psnr (device)   oracle composition (CPU)   estimate from achieved   body bytes   of uncut", flush=True)
out["psnr_rows"] = []
for case in ((64, 48, 3, 8, (0, 0), 2), (192, 128, 3, 8, (0, 0), 3)):
    for lossless, q in ((True, 0), (False, 20)):
        spec = (case, lossless, q, 8)
        W, H, Cn, prec, tile, nres = case
        plan = tl._plan(ctx, spec)
        F = tl.Frame(torch, plan, spec)
        Hs = qc.Hulls(F.R, F.D, F.nbs, F.ws)
        src = F.pix.reshape(H, -1, 4)[:, :W, :3].astype(np.int64)
        for db in (30.0, 40.0, 50.0):
            cs, toffs, ach = plan.encode_frame_pixels(F.fmt, F.d_pix, min_psnr=db)
            plan.frame_status()
            back = torch.zeros((H, W * 4), dtype=torch.uint8, device=plan.device)
            plan.decode_frame_pixels(cs, int(toffs[-1].item()), back, truncated=True)
            plan.frame_status()
            dev = pixels.psnr(F.fmt, back, F.d_pix, W, H, ctx=ctx)
            ps, b, S = Hs.search(plan.psnr_distortion(db))
            exp = rf._expected_pixels(orc, case, lossless, q, F.ctiles, F.wins, [nb - p for nb, p in zip(F.nbs, ps)], 0)
            cpu = qc.psnr(int(((exp.reshape(H, -1, 4)[:, :W, :3].astype(np.int64) - src) ** 2).sum()), W * H * 3, 255)
            a = float(ach[0].item())
            est = float("inf") if a == 0 else db + 10.0 * float(np.log10(plan.psnr_distortion(db) / a))
            out["psnr_rows"].append(dict(frame="%dx%d" % (W, H), wavelet="5-3" if lossless else "9-7 q%d" % q, min_psnr=db, device_psnr=dev, oracle_psnr=cpu, estimate=est,
                                         body_bytes=b, uncut=F.U))
            print("%-8s %-9s %8.0f   %20.2f   %24.2f   %22.2f   %10d   %8d" % ("%dx%d" % (W, H), "5-3" if lossless else "9-7 q%d" % q, db, dev, cpu, est, b, F.U), flush=True)
        plan.close()
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(out, f)
