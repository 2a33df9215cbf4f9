"""What the rate tables and the allocation cost on the device: 3840x2160 RGB, 12 bit, 64x64 blocks, Mallat closed loop, MQ coder, one context
(one frame at a time).  HIP events around encode_blocks (the plain block encode), encode_blocks(planes=True) (the PLANES kernels + the
distortion kernel) and rate_allocate at budgets of 100 / 50 / 25 / 10 % of the unconstrained body bytes: mean and min of 10 calls after 2,
in ms.  Beside every budget: the bytes chosen, the blocks cut inside / dropped, and a PSNR ESTIMATE of that choice from the tables (the
weighted squared coefficient errors, i.e. each band's error times its synthesis gain, over the samples; peak 2^12 - 1; the colour transform
is not accounted for) next to the uniform floor skip_planes = k with the nearest byte count.  Then the frame calls at the same budgets:
encode_frame_pixels(max_body_bytes=...) and decode_frame_pixels(truncated=True) timed the same way, the frame's bytes, and the PSNR of the
DECODED picture (16-bit samples, against the lossless decode) beside the uniform skip_planes of the whole stream that comes nearest from
below.  Information: nothing is asserted but that the tables-filling encode writes the plain encode's bytes.

A library without j2k_plan_encode_blocks_planes is measured through encode_blocks alone: the same script gives the row of an older checkout
when it is put beside that checkout's package.      python tools/rate_encode_time.py [--json FILE]"""
import json
import os
import sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-jpeg2000_amd"))
from j2kgfx.codec import FramePlan         # noqa: E402
from j2kgfx.context import Context         # noqa: E402

WARM, REP = 2, 10
ctx = Context(0)
have = hasattr(ctx.L, "j2k_plan_encode_blocks_planes")
W, H, PREC = 3840, 2160, 12
rng = np.random.default_rng(1)
yy, xx = np.mgrid[0:H, 0:W]
top = (1 << PREC) - 1
frame = np.clip(np.stack([xx * top // W, yy * top // H, (xx + yy) * (top // 2) // W]) + rng.integers(-64, 65, (3, H, W)), 0, top).astype(np.int32)
plan = FramePlan(W, H, 3, precision=PREC, lossless=True, num_resolutions=6, cb=(64, 64), coder=0, ctx=ctx, mallat=True, track_streams=False)
ext = torch.cuda.ExternalStream(ctx.stream)
n = int(plan.info.blocks)
coeff = plan.forward(torch.from_numpy(frame).to(plan.device))
ctx.sync()


def timed(f):
    ms = []
    for i in range(WARM + REP):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext); f(); e1.record(ext)
        ctx.sync()
        if i >= WARM:
            ms.append(e0.elapsed_time(e1))
    return float(np.mean(ms)), float(np.min(ms))


slots = plan.empty(plan.info.bytes_cap, torch.uint8); lens = plan.empty(n, torch.int32); nbs = plan.empty(n, torch.uint8)
plain = timed(lambda: plan.encode_blocks(coeff, slots, lens, nbs))
total = int(lens[:n].to(torch.int64).sum().item())
out = dict(planes_entries=have, blocks=n, body_bytes=total, encode_blocks_ms=plain, rows=[])
print("4K RGB 12 bit Mallat closed loop, MQ, %d blocks, %d body bytes; ms, mean / min of %d calls after %d" % (n, total, REP, WARM), flush=True)
print("encode_blocks                   %8.2f / %-8.2f" % plain, flush=True)
# the whole plain frame call: the same picture as image.RGBA64 pixels (big-endian 16-bit samples, rescaled to 12 bits by the call) -> tile-parts
from j2kgfx import _lib                    # noqa: E402
p16 = np.full((H, W, 4), 0xFFFF, np.uint16); p16[..., :3] = (frame.transpose(1, 2, 0) << 4).astype(np.uint16)
d_pix = torch.from_numpy(p16.astype(">u2").view(np.uint8).reshape(H, W * 8)).to(plan.device)
cs = plan.empty(plan.frame_bound(), torch.uint8); toffs = plan.empty(int(plan.info.tiles) + 1, torch.int64)[:int(plan.info.tiles) + 1]
whole = timed(lambda: plan.encode_frame_pixels(_lib.PIX_RGBA64, d_pix, False, False, cs, toffs))
plan.frame_status()
out["encode_frame_pixels_ms"] = whole
out["frame_bytes"] = int(toffs[-1].item())
print("encode_frame_pixels             %8.3f / %-8.3f   (%d bytes of tile-parts)" % (whole + (out["frame_bytes"],)), flush=True)
if have:
    s2 = plan.empty(plan.info.bytes_cap, torch.uint8); l2 = plan.empty(n, torch.int32); n2 = plan.empty(n, torch.uint8)
    res = []
    tab = timed(lambda: res.append(plan.encode_blocks(coeff, s2, l2, n2, planes=True)))
    rate, dist = res[-1][3], res[-1][4]
    assert torch.equal(l2[:n], lens[:n]) and torch.equal(n2[:n], nbs[:n]) and torch.equal(s2, slots), "the tables-filling encode writes other bytes"
    out["encode_blocks_planes_ms"] = tab
    print("encode_blocks(planes=True)      %8.2f / %-8.2f   (the PLANES kernels + the distortion kernel; each alone: not measured)" % tab, flush=True)
    R = rate.cpu().numpy().view(np.uint32).astype(np.int64)[:n]
    # every block's weight (jobs run component -> resolution -> band): weighted coefficient errors estimate the picture's error
    wt, wj, r, last = plan.rate_weights(), [], 0, None
    for b in plan.blocks():
        key = (int(b["plane"]), int(b["band"]))
        if last is not None and key != last:
            r = 0 if key[0] != last[0] else (r + 1 if (key[1] < last[1] or last[1] == 0) else r)
        wj.append(wt[key[0] % 3, r, key[1]])
        last = key
    D = dist.cpu().numpy().view(np.uint64)[:n].astype(np.float64) * np.array(wj)[:, None]
    nb = nbs.cpu().numpy()[:n].astype(np.int64)
    samples = float(3 * W * H)
    psnr = lambda sse: float("inf") if sse == 0 else 10 * np.log10(top ** 2 / (sse / samples))
    uniform = []                                                     # (bytes, PSNR) of every uniform floor k
    for k in range(0, 16):
        p = np.maximum(nb - k, 0)
        uniform.append((k, int(R[np.arange(n), p].sum()), psnr(float(D[np.arange(n), p].sum()))))
    print("budget %   rate_allocate            bytes chosen   cut inside  dropped   PSNR (coefficients)   nearest uniform floor: k, bytes, PSNR", flush=True)
    for pct in (100, 50, 25, 10):
        budget = total * pct // 100
        got = []
        t = timed(lambda: got.append(plan.rate_allocate(rate, dist, nbs, budget)))
        kept = got[-1][0].cpu().numpy()[:n].astype(np.int64)
        chosen = int(got[-1][1].item())
        sse = float(D[np.arange(n), kept].sum())
        k, ub, up = min(uniform, key=lambda u: abs(u[1] - chosen))
        row = dict(budget_pct=pct, budget=budget, allocate_ms=t, chosen=chosen, cut_inside=int(((kept > 0) & (kept < nb)).sum()), dropped=int(((kept == 0) & (nb > 0)).sum()),
                   psnr=psnr(sse), uniform_k=k, uniform_bytes=ub, uniform_psnr=up)
        out["rows"].append(row)
        print("%7d   %8.2f / %-8.2f   %14d   %10d  %7d   %19.2f   %d, %d, %.2f" % (pct, t[0], t[1], chosen, row["cut_inside"], row["dropped"], row["psnr"], k, ub, up), flush=True)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(out, f)

# ---- the frame calls: encode_frame_pixels(max_body_bytes) and decode_frame_pixels(truncated=True), pictures decoded ------------------------
if have and hasattr(ctx.L, "j2k_plan_encode_frame_pixels_rate"):
    def rgb(t):                                                  # RGBA64 pixels (big-endian 16-bit) -> float64 [H, W, 3]
        return t.cpu().numpy().reshape(H, W, 4, 2).astype(np.float64)[..., :3, :] @ np.array([256.0, 1.0])

    def psnr16(a, b):
        mse = float(((a - b) ** 2).mean())
        return float("inf") if mse == 0 else 10 * np.log10(65535.0 ** 2 / mse)

    back = torch.zeros((H, W * 8), dtype=torch.uint8, device=plan.device)
    plan.decode_frame_pixels(cs, out["frame_bytes"], back, toffs)
    plan.frame_status()
    src = rgb(back)                                              # the lossless decode: the picture itself
    flat = []                                                        # uniform floors on the WHOLE stream: (k, PSNR)
    for k in range(1, 9):
        plan.decode_frame_pixels(cs, out["frame_bytes"], back, toffs, skip_planes=k)
        plan.frame_status()
        flat.append((k, psnr16(rgb(back), src)))
    print("budget %%   encode_frame_pixels(max_body_bytes)   frame bytes   decode_frame_pixels(truncated)   PSNR, dB   uniform skip_planes with the nearest PSNR below: k, PSNR (its stream: all %d bytes)" % out["frame_bytes"], flush=True)
    cs2 = plan.empty(plan.frame_bound(), torch.uint8); toffs2 = plan.empty(int(plan.info.tiles) + 1, torch.int64)[:int(plan.info.tiles) + 1]
    out["frame_rows"] = []
    for pct in (100, 50, 25, 10):
        budget = total * pct // 100
        enc = timed(lambda: plan.encode_frame_pixels(_lib.PIX_RGBA64, d_pix, False, False, cs2, toffs2, max_body_bytes=budget))
        plan.frame_status()
        fb = int(toffs2[-1].item())
        dec = timed(lambda: plan.decode_frame_pixels(cs2, fb, back, toffs2, truncated=True))
        plan.frame_status()
        p = psnr16(rgb(back), src)
        below = [u for u in flat if u[1] <= p] or [flat[-1]]
        k, up = max(below, key=lambda u: u[1])
        out["frame_rows"].append(dict(budget_pct=pct, encode_ms=enc, frame_bytes=fb, decode_ms=dec, psnr=p, uniform_k=k, uniform_psnr=up))
        print("%7d   %10.2f / %-10.2f            %11d   %10.2f / %-10.2f        %8.2f   %d, %.2f" % (pct, enc[0], enc[1], fb, dec[0], dec[1], p, k, up), flush=True)
    print("uniform floors on the whole stream: " + ", ".join("k=%d %.2f dB" % u for u in flat), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(out, f)
