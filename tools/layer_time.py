"""What quality layers cost on the device: 3840x2160 RGB, 12 bit, 64x64 blocks, 6 resolutions, Mallat closed loop, MQ coder, one context (one
frame in flight).  HIP events around each call, mean and min of 10 calls after 2, in ms; the whole script is meant to be run several times
(a run's means are one sample of the run-to-run spread).

  encode_frame_pixels(max_body_bytes=U/2)           the path that may not change (also what an older checkout's package gives: --pkg DIR)
  encode_frame_pixels(layer_bytes=...) at L = 1, 3, 8   the cost of a layer
  rate_allocate_layers(L budgets) against L x rate_allocate
  decode_frame_pixels(truncated=True) on the one-layer stream against decode_frame_pixels(layers=L) and (layers=1) on the L = 3 and L = 8 streams,
  and decode_tile_parts(layers=k) alone (the layered packet read + the three gather launches)

    python tools/layer_time.py [--pkg DIR] [--json FILE] [--common]     DIR: a directory that holds the package j2kgfx and its libj2kgfx.so;
                                                                       --common: only the two calls an older checkout has as well"""
import json
import os
import sys
import numpy as np
import torch
pkg = sys.argv[sys.argv.index("--pkg") + 1] if "--pkg" in sys.argv else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-jpeg2000_amd")
sys.path.insert(0, pkg)
from j2kgfx import _lib                    # noqa: E402
from j2kgfx.codec import FramePlan         # noqa: E402
from j2kgfx.context import Context         # noqa: E402

WARM, REP = 2, 10
ctx = Context(0)
have = hasattr(ctx.L, "j2k_plan_encode_frame_pixels_layers")
W, H, PREC = 3840, 2160, 12
rng = np.random.default_rng(1)
yy, xx = np.mgrid[0:H, 0:W]
top = (1 << PREC) - 1
frame = np.clip(np.stack([xx * top // W, yy * top // H, (xx + yy) * (top // 2) // W]) + rng.integers(-64, 65, (3, H, W)), 0, top).astype(np.int32)
plan = FramePlan(W, H, 3, precision=PREC, lossless=True, num_resolutions=6, cb=(64, 64), coder=0, ctx=ctx, mallat=True, track_streams=False)
ext = torch.cuda.ExternalStream(ctx.stream)
n, nt = int(plan.info.blocks), int(plan.info.tiles)
p16 = np.full((H, W, 4), 0xFFFF, np.uint16); p16[..., :3] = (frame.transpose(1, 2, 0) << 4).astype(np.uint16)
d_pix = torch.from_numpy(p16.astype(">u2").view(np.uint8).reshape(H, W * 8)).to(plan.device)
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


coeff = plan.forward_pixels(_lib.PIX_RGBA64, d_pix)
slots, lens, nbs, rate, dist = plan.encode_blocks(coeff, planes=True)
ctx.sync()
U = int(lens[:n].to(torch.int64).sum().item())
out = dict(layers_entries=have, blocks=n, body_bytes=U)
print("4K RGB 12 bit Mallat closed loop, MQ, %d blocks, %d body bytes; ms, mean / min of %d calls after %d" % (n, U, REP, WARM), flush=True)
cap = plan.frame_bound_layers(8) if have else plan.frame_bound()
cs = plan.empty(cap, torch.uint8); toffs = plan.empty(nt + 1, torch.int64)[:nt + 1]
back = torch.zeros((H, W * 8), dtype=torch.uint8, device=plan.device)
t = timed(lambda: plan.encode_frame_pixels(_lib.PIX_RGBA64, d_pix, False, False, cs, toffs, max_body_bytes=U // 2))
plan.frame_status()
fb = int(toffs[-1].item())
out["encode_rate_ms"] = t
print("encode_frame_pixels(max_body_bytes=U/2)      %8.3f / %-8.3f   (%d bytes)" % (t + (fb,)), flush=True)
t = timed(lambda: plan.decode_frame_pixels(cs, fb, back, toffs, truncated=True))
plan.frame_status()
out["decode_truncated_ms"] = t
print("decode_frame_pixels(truncated=True)          %8.3f / %-8.3f" % t, flush=True)
if have and "--common" not in sys.argv:
    def budgets(L):                                                  # the last layer = U/2, the ones before it halve
        return [U // 2 >> (L - 1 - l) for l in range(L)]
    streams = {}
    for L in (1, 3, 8):
        c2 = plan.empty(cap, torch.uint8)
        res = []
        t = timed(lambda: res.append(plan.encode_frame_pixels(_lib.PIX_RGBA64, d_pix, False, False, c2, toffs, layer_bytes=budgets(L))))
        plan.frame_status()
        streams[L] = (c2, toffs.clone(), int(toffs[-1].item()))
        out["encode_layers_%d_ms" % L] = t
        print("encode_frame_pixels(layer_bytes, L = %d)      %8.3f / %-8.3f   (%d bytes)" % (L, t[0], t[1], streams[L][2]), flush=True)
    assert torch.equal(streams[1][0][:fb], cs[:fb]), "L = 1 is not the max_body_bytes stream"
    for L in (1, 3, 8):
        b = budgets(L)
        one = timed(lambda: plan.rate_allocate_layers(rate, dist, nbs, b))
        many = timed(lambda: [plan.rate_allocate(rate, dist, nbs, x) for x in b])
        out["allocate_%d_ms" % L] = (one, many)
        print("rate_allocate_layers(L = %d) %8.3f / %-8.3f   against %d x rate_allocate %8.3f / %-8.3f" % (L, one[0], one[1], L, many[0], many[1]), flush=True)
    for L in (1, 3, 8):
        c2, to2, fb2 = streams[L]
        for k in sorted({L, 1}, reverse=True):
            t = timed(lambda: plan.decode_frame_pixels(c2, fb2, back, to2, layers=k))
            plan.frame_status()
            g = timed(lambda: plan.decode_tile_parts(c2, fb2, to2, layers=k))
            plan.frame_status()
            out["decode_layers_%d_of_%d_ms" % (k, L)] = (t, g)
            print("decode_frame_pixels(layers=%d) of L = %d       %8.3f / %-8.3f   its decode_tile_parts(layers=%d) alone (packet read + gather, one allocation included) %8.3f / %-8.3f"
                  % (k, L, t[0], t[1], k, g[0], g[1]), flush=True)
    t = timed(lambda: plan.decode_tile_parts(cs, fb, toffs, floors=True))
    plan.frame_status()
    out["decode_tile_parts_floors_ms"] = t
    print("decode_tile_parts(floors=True) of the one-layer stream (the packet read of truncated=True)   %8.3f / %-8.3f" % t, flush=True)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(out, f)
