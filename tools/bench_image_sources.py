"""Timing of the image.YCbCr source (encoder.go:178-195) on the 4K frame (3840x2160, 512x512 tiles, 5-3, HT), one device:
  j2k_plan_forward_image for 4:2:0, fused (the level-0 kernel reads the planes) and staged (pix_fuse = 0: through an RGBA8 frame),
  against j2k_plan_forward_pixels(RGBA8) of the same colours; j2k_encode_image_host against j2k_encode_pixels_host(RGBA8) from pinned
  memory.  Prints the H2D bytes of each.  Kernel times: run it under rocprofv3 --kernel-trace --stats (profiles/).
  python tools/bench_image_sources.py [--reps N]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-jpeg2000_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import go_image_ref as ref                  # noqa: E402
from j2kgfx import _lib                     # noqa: E402
from j2kgfx.codec import FramePlan          # noqa: E402
from j2kgfx.context import Context          # noqa: E402
from j2kgfx.pixels import YCbCr             # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 50
W, H = 3840, 2160
rng = np.random.default_rng(1)
yy, xx = np.mgrid[0:H, 0:W]
Y = np.clip((xx * 255 // W + yy * 64 // H) + rng.integers(-8, 9, (H, W)), 0, 255).astype(np.uint8)
cyy, cxx = np.mgrid[0:H // 2, 0:W // 2]
Cb = np.clip(96 + cxx * 64 // (W // 2) + rng.integers(-8, 9, cxx.shape), 0, 255).astype(np.uint8)
Cr = np.clip(160 - cyy * 64 // (H // 2) + rng.integers(-8, 9, cyy.shape), 0, 255).astype(np.uint8)
y, cb, cr = (torch.from_numpy(a.reshape(-1)).pin_memory() for a in (Y, Cb, Cr))
rgba = torch.from_numpy(ref.rgba8_frame(ref.ycbcr_image_rgb(Y.reshape(-1), Cb.reshape(-1), Cr.reshape(-1), W, W // 2, 2, (0, 0, W, H)))).pin_memory()
h2d_img, h2d_rgba = Y.nbytes + Cb.nbytes + Cr.nbytes, rgba.numel()


def dev_time(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(torch.cuda.ExternalStream(plan.ctx.stream))
    for _ in range(reps):
        fn()
    e1.record(torch.cuda.ExternalStream(plan.ctx.stream))
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


for pix_fuse in (1, 0):
    ctx = Context(0)
    ctx.set_option("pix_fuse", pix_fuse)
    plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=6, cb=(64, 64), tile=(512, 512), coder=1, ctx=ctx, track_streams=False)
    dimg = YCbCr(y.cuda(), cb.cuda(), cr.cuda(), W, W // 2, 2, (0, 0, W, H))
    drgba = rgba.cuda()
    coeff = plan.alloc_coeff()
    torch.cuda.synchronize()
    fused = plan.image_fused(dimg)
    t_img = dev_time(lambda: plan.forward_image(dimg, coeff))
    t_pix = dev_time(lambda: plan.forward_pixels(_lib.PIX_RGBA8, drgba, coeff))
    print("pix_fuse=%d: j2k_plan_forward_image 4:2:0 (%s) %.3f ms, j2k_plan_forward_pixels RGBA8 %.3f ms per 4K frame"
          % (pix_fuse, "fused" if fused else "staged", t_img, t_pix), flush=True)
    if pix_fuse == 1:
        himg = YCbCr(y.numpy(), cb.numpy(), cr.numpy(), W, W // 2, 2, (0, 0, W, H))
        hrgba = rgba.numpy()
        for label, call, nbytes in (("j2k_encode_image_host 4:2:0", lambda: plan.encode_image_host(himg), h2d_img),
                                    ("j2k_encode_pixels_host RGBA8", lambda: plan.encode_pixels_host(_lib.PIX_RGBA8, hrgba), h2d_rgba)):
            out = call()
            t0 = time.perf_counter()
            for _ in range(max(reps // 5, 3)):
                out = call()
            dt = (time.perf_counter() - t0) / max(reps // 5, 3)
            print("%s from pinned memory: %.2f ms per 4K frame, H2D %.1f MB, %d bytes out" % (label, dt * 1e3, nbytes / 1e6, out["bytes"].size), flush=True)
        a, b = plan.encode_image_host(himg), plan.encode_pixels_host(_lib.PIX_RGBA8, hrgba)
        assert np.array_equal(a["bytes"], b["bytes"]), "image and RGBA8 encodes differ"
        print("encode_image_host bytes == encode_pixels_host(RGBA8) bytes", flush=True)
    plan.close()
    ctx.close()
