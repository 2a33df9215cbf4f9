"""GPU fuzz, third part (dev tool, run on the GPU box): the CLOSED-LOOP mode (j2k_params.closed_loop; this library's, not the
reference's) -- random geometries (tiles down to one sample wide, odd sizes, 1..6 resolutions, 4..64 code-blocks), contents and
precisions, both coders, SOP / EPH on and off.  Every frame: tile-parts == the oracle's composition (tests/closed_loop_ref.oracle_frame:
preprocess, the job list with partitioning windows, the block coder, t2ref.PacketEncoder(len_bits=5) per tile, createTileHeader); parse ->
block decode -> placement == orc.decode_tile_blocks; MQ frames come back bit-exact; tile-part positions given and found by walking the SOTs.
    python tools/fuzz_gpu_closed_loop.py [seconds] [seed] [frames] [--oracle-only]
frames: stop after that many frames (clean ones and ones in the reference's HT panic domain together); the time budget ending first is then
an error (exit status 2) -- what a seeded slice covers does not depend on the machine's speed.
--oracle-only: the same frames (every random draw is made before the modes part), the oracle's side alone -- no torch.cuda, no product
library; one line per frame in both modes: the cell (components, precision, coder), the markers, whether the reference's HT encoder panics.
tests/test_gpu_bench_kernels_direct.py::test_oracle_fuzz_slice runs a seeded slice and states what the seed has to cover."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in ("go-jpeg2000_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p_))
import oracle as orc                                     # noqa: E402
import t2ref                                             # noqa: E402
from closed_loop_ref import oracle_frame                 # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
oracle_only = "--oracle-only" in sys.argv[1:]
if not oracle_only:
    import torch                                         # noqa: E402
    from j2kgfx import J2KError, _lib                    # noqa: E402
    from j2kgfx.codec import FramePlan                   # noqa: E402

budget = float(args[0]) if len(args) > 0 else 120.0
seed = int(args[1]) if len(args) > 1 else 1
want_frames = int(args[2]) if len(args) > 2 else 0
rng = np.random.default_rng(seed)
t0 = time.time()
n = npanic = npar_tiles = nser_tiles = nframe_enc = 0
t_say = t0
while time.time() - t0 < budget and not (want_frames and n + npanic >= want_frames):
    if time.time() - t_say > 60:
        t_say = time.time(); print("... %d frames, %.0f s" % (n, t_say - t0), flush=True)
    Cn = int(rng.choice([1, 3, 3, 4]))
    tw = int(rng.choice([1, 2, 3, 5, 16, 32, 64, 100, 128, 256]))
    th = int(rng.choice([1, 2, 7, 16, 33, 64, 128]))
    W = int(rng.choice([tw, tw + 1, 2 * tw, 2 * tw + 3, 3 * tw - 1, 37, 100, 264]))
    H = int(rng.choice([th, th + 3, 2 * th - 1, 5, 33, 64, 130]))
    if W < 1 or H < 1 or W * H * Cn > 120000 or ((W + tw - 1) // tw) * ((H + th - 1) // th) > 400:
        continue
    nres = int(rng.integers(1, 7))
    cb = int(rng.choice([4, 8, 16, 32, 64]))
    coder = int(rng.integers(0, 2))
    prec = int(rng.choice([8, 12, 16]))
    sop, eph = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    if rng.integers(0, 3) == 0:
        sop = eph = True                                        # (about half the frames: SOP + EPH, the packets of a tile parsed side by side)
    top = (1 << prec) - 1
    kind = int(rng.integers(0, 4))
    if kind == 0:
        frame = rng.integers(0, top + 1, (Cn, H, W))
    elif kind == 1:
        yy, xx = np.mgrid[0:H, 0:W]
        frame = np.clip(np.stack([(xx * top // max(W, 1) + yy + c * 5) for c in range(Cn)]) + rng.integers(-3, 4, (Cn, H, W)), 0, top)
    elif kind == 2:
        frame = (top // 3) + rng.integers(-1, 2, (Cn, H, W))
    else:
        frame = np.full((Cn, H, W), top // 2)                    # flat: all-zero bands, empty packets
        frame[:, rng.integers(0, H), rng.integers(0, W)] = top
    frame = frame.astype(np.int32)
    desc = (Cn, W, H, tw, th, nres, cb, coder, prec, kind, sop, eph)
    # ---- every draw is made: the oracle's side (both modes) -------------------------------------------------------------------------
    tiles_x = (W + tw - 1) // tw
    ntiles = tiles_x * ((H + th - 1) // th)
    try:
        want = oracle_frame(frame, W, H, tw, th, nres, cb, coder, sop, eph, orc, t2ref, precision=prec)
        panics = False
    except ValueError:
        want, panics = None, True                               # the reference's HT encoder panics on this input
    print("frame %d: components=%d precision=%d coder=%s sop=%d eph=%d %s" % (n + npanic, Cn, prec, "HT" if coder == 1 else "MQ", sop, eph, "panic" if panics else "ok"), flush=True)
    ref = None if panics else [(want[tl]["x0"], want[tl]["y0"], want[tl]["w"], want[tl]["h"], want[tl]["bytes"], want[tl]["lens"], want[tl]["numbps"]) for tl in range(ntiles)]
    if oracle_only:
        if panics:
            npanic += 1
            continue
        for (x0, y0, w, h, by, ln, nb) in ref:
            orc.decode_tile_blocks(by, ln, nb, Cn, w, h, nres, cb, cb, coder, 1)
        n += 1
        continue
    # ---- the product ------------------------------------------------------------------------------------------------------------------
    plan = FramePlan(W, H, Cn, precision=prec, lossless=True, num_resolutions=nres, cb=(cb, cb), tile=(tw, th), coder=coder, closed_loop=True)
    d = torch.from_numpy(frame).to(plan.device)
    coeff = plan.forward(d)
    try:
        stream, offs, lens, numbps = plan.encode_stream(coeff)
        plan.ctx.sync()
    except J2KError as e:
        assert e.status == -5 and coder == 1, desc               # the reference's HT encoder panics on this input ...
        assert panics, ("the product reports a panic where the oracle does not", desc)
        npanic += 1
        plan.close()
        continue
    assert not panics, ("oracle panics where the product did not", desc)
    cs, toffs = plan.encode_tile_parts(stream, offs, lens, numbps, sop=sop, eph=eph)
    plan.frame_status()
    h_cs, h_t = cs.cpu().numpy(), toffs.cpu().numpy()
    total = int(h_t[-1])
    planes = plan.planes()
    nres_jobs = nres
    for tl in range(ntiles):
        assert bytes(h_cs[int(h_t[tl]):int(h_t[tl + 1])]) == want[tl]["part"], ("tile-part", desc, tl)
    if Cn == 3 and prec == 8:
        # the one-call frame encoder (blocks gathered from their coding slots straight into the tile-parts) == the stage calls
        pix = np.full((H, W, 4), 255, np.uint8)
        pix[..., :3] = frame.transpose(1, 2, 0)
        cs_f, toffs_f = plan.encode_frame_pixels(_lib.PIX_RGBA8, torch.from_numpy(pix.reshape(H, W * 4)).to(plan.device), sop=sop, eph=eph)
        plan.frame_status()
        assert np.array_equal(toffs_f.cpu().numpy(), h_t) and np.array_equal(cs_f.cpu().numpy()[:total], h_cs[:total]), ("frame encoder", desc)
        nframe_enc += 1
    for given in (True, False):
        plan.frame_parallel_tiles()
        offs2, lens2, nb2 = plan.decode_tile_parts(cs, total, tile_offs=toffs if given else None, sop=sop, eph=eph)
        decoded = plan.decode_blocks(cs, offs2, lens2, nb2)
        placed = plan.place_blocks(decoded)
        back = plan.inverse(placed)
        try:
            plan.frame_status()
        except J2KError as e:
            raise AssertionError(("decode status", e.status, desc, given, total, [int(x) for x in h_t[:6]]))
        par = plan.frame_parallel_tiles()
        npar_tiles += par
        nser_tiles += ntiles - par if (sop and eph) else 0
        assert par == 0 or (sop and eph), desc
        hp, hb = placed.cpu().numpy(), back.cpu().numpy().reshape(Cn, H, W)
        for tl, (x0, y0, w, h, by, ln, nb) in enumerate(ref):
            want_p = orc.decode_tile_blocks(by, ln, nb, Cn, w, h, nres_jobs, cb, cb, coder, 1)
            for c in range(Cn):
                row = planes[tl * Cn + c]
                got = hp[int(row[6]):int(row[6]) + w * h].reshape(h, w)
                assert np.array_equal(got, want_p[c]), ("placed", desc, tl, c, given)
        if coder == 0:
            assert np.array_equal(hb, frame), ("round trip", desc, given)
        if Cn == 3 and prec == 8 and given:
            # the one-call frame decoder (HT: coded rows straight into the planes' windows, planes zeroed once) == the stage calls, frame after frame
            want_px = plan.inverse_pixels(placed, torch.zeros(H, W * 4, dtype=torch.uint8, device=plan.device))
            got_px = torch.zeros_like(want_px)
            for _ in range(2):
                plan.decode_frame_pixels(cs, total, got_px, tile_offs=toffs, sop=sop, eph=eph)
                plan.frame_status()
                assert torch.equal(got_px, want_px), ("frame decoder", desc)
    plan.close()
    n += 1
if want_frames and n + npanic < want_frames:
    print("closed-loop fuzz: the time budget of %.0f s ended after %d of %d frames, seed %d" % (budget, n + npanic, want_frames, seed))
    sys.exit(2)
if oracle_only:
    print("closed-loop fuzz, the oracle's side alone: %d frames (%d in the reference's HT panic domain) in %.1f s, seed %d" % (n + npanic, npanic, time.time() - t0, seed))
    sys.exit(0)
print("closed-loop fuzz: %d frames clean (%d in the reference's HT panic domain; SOP + EPH frames: %d tiles parsed packet-parallel, %d fell back to the tile chain; %d frames also through the one-call frame encoder) in %.0f s, seed %d"
      % (n, npanic, npar_tiles, nser_tiles, nframe_enc, time.time() - t0, seed))
