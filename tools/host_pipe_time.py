"""host_pipe_time.py -- what the pipelined host codec (j2k_pipe_*) adds over the one-call forms, on the frame of bench.py's host boundary:
4K RGB8 (image.RGBA in host memory), 512 x 512 tiles, 5-3 + HT.  Not part of bench.py; one run on one MI355X is one session's numbers.

Workloads: reference-mode encode; closed-loop encode; closed-loop decode.  Configurations, each run RUNS times over FRAMES frames: the one-call
form (j2k_encode_pixels_host / j2k_decode_pixels_host: the baseline, code the library had before the pipe), and the pipe at depth 1, 2, 3 with
pinned (j2k_host_alloc) and with pageable (numpy: what Go's heap is) caller memory.  Every call goes through ctypes on buffers made before the
clock starts, the tables (tile_offs, lens, numbps) asked for everywhere.  Reported per configuration: Gpixel/s (median of the runs, and
their min ... max), GB/s each way, those as a fraction of bench_host.pinned_copy_peak's both-directions rate measured in this process.
After the clock every configuration's last results are compared with the one-call form's (computed before any clock), byte for byte.

    python tools/host_pipe_time.py [--frames 60] [--runs 5] [--out TABLE.md]      # one JSON line per configuration, then the table
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "go-jpeg2000_amd"))

W, H, TILE, NRES, CB = 3840, 2160, 512, 6, 64
RGBA8 = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench_host
    from j2kgfx import CODER_HT, Context
    from j2kgfx.codec import FramePlan, pinned_empty
    if not torch.cuda.is_available():
        raise SystemExit("host_pipe_time.py needs a HIP device")
    torch.cuda.set_device(0)
    peak = bench_host.pinned_copy_peak(torch, "cuda:0")
    ctx = Context(0)
    L = ctx.L
    L.j2k_plan_tile_parts_bound.restype = C.c_size_t
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    frames = [bench_host._rgba_host(np, i) for i in range(3)]
    stride = W * 4
    rows = []

    def alloc(shape, dtype, pinned):
        return pinned_empty(shape, dtype) if pinned else np.zeros(shape, dtype)

    def timed(body):
        """RUNS x body() -> seconds per run; one untimed run first (first-use allocations, the ring)"""
        body()
        out = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            body()
            out.append(time.perf_counter() - t0)
        return out

    def record(workload, config, secs, in_bytes, out_bytes):
        px = [args.frames * W * H / s / 1e9 for s in secs]
        med = statistics.median(px)
        s_med = args.frames * W * H / med / 1e9
        row = dict(workload=workload, config=config, gpix_median=round(med, 3), gpix_min=round(min(px), 3), gpix_max=round(max(px), 3),
                   spread_pct=round(100 * (max(px) - min(px)) / med, 1), h2d_gbs=round(in_bytes / s_med / 1e9, 2), d2h_gbs=round(out_bytes / s_med / 1e9, 2),
                   h2d_of_peak=round(in_bytes / s_med / 1e9 / peak["both_each"], 3), d2h_of_peak=round(out_bytes / s_med / 1e9 / peak["both_each"], 3))
        rows.append(row)
        print(json.dumps(row), flush=True)

    for workload, closed in (("reference-mode encode", False), ("closed-loop encode", True), ("closed-loop decode", True)):
        decode = workload.endswith("decode")
        plan = FramePlan(W, H, 3, precision=8, lossless=True, num_resolutions=NRES, cb=(CB, CB), tile=(TILE, TILE), coder=CODER_HT, ctx=ctx, track_streams=False,
                         closed_loop=closed)
        n, nt = int(plan.info.blocks), int(plan.info.tiles)
        cap = max(plan.frame_bound(), int(L.j2k_plan_tile_parts_bound(plan.h))) + 64
        want = [plan.encode_pixels_host(RGBA8, f) for f in frames]                  # the one-call results (and the decode's input)
        nbytes = [int(w["bytes"].size) for w in want]
        # (the HT block decoder mirrors the reference's, which is no exact inverse: the decode is checked against the one-call form, not the frame)
        want_pix = [plan.decode_pixels_host(w["bytes"], (H, stride)) for w in want] if decode else None

        def buffers(pinned, count):
            b = []
            for k in range(count):
                pix = alloc((H, stride), np.uint8, pinned)
                cs = alloc(cap, np.uint8, pinned)
                if decode:
                    cs[:nbytes[k % 3]] = want[k % 3]["bytes"]
                else:
                    pix[:] = frames[k % 3]
                b.append(dict(pix=pix, cs=cs, toffs=np.zeros(nt + 1, np.uint64), lens=np.zeros(max(n, 1), np.uint32), nb=np.zeros(max(n, 1), np.uint8), src=k % 3))
            return b

        def check(b, olen):
            k = b["src"]
            if decode:
                assert np.array_equal(b["pix"], want_pix[k]), "decoded pixels differ from the one-call form's"
            else:
                assert olen == nbytes[k] and np.array_equal(b["cs"][:olen], want[k]["bytes"]), "tile-parts differ from the one-call form's"
                assert np.array_equal(b["toffs"], want[k]["tile_offs"]) and np.array_equal(b["lens"][:n], want[k]["lens"]) and np.array_equal(b["nb"][:n], want[k]["numbps"])

        in_bytes = args.frames * (sum(nbytes) / 3 if decode else H * stride)
        out_bytes = args.frames * (H * stride if decode else sum(nbytes) / 3)
        # the one-call forms, pageable and pinned caller memory
        for pinned in (False, True):
            bufs = buffers(pinned, 3)
            olen = C.c_size_t(0)

            def one_call():
                for i in range(args.frames):
                    b = bufs[i % 3]
                    if decode:
                        st = L.j2k_decode_pixels_host(plan.h, ptr(b["cs"]), C.c_size_t(nbytes[b["src"]]), 0, 0, ptr(b["pix"]), C.c_size_t(stride))
                    else:
                        st = L.j2k_encode_pixels_host(plan.h, RGBA8, ptr(b["pix"]), C.c_size_t(stride), 0, 0, ptr(b["cs"]), C.c_size_t(cap), C.byref(olen), ptr(b["toffs"]),
                                                      ptr(b["lens"]), ptr(b["nb"]))
                    ctx.check(st)
            secs = timed(one_call)
            check(bufs[(args.frames - 1) % 3], olen.value)
            record(workload, "one-call, %s" % ("pinned" if pinned else "pageable"), secs, in_bytes, out_bytes)
        # the pipe
        for depth in (1, 2, 3):
            for pinned in (True, False):
                bufs = buffers(pinned, depth)
                h = C.c_void_p()
                ctx.check(L.j2k_pipe_create(plan.h, depth, C.byref(h)))
                lens_out = [C.c_size_t(0) for _ in range(depth)]

                def piped():
                    tickets = [0] * depth
                    t = C.c_uint64(0)
                    for i in range(args.frames):
                        k = i % depth
                        if i >= depth:
                            ctx.check(L.j2k_pipe_wait(h, C.c_uint64(tickets[k]), C.byref(lens_out[k])))
                        b = bufs[k]
                        if decode:
                            st = L.j2k_pipe_submit_decode(h, ptr(b["cs"]), C.c_size_t(nbytes[b["src"]]), 0, 0, ptr(b["pix"]), C.c_size_t(stride), C.byref(t))
                        else:
                            st = L.j2k_pipe_submit_encode(h, RGBA8, ptr(b["pix"]), C.c_size_t(stride), 0, 0, ptr(b["cs"]), C.c_size_t(cap), ptr(b["toffs"]), ptr(b["lens"]),
                                                          ptr(b["nb"]), C.byref(t))
                        ctx.check(st)
                        tickets[k] = t.value
                    for i in range(args.frames, args.frames + depth):
                        k = i % depth
                        ctx.check(L.j2k_pipe_wait(h, C.c_uint64(tickets[k]), C.byref(lens_out[k])))
                try:
                    secs = timed(piped)
                    for k in range(depth):
                        check(bufs[k], lens_out[k].value)
                finally:
                    L.j2k_pipe_destroy(h)
                record(workload, "pipe depth %d, %s" % (depth, "pinned" if pinned else "pageable"), secs, in_bytes, out_bytes)
        plan.close()
    ctx.close()
    table = "pinned-copy peak (GB/s): %s; %d frames per run, %d runs\n\n" % (json.dumps(peak), args.frames, args.runs)
    table += "| workload | configuration | Gpixel/s median (min ... max) | spread | H2D GB/s (of peak) | D2H GB/s (of peak) |\n|---|---|---|---|---|---|\n"
    for r in rows:
        table += "| %s | %s | %.2f (%.2f ... %.2f) | %.1f %% | %.2f (%.2f) | %.2f (%.2f) |\n" % (
            r["workload"], r["config"], r["gpix_median"], r["gpix_min"], r["gpix_max"], r["spread_pct"], r["h2d_gbs"], r["h2d_of_peak"], r["d2h_gbs"], r["d2h_of_peak"])
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table)


if __name__ == "__main__":
    main()
