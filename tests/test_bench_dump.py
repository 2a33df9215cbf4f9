"""bench.py's plain run and --dump-outputs: the run times exactly --steps steps, prints ONE line without the --full records, and writes
what the last timed step computed (float32 / float64 arrays, 64 MB at most); every frame in flight gives back the seeded input frame
(whole-array checksums of the pixels equal those of the input)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _checksum(x):
    """bench.dump_outputs' row: count, int64 sum and position-weighted sum, each as (high, low) 32-bit halves"""
    x = np.asarray(x).reshape(-1).astype(np.int64)
    w = np.arange(x.size, dtype=np.int64) % 65521 + 1
    row = [float(x.size)]
    for v in (int(x.sum()), int((x * w).sum())):
        v &= 0xFFFFFFFFFFFFFFFF
        row += [float(v >> 32), float(v & 0xFFFFFFFF)]
    return np.array(row)


def test_dump_outputs_refused_outside_the_headline(tmp_path):
    out = subprocess.run([sys.executable, BENCH, "--config", "c3", "--dump-outputs", str(tmp_path)], env=_env(),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--dump-outputs is implemented for the C2 headline run" in out.stderr
    assert not os.listdir(tmp_path)


@pytest.mark.gpu
def test_plain_run_times_steps_and_dumps_the_last_step(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                         env=_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["higher_is_better"] is True and d["unit"] == "Mpixels/s" and d["dtype"] == "int32"
    assert d["roofline"] is None and "cpu_baseline" not in d and "other_configs" not in d and d["config"]["full"] is False
    F = d["config"]["frames_in_flight"]
    n = d["config"]["code_blocks"]
    names = ("checksums", "decoded", "lengths", "numbps", "offsets", "pixels", "stream")
    assert sorted(os.listdir(tmp_path)) == sorted("frame%d_%s.npy" % (f, k) for f in range(min(F, 8)) for k in names)
    total = 0
    for fn in os.listdir(tmp_path):
        a = np.load(os.path.join(tmp_path, fn))
        assert a.dtype in (np.float32, np.float64), fn
        total += a.nbytes
    assert total <= 64 << 20
    frame = bench.synth_frame(np, 0)
    rgba = np.concatenate([frame.transpose(1, 2, 0), np.full((bench.H, bench.W, 1), 255, np.int32)], axis=2).astype(np.uint8)
    want_pix = _checksum(rgba)
    first = {k: np.load(os.path.join(tmp_path, "frame0_%s.npy" % k)) for k in names}
    assert first["offsets"].shape == (n + 1,) and first["lengths"].shape == (n,) and first["numbps"].shape == (n,)
    assert first["offsets"][-1] == d["config"]["compressed_bytes_per_frame"] == first["checksums"][0][0]
    for f in range(min(F, 8)):
        cs = np.load(os.path.join(tmp_path, "frame%d_checksums.npy" % f))
        assert np.array_equal(cs[2], want_pix), "frame %d: pixels back differ from the input" % f
        for k in names:                               # the frames in flight code the same input
            assert np.array_equal(np.load(os.path.join(tmp_path, "frame%d_%s.npy" % (f, k))), first[k]), (f, k)
