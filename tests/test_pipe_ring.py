"""CPU: the bookkeeping of the pipelined host codec (go-jpeg2000_amd/csrc/pipe_ring.h: ticket -> slot, slot states, which copy may be queued when, the
un-waited limit) has no HIP in it, so tests/pipe_ring_main.cpp -- a stand-alone program with its own main -- drives it with a scripted event oracle,
built with AddressSanitizer + UBSan and run directly.  What it checks is listed at its top."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pipe_ring_state_machine_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pipe_ring_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "pipe_ring_main.cpp"), "-o", exe])
    # 8 depths x 64 seeds x 400 steps: a few thousand interleavings' worth of submits, completions, polls and waits in any order
    out = subprocess.run([exe, "64", "400"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.startswith("pipe_ring ok: 512 interleavings")
    assert int(out.stdout.split()[4]) > 20000            # the waits the interleavings made: the state machine was exercised, not skipped


def test_pipe_ring_header_has_no_hip():
    """the header must stay testable on the CPU: it includes nothing of HIP or of the library"""
    txt = open(os.path.join(ROOT, "go-jpeg2000_amd", "csrc", "pipe_ring.h")).read()
    includes = [l.split()[1] for l in txt.splitlines() if l.startswith("#include")]
    assert includes == ["<cstdint>"]
