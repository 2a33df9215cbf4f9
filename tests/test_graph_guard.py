"""CPU: the lifetime bookkeeping of captured graphs (go-jpeg2000_amd/csrc/graph_guard.h: which staging slots and plans a capture used, the
generations j2k_graph_launch compares, the plan serials) has no HIP in it, so tests/graph_guard_main.cpp -- a stand-alone program with its
own main -- drives it through scripted histories and prints a verdict per check.  The expected verdicts are the table below, written out
by hand from the rule (include/j2kgfx.h, "LIFETIME"), not taken from the program.  Built and run twice: plain, and with AddressSanitizer +
UBSan.  Also: every plan entry point of the C ABI notes its plan, read off the sources."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-jpeg2000_amd", "csrc")

# "<history>.<check>" -> verdict.  stale_a:<slot>, stale_b:<plan serial>, stale_c:<plan serial>
EXPECTED = [
    # a capture that reserved slots 0 and 2 (slot 0 twice, neither grew): both are noted -- bits 0 and 2
    ("slots.noted", "5"),
    ("slots.fresh", "valid"),
    ("slots.grow1", "valid"),                  # growth of a slot the capture did not use
    ("slots.grow34", "valid"),
    ("slots.grow2", "stale_a:2"),              # growth of one it used
    ("slots.grow0", "stale_a:0"),
    # what is reserved or called outside a capture is not noted; the capture used slot 3 only and no plan
    ("idle.noted", "8 0"),
    ("idle.after", "valid"),                   # slot 1 grew, plan A grew and was destroyed: none of them recorded
    ("idle.second", "0 0"),                    # a capture starts from nothing
    # plans A (serial 1) and B (2), a graph each on slot 0
    ("plans.serials", "1 2"),
    ("plans.noted", "1 1"),                    # a plan called twice is noted once
    ("plans.A0", "valid"), ("plans.B0", "valid"),
    ("plans.A1", "valid"), ("plans.B1", "stale_b:2"),          # B grows its own buffer
    ("plans.A2", "stale_c:1"), ("plans.B2", "stale_b:2"),      # A is destroyed: B's graph is what it was
    ("plans.reborn", "3"),                     # a new plan (at A's address or not) has a new serial ...
    ("plans.A3", "stale_c:1"),                 # ... so A's old graph stays refused
    ("plans.A2graph", "valid"), ("plans.A4", "stale_c:1"),     # the new plan's own graph is valid, the old one still is not
    ("plans.Bnew", "valid"), ("plans.Bold", "stale_b:2"),      # stale, captured again: new valid, old stale
    ("plans.X1", "stale_b:2"),                 # a graph over B and the new plan: B grows
    ("plans.X2", "stale_c:3"),                 # the new plan is destroyed too: (c) outranks (b)
    ("plans.Bnew2", "stale_b:2"),              # B's second graph was taken before that growth
    ("plans.Bnewest", "valid"),                # a serial the table does not hold (another context's plan, a plan destroyed twice) changes nothing
    ("plans.A2graph2", "stale_c:3"),
    ("both.ab", "stale_a:4"),                  # a slot and a plan buffer: (a) is named
    # 64-bit counters compared for equality: a snapshot at 2^64 - 1, one bump wraps both to 0 -> stale; 2^k more bumps, k = 0 ... 63: stale every
    # time (64 of 64, slot and plan); only exactly 2^64 bumps read as valid again
    ("wrap.fresh", "valid"),
    ("wrap.gens", "0 0"),
    ("wrap.one", "stale_a:2"),
    ("wrap.pow2", "64 64"),
    ("wrap.back", "valid"),
    ("wrap.width", "64 64"),
]


def build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "graph_guard_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return [tuple(l.split(" ", 1)) for l in out.stdout.splitlines()]


def test_graph_guard_histories(tmp_path):
    assert build_and_run(tmp_path, "graph_guard_main", []) == EXPECTED


def test_graph_guard_histories_under_sanitizers(tmp_path):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + flags, input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no AddressSanitizer / UBSan runtime")
    assert build_and_run(tmp_path, "graph_guard_main_asan", flags) == EXPECTED


def test_graph_guard_header_has_no_hip():
    """the header must stay testable on the CPU: it includes nothing of HIP or of the library"""
    txt = open(os.path.join(CSRC, "graph_guard.h")).read()
    includes = [l.split()[1] for l in txt.splitlines() if l.startswith("#include")]
    assert includes == ["<cstdint>", "<map>", "<utility>", "<vector>"]


def entry_points():
    """(file, name, const plan?, first statement) of every extern "C" function whose first parameter is a plan"""
    out = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.cpp"))):
        txt = open(path).read()
        for m in re.finditer(r'^extern "C" [^\n(]*?\b(j2k_\w+)\((const )?j2k_plan \*(\w+)[,)]', txt, flags=re.M):
            body = txt[txt.index("{", m.end() - 1) + 1:]
            first = body.split(";", 1)[0].strip()
            out.append((os.path.basename(path), m.group(1), bool(m.group(2)), first))
    return out


def test_every_plan_entry_point_notes_its_plan():
    """No call family reaches a launch around the plan note: every C ABI function that takes a non-const plan has graph_note_plan(P) as its
    first statement (j2k_plan_destroy has the tombstone in its place); the ones that take a const plan are queries, and none of them launches."""
    eps = entry_points()
    assert len(eps) >= 100
    noting = [e for e in eps if not e[2]]
    assert len(noting) >= 80
    for f, name, _, first in noting:
        if name == "j2k_plan_destroy":
            continue
        assert first == "graph_note_plan(P)", "%s: %s starts with %r" % (f, name, first)
    destroy = open(os.path.join(CSRC, "j2k_planbuild.cpp")).read().split('extern "C" void j2k_plan_destroy', 1)[1].split("\n}\n", 1)[0]
    assert destroy.index("guard.plan_destroyed(P->serial)") < destroy.index("hipFree")
    # a const plan launches nothing: no stream in the body of such a function
    for path in sorted(glob.glob(os.path.join(CSRC, "*.cpp"))):
        txt = open(path).read()
        for m in re.finditer(r'^extern "C" [^\n(]*?\b(j2k_\w+)\(const j2k_plan \*', txt, flags=re.M):
            body = txt[m.end():].split("\n}\n", 1)[0]
            assert "->stream" not in body and "stage_reserve" not in body, m.group(1)


def test_every_reallocation_bumps_a_generation():
    """the two free-and-reallocate sites that a recorded launch can reach bump their generation BEFORE the hipFree"""
    ctx = open(os.path.join(CSRC, "j2k_ctx.cpp")).read().split("int stage_reserve(", 1)[1]
    assert ctx.index("guard.slot_used(slot)") < ctx.index("return J2K_OK")           # noted also when the slot is big enough
    assert ctx.index("guard.slot_reallocated(slot)") < ctx.index("hipFree(")
    host = open(os.path.join(CSRC, "j2k_hostcalls.cpp")).read().split("int ensure_sized(", 1)[1].split("\n}\n", 1)[0]
    assert host.index("guard.plan_buffer_reallocated(P->serial)") < host.index("hipFree(")
