"""CPU: the plan's table builder (go-jpeg2000_amd/csrc/plan_tables.h, plan_tables.cpp) has no HIP in it, so tests/plan_tables_main.cpp -- a
stand-alone program with its own main -- runs it over a fixed matrix of geometries and option settings, built with AddressSanitizer + UBSan and run
directly.  Every table it makes (element size, count, FNV-1a 64 of the bytes) and every scalar it derives must equal tests/plan_tables_recorded.json,
which was recorded from build_plan / plan_reduced as they were while the tables were still built between the uploads (docs/HISTORY.md says how): a
digest that differs is a wrong table, not a stale recording.  The program also checks the invariants listed at its top and fails on a violation.

The recording keeps a run with an option set (`case+option=value`) as its difference from the case's default run."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-jpeg2000_amd", "csrc")
RECORDED = os.path.join(ROOT, "tests", "plan_tables_recorded.json")
TABLE = re.compile(r"^\d+:(\d+):(-|[0-9a-f]{16})$")
# the per-level and per-`reduce` tables, whatever the level: each must occur somewhere (the others have fixed names and are printed even when empty)
LEVEL_TABLES = (["%s[%d][*].%s" % (d, c, t) for d in ("fwd", "inv") for c in (0, 1) for t in ("planes", "jobs", "pjobs")]
                + ["reduce[*].inv[%d].%s" % (c, t) for c in (0, 1) for t in ("planes", "jobs")]
                + ["reduce[*].%s" % t for t in ("ll", "ids", "bjobs", "djobs", "placed")])


def parse(text):
    """the program's output -> {run: {name: value}}, in the program's order"""
    runs, cur = {}, None
    for line in text.splitlines():
        if line.startswith("@ "):
            cur = runs.setdefault(line[2:], {})
            continue
        name, value = line.split(" ", 1)
        assert name not in cur, (name, "printed twice")
        cur[name] = value
    return runs


def compact(runs):
    """option runs as their difference from the default run of their case (None: the name is gone)"""
    out = {}
    for run, vals in runs.items():
        if "+" not in run:
            out[run] = vals
            continue
        base = runs[run.split("+")[0]]
        out[run] = {k: vals.get(k) for k in list(vals) + list(base) if vals.get(k) != base.get(k)}
    return out


def expand(rec):
    out = {}
    for run, vals in rec.items():
        if "+" in run:
            full = dict(rec[run.split("+")[0]])
            full.update(vals)
            vals = {k: v for k, v in full.items() if v is not None}
        out[run] = vals
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(RECORDED) as f:
        return json.load(f)


def test_plan_tables_equal_the_recording_under_sanitizers(tmp_path, recorded):
    exe = str(tmp_path / "plan_tables_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "plan_tables_main.cpp"), os.path.join(CSRC, "plan_tables.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]      # sanitizer reports and invariant violations
    got = compact(parse(out.stdout))
    assert list(got) == list(recorded), "the matrix itself changed"
    wrong = ["%s: %s = %s, recorded %s" % (run, k, got[run].get(k), recorded[run].get(k))
             for run in recorded for k in sorted(set(got[run]) | set(recorded[run])) if got[run].get(k) != recorded[run].get(k)]
    assert not wrong, "%d values differ from the recording:\n%s" % (len(wrong), "\n".join(wrong[:40]))


def test_matrix_fills_every_table_somewhere(recorded):
    filled, names = set(), set(LEVEL_TABLES)
    for vals in expand(recorded).values():
        for k, v in vals.items():
            m = TABLE.match(v)
            if not m:
                continue
            k = re.sub(r"^(fwd|inv)\[(\d)\]\[\d+\]", r"\1[\2][*]", re.sub(r"^reduce\[\d+\]", "reduce[*]", k))
            names.add(k)
            if int(m.group(1)) > 0:
                filled.add(k)
    assert len(names) > 50
    assert sorted(names - filled) == []


def test_every_option_value_changes_a_table(recorded):
    """... in at least one of the cases it is swept over (the 9-7 options only shape the lossy case, the Mallat instantiations only the Mallat one)"""
    changes = {}
    for run, vals in recorded.items():
        if "+" in run:
            changes.setdefault(run.split("+", 1)[1], []).append(len(vals))
    assert len(changes) >= 50
    assert sorted(o for o, n in changes.items() if not any(n)) == []


def test_builder_sources_have_no_hip():
    """the builder and the headers it needs must stay testable on the CPU"""
    for name, allowed in (("j2k_tables.h", ["<stddef.h>", "<stdint.h>"]),
                          ("plan_tables.h", ["<cstddef>", "<cstdint>", "<vector>", '"../../include/j2kgfx.h"', '"j2k_tables.h"', '"j2k_plan.h"']),      # (its HIP-free first part)
                          ("plan_tables.cpp", ['"plan_tables.h"', "<algorithm>", "<map>", "<tuple>"])):
        txt = open(os.path.join(CSRC, name)).read()
        assert [l.split()[1] for l in txt.splitlines() if l.startswith("#include")] == allowed
