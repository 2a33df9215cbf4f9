"""Writes tests/golden/closed_loop_mallat_v1.json: SHA-256 digests of the tile-parts of the two frames of mallat_cases.GOLDEN_CASES, composed by the
oracle (tests/mallat_cases.py: the Mallat coefficients through the block coder and the packet loop of closed_loop_ref.oracle_frame).  The
Mallat closed loop is this library's own stream format; the digests pin it.  Run from the repository root: python tests/golden/make_closed_loop_mallat_golden.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import oracle as orc  # noqa: E402
import t2ref  # noqa: E402
import mallat_cases as mc  # noqa: E402


def main():
    out = {}
    for case in mc.GOLDEN_CASES:
        _, _, stream = mc.golden_stream(case, orc, t2ref)
        out[case["name"]] = dict(bytes=len(stream), head=stream[:24].hex(), sha256=hashlib.sha256(stream).hexdigest())
    with open(os.path.join(HERE, mc.GOLDEN_FILE), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
