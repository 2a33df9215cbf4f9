"""Writes tests/golden/closed_loop_layers_v1.json: SHA-256 digests of the two layered streams of layer_cases.GOLDEN_CASES as the yardstick composes
them (tests/layer_cases.py: Mallat coefficients and codewords by the oracle, rate tables by shortest_rates, cuts by allocate_layers, packets by
oracle/t2ref.py's PacketEncoder fed per-layer blocks), and where every layer ends.  The layered stream is this library's own format;
the digests pin it.  Run from the repository root: python tests/golden/make_closed_loop_layers_golden.py"""
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
import layer_cases as lc  # noqa: E402


def main():
    out = {}
    for case in lc.GOLDEN_CASES:
        _, _, kept, (stream, toffs, loffs) = lc.golden_stream(case, orc, t2ref)
        out[case["name"]] = dict(bytes=len(stream), head=stream[:24].hex(), sha256=hashlib.sha256(stream).hexdigest(), layers=len(kept),
                                 layer_offs=[int(x) for x in loffs])
    with open(os.path.join(HERE, lc.GOLDEN_FILE), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
