"""Writes tests/golden/closed_loop_raw_magref_v1.json: SHA-256 and length of the closed-loop tile-parts, in the raw-MagRef coding style
(j2k_plan_set_raw_magref), of the frames tests/raw_magref_cases.GOLDEN_FRAMES names, as the DEFINITION composes them (pyref's T1 with the MagRef
contexts diverted, the oracle's raw coder and packet layer).  The style is this library's own body format: the digests pin it --
a change of the format has to change this file on purpose.
    python tests/golden/make_raw_magref_golden.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import oracle as orc              # noqa: E402
import t2ref                      # noqa: E402
import raw_magref_cases as rm     # noqa: E402

out = {}
for name in rm.GOLDEN_FRAMES:
    sop, eph = rm.GOLDEN_FLAGS[name]
    s = rm.frame_stream(name, sop, eph, orc, t2ref)
    out[name] = {"sop": sop, "eph": eph, "bytes": len(s), "sha256": hashlib.sha256(s).hexdigest()}
json.dump(out, open(os.path.join(HERE, rm.GOLDEN_FILE), "w"), indent=1, sort_keys=True)
print(json.dumps(out, indent=1, sort_keys=True))
