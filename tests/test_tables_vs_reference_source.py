"""CPU: the numeric tables the oracle and the kernels carry are compared with the reference's source text through
fingerprints recorded from it: the sha256 of each table as the reference states it (mqc.go's mqStates rows as little-endian
uint32 (Qe, MPS, NMPS, NLPS); ht_luts.go's vlcTbl0 / vlcTbl1 as 1024 little-endian uint16, zero-padded) and the positions of the
context constants in mqc.go's declaration.  Nothing outside the repository is read."""
import hashlib
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# recorded from the reference's internal/entropy/mqc.go and ht_luts.go
MQ_STATES_SHA256 = "af7f2991749d540f7111e96a4516f41ac7e9c11cab9ce4c6281a59dd34e728a6"
VLC_TBL_SHA256 = {"J2K_HT_VLC_TBL0": "018c57541fdaf582791c3e61bb4e8defa6d830aa2b309d8b5616de09f27539cb",
                  "J2K_HT_VLC_TBL1": "00915bca44a0267ade790e2396aee69e11af50f3db3397c546371c6762311457"}
# mqc.go's const block: CtxZC0..CtxZC8, CtxSC0..CtxSC4, CtxMag0..CtxMag2, CtxRL, CtxUni, NumContexts
REF_CONTEXTS = {"CtxSC0": 9, "CtxMag0": 14, "CtxMag1": 15, "CtxMag2": 16, "CtxRL": 17, "CtxUni": 18, "NumContexts": 19}


def test_mq_state_table(oracle):
    qe, nm, nl = oracle.mq_table()
    assert len(qe) == 94
    rows = np.stack([qe.astype("<u4"), (np.arange(94) & 1).astype("<u4"), nm.astype("<u4"), nl.astype("<u4")], 1)
    assert hashlib.sha256(np.ascontiguousarray(rows).tobytes()).hexdigest() == MQ_STATES_SHA256


def test_ht_tables_match_generated_headers():
    for hdr in ("oracle/ht_tables.h", "go-jpeg2000_amd/csrc/ht_tables.h"):
        h = open(os.path.join(ROOT, hdr)).read()
        for macro, want in VLC_TBL_SHA256.items():
            got = [int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]{4}", re.search(r"#define %s_INIT \{(.*?)\n\}" % macro, h, re.S).group(1))]
            assert len(got) == 1024, (hdr, macro)
            assert hashlib.sha256(np.array(got, "<u2").tobytes()).hexdigest() == want, (hdr, macro)


def test_context_constants():
    for src in ("oracle/j2k_oracle.c", "go-jpeg2000_amd/csrc/t1.hip"):
        txt = open(os.path.join(ROOT, src)).read()
        enum = dict((k, int(v)) for k, v in re.findall(r"\b(Ctx[A-Za-z0-9]+|NumContexts)\s*=\s*(\d+)", txt))
        for name, idx in REF_CONTEXTS.items():
            assert enum.get(name) == idx, (src, name)
