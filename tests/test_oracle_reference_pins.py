"""CPU: every NUMERIC vector the reference's own unit tests hold below round-trip level, reproduced by the C oracle
(oracle/j2k_oracle.c, "pins" section) and -- where it has the function -- by the independent Python restatement
(oracle/pyref.py).  Source of each vector: internal/entropy/coverage_test.go, t1_test.go, mqc_test.go, ht_test.go and
internal/mct/mct_test.go of mrjoshuak/go-jpeg2000; the vectors are data (inputs + expected outputs), retyped here as Python literals.

VERDICT r1 "missing #4": TestMqByteOutLocal, TestGetSignContextParams, TestT1_GetMRContext(_Detailed),
TestLutSCCtx/LutSignCtx/LutSC_Values, TestMQEncoder_ByteOut_*, TestT1_CanUseRunLength, ht_test.go:126-147.
"""
import ctypes as C

import numpy as np
import pytest

T1Sig, T1Visit, T1Refine, T1SignNeg, T1SigN, T1SigS, T1SigE, T1SigW = 1, 2, 4, 8, 16, 32, 64, 128   # t1.go:74-91
CtxZC0, CtxSC0, CtxSC4, CtxMag0, CtxMag1, CtxMag2, CtxRL, CtxUni = 0, 9, 13, 14, 15, 16, 17, 18        # mqc.go:135-166


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


class Flags:
    """NewT1(w, h).flags with setFlag / updateNeighborFlags (t1.go:94-122, 307-345)."""

    def __init__(self, lib, w, h):
        self.lib, self.w, self.h = lib, w, h
        self.f = np.zeros((h + 2) * (w + 2), np.uint8)

    def clear(self):
        self.f[:] = 0

    def set(self, x, y, flag):
        self.f[(y + 1) * (self.w + 2) + x + 1] |= flag

    def has(self, x, y, flag):
        return bool(self.f[(y + 1) * (self.w + 2) + x + 1] & flag)

    def call(self, name, x, y, *extra):
        return getattr(self.lib, name)(_u8p(self.f), self.w, self.h, x, y, *extra)


@pytest.fixture(scope="module")
def lib(oracle):
    return oracle.lib()


# ---- coverage_test.go:904-959 TestMqByteOutLocal (4 vectors: expected bp and CT) + the byte/C it implies -----------
@pytest.mark.parametrize("name,buf,c,exp_bp,exp_ct,exp_buf,exp_c", [
    ("normal byte", [0x00, 0, 0], 0x100000, 1, 8, [0x00, 0x02, 0], 0x100000 & 0x7FFFF),
    ("0xFF byte", [0xFF, 0, 0], 0x100000, 1, 7, [0xFF, 0x01, 0], 0x100000 & 0xFFFFF),
    ("carry bit set", [0x00, 0, 0], 0x8000000, 1, 8, [0x01, 0x00, 0], 0),
    ("carry causes 0xFF", [0xFE, 0, 0], 0x8000000, 1, 7, [0xFF, 0x00, 0], 0),
])
def test_mq_byte_out_local(lib, name, buf, c, exp_bp, exp_ct, exp_buf, exp_c):
    b = np.array(buf, np.uint8)
    bp, cc, ct = C.c_long(), C.c_uint32(), C.c_uint32()
    lib.orc_pin_mq_byte_out(_u8p(b), C.c_size_t(b.size), C.c_long(0), C.c_uint32(c), C.byref(bp), C.byref(cc), C.byref(ct))
    assert (bp.value, ct.value) == (exp_bp, exp_ct), name            # what the reference test asserts
    assert b.tolist() == exp_buf and cc.value == exp_c, name         # what t1_fast.go:11-34 implies beyond that


# ---- coverage_test.go:354-378 TestMqByteOutRare, :335-352 TestMqByteOutCommon, :309-333 TestMqNeedsSlowPath ----------
@pytest.mark.parametrize("buf0,c,exp_ct", [(0xFF, 0xFFFFF, 7), (0xFE, 0x8000000, 7), (0x00, 0x8000000, 8)])
def test_mq_byte_out_rare(lib, buf0, c, exp_ct):
    b = np.zeros(10, np.uint8); b[0] = buf0
    bp, cc, ct = C.c_long(), C.c_uint32(), C.c_uint32()
    lib.orc_pin_mq_byte_out(_u8p(b), C.c_size_t(b.size), C.c_long(0), C.c_uint32(c), C.byref(bp), C.byref(cc), C.byref(ct))
    assert ct.value == exp_ct


def test_mq_byte_out_common(lib):
    b = np.zeros(10, np.uint8)
    c = 0x7FFFF80
    bp, cc, ct = C.c_long(), C.c_uint32(), C.c_uint32()
    lib.orc_pin_mq_byte_out(_u8p(b), C.c_size_t(b.size), C.c_long(0), C.c_uint32(c), C.byref(bp), C.byref(cc), C.byref(ct))
    assert (bp.value, ct.value, cc.value) == (1, 8, c & 0x7FFFF)
    assert b[1] == (c >> 19) & 0xFF


@pytest.mark.parametrize("byte,c,exp", [(0x00, 0, False), (0xFF, 0, True), (0x00, 0x8000000, True), (0xFF, 0x8000000, True),
                                        (0x7F, 0, False), (0x7F, 0x7FFFFFF, False)])
def test_mq_needs_slow_path(lib, byte, c, exp):
    assert bool(lib.orc_pin_mq_needs_slow_path(C.c_uint8(byte), C.c_uint32(c))) == exp


# ---- coverage_test.go:1193-1207 TestMQEncoder_ByteOut_AllBranches (state given, "buf[1] should be 0xFF") -------------
def test_mq_encoder_byte_out_all_branches(lib):
    b = np.array([0x00, 0xFE, 0x00, 0x00, 0x00], np.uint8)
    bp, cc, ct = C.c_long(), C.c_uint32(), C.c_uint32()
    lib.orc_pin_mq_byte_out(_u8p(b), C.c_size_t(b.size), C.c_long(1), C.c_uint32(0x8000000), C.byref(bp), C.byref(cc), C.byref(ct))
    assert b[1] == 0xFF and bp.value == 2 and ct.value == 7


# ---- coverage_test.go:1209-1239 TestMQDecoder_ByteIn_AllBranches -------------------------------------------------------
def test_mq_decoder_byte_in_all_branches(lib):
    data = np.array([0x00, 0x01, 0x02], np.uint8)
    bp, cc, ct, end = C.c_long(-1), C.c_uint32(0), C.c_uint32(0), C.c_int(0)
    lib.orc_pin_mq_byte_in(_u8p(data), C.c_long(3), C.byref(bp), C.byref(cc), C.byref(ct), C.byref(end))
    assert bp.value >= 0                                               # the reference's assertion
    assert (bp.value, cc.value, ct.value, end.value) == (1, 0x01 << 8, 8, 0)   # mqc.go:430-438
    bp, cc, ct, end = C.c_long(10), C.c_uint32(0), C.c_uint32(0), C.c_int(0)
    lib.orc_pin_mq_byte_in(_u8p(data), C.c_long(3), C.byref(bp), C.byref(cc), C.byref(ct), C.byref(end))
    assert end.value == 1 and cc.value == 0xFF00 and ct.value == 8     # "endCounter should be 1"


# ---- coverage_test.go:134-170 ByteOut_0xFF / ByteOut_Carry, mqc_test.go:43-66 LongSequence: the reference asserts
# "data is not empty" and decodability; pinned here as C oracle == pyref on those exact symbol sequences -------------------
@pytest.mark.parametrize("ctxs,decs", [
    ([0] * 500, [1] * 500),                                            # TestMQEncoder_ByteOut_0xFF
    ([i % 5 for i in range(1000)], [(i * 7) % 2 for i in range(1000)]),  # TestMQEncoder_ByteOut_Carry
    ([0] * 1000, [i % 2 for i in range(1000)]),                        # TestMQEncoder_LongSequence (mqc_test.go:43-66)
])
def test_mq_encoder_sequences(oracle, ctxs, decs):
    import pyref
    got = oracle.mq_encode(np.array(ctxs, np.uint8), np.array(decs, np.uint8))
    assert got.size > 0
    enc = pyref.MQEncoder()
    for c, d in zip(ctxs, decs):
        enc.encode(c, d)
    assert bytes(got) == bytes(enc.flush())
    assert oracle.mq_decode(got, np.array(ctxs, np.uint8)).tolist() == decs


# ---- coverage_test.go:961-989 TestGetSignContextParams (8 vectors), :991-1008 TestLutSC_Values ---------------------------
@pytest.mark.parametrize("hc,vc,exp_ctx,exp_xor", [(0, 0, 10, 0), (1, 0, 12, 0), (0, 1, 11, 0), (1, 1, 14, 0), (-1, 0, 12, 1),
                                                   (0, -1, 11, 1), (2, 0, 12, 0), (0, 2, 11, 0)])
def test_get_sign_context_params(lib, hc, vc, exp_ctx, exp_xor):
    ctx, x = C.c_int(), C.c_int()
    lib.orc_pin_sign_context_params(hc, vc, C.byref(ctx), C.byref(x))
    assert (ctx.value, x.value) == (exp_ctx, exp_xor)


# ---- coverage_test.go:261-307 TestGetSignContrib / TestClampContrib --------------------------------------------------------
@pytest.mark.parametrize("flag,exp", [(0, 0), (T1Sig, 1), (T1Sig | T1SignNeg, -1), (T1SignNeg, 0), (T1Visit, 0), (T1Sig | T1Visit, 1),
                                      (T1Sig | T1SignNeg | T1Refine, -1)])
def test_get_sign_contrib(lib, flag, exp):
    assert lib.orc_pin_sign_contrib(flag) == exp


@pytest.mark.parametrize("v,exp", [(0, 0), (1, 1), (-1, -1), (2, 2), (-2, -2), (3, 2), (-3, -2), (100, 2), (-100, -2)])
def test_clamp_contrib(lib, v, exp):
    assert lib.orc_pin_clamp_contrib(v) == exp


# ---- coverage_test.go:780-794 TestLutSCCtx_Values, :395-412 TestGetSCContextFast ------------------------------------------
def test_lut_sc_ctx_values(lib):
    v = lib.orc_pin_lut_sc_ctx(0, 0)
    assert (v >> 1, v & 1) == (CtxSC0, 0)                              # "(0,0) should be CtxSC0 with pred=0"
    for h in range(-3, 4):
        for vv in range(-3, 4):
            assert lib.orc_pin_lut_sc_ctx(h, vv) & 1 in (0, 1)
    # the 25-entry LUT and the 256-entry LUT the coders actually use (t1_luts.go:153-230) state the same rule
    zc, sc, sp = None, None, None
    import oracle as o
    zc, sc, sp = o.t1_luts()
    for i in range(256):
        wS, wC, eS, eC, nS, nC, sS, sC = [(i >> k) & 1 for k in range(8)]
        hc = (0 if not wS else (-1 if wC else 1)) + (0 if not eS else (-1 if eC else 1))
        vc = (0 if not nS else (-1 if nC else 1)) + (0 if not sS else (-1 if sC else 1))
        v = lib.orc_pin_lut_sc_ctx(hc, vc)
        assert (v & 1) == sp[i], (i, hc, vc)
        if hc == 0 and abs(vc) == 2:
            # the one place they differ: t1_luts.go:136-142 leaves `ctx` at its zero value (context 0, not CtxSC0) --
            # "it seems ctx can be 0 for certain edge cases" (coverage_test.go:403); getSCContextFast is dead code, the
            # coders use the 256-entry LUT, which (like t1.go:440-458) gives CtxSC0 here
            assert (v >> 1) == 0 and sc[i] == 0
        else:
            assert (v >> 1) - CtxSC0 == sc[i], (i, hc, vc)


# ---- coverage_test.go:796-812 TestLutSignCtx_Values, :764-778 TestLutZCCtx_Values, :380-393 TestGetZCContextFast ---------
def test_lut_sign_and_zc_values(oracle):
    zc, sc, sp = oracle.t1_luts()
    assert sc[0] == 0 and sc.max() <= 4 and sp.max() <= 1
    assert zc[0 * 256 + 0] == 0 and zc[0 * 256 + 0x03] == 8
    assert zc.max() <= 8


# ---- t1_test.go:181-197 TestT1_GetMRContext, coverage_test.go:690-718 TestT1_GetMRContext_Detailed -----------------------
def test_get_mr_context(lib):
    f = Flags(lib, 4, 4)
    assert f.call("orc_pin_mr_context", 1, 1) == CtxMag0              # first refinement, no neighbours
    f.set(1, 1, T1Refine)
    assert f.call("orc_pin_mr_context", 1, 1) == CtxMag2              # after refinement
    f = Flags(lib, 8, 8)
    assert f.call("orc_pin_mr_context", 4, 4) == CtxMag0
    f.set(3, 4, T1Sig)
    assert f.call("orc_pin_mr_context", 4, 4) == CtxMag1              # no refine, has neighbour
    f.clear(); f.set(4, 4, T1Refine)
    assert f.call("orc_pin_mr_context", 4, 4) == CtxMag2


# ---- coverage_test.go:721-762 TestT1_CanUseRunLength ------------------------------------------------------------------------
def test_can_use_run_length(lib):
    f = Flags(lib, 8, 12)
    assert not f.call("orc_pin_can_use_run_length", 0, 10)            # y + 4 > height
    f.set(0, 0, T1Sig)
    assert not f.call("orc_pin_can_use_run_length", 0, 0)             # coefficient significant
    f.clear(); f.set(0, 1, T1Visit)
    assert not f.call("orc_pin_can_use_run_length", 0, 0)             # coefficient visited
    f.clear(); f.set(1, 0, T1Sig); f.call("orc_pin_update_neighbor_flags", 1, 0)
    assert not f.call("orc_pin_can_use_run_length", 0, 0)             # neighbour significant
    f.clear()
    assert f.call("orc_pin_can_use_run_length", 4, 0)                 # all clear


# ---- coverage_test.go:1010-1056 HasSignificantNeighbor_Edges / UpdateNeighborFlags_Edges ----------------------------------
def test_neighbor_flags_edges(lib):
    f = Flags(lib, 8, 8)
    f.set(1, 0, T1Sig)
    assert f.call("orc_pin_has_sig_neighbor", 0, 0)                   # east neighbour of the corner
    f.clear(); f.set(6, 7, T1Sig)
    assert f.call("orc_pin_has_sig_neighbor", 7, 7)                   # west neighbour of the far corner
    f.clear(); f.call("orc_pin_update_neighbor_flags", 0, 0)
    assert f.has(1, 0, T1SigW) and f.has(0, 1, T1SigN)
    assert int(f.f.astype(bool).sum()) == 2                           # nothing outside the block (x > 0, y > 0 guards)
    f.clear(); f.call("orc_pin_update_neighbor_flags", 7, 7)
    assert f.has(6, 7, T1SigE) and f.has(7, 6, T1SigS)
    assert int(f.f.astype(bool).sum()) == 2


# ---- t1_test.go:148-179 GetZCContext / GetSCContext, coverage_test.go:537-688 *_Detailed ------------------------------------
def test_zc_sc_context_from_flags(lib):
    f = Flags(lib, 4, 4)
    assert f.call("orc_pin_zc_context", 1, 1, 0) == CtxZC0
    f.set(0, 1, T1Sig); f.call("orc_pin_update_neighbor_flags", 0, 1)
    assert f.call("orc_pin_zc_context", 1, 1, 0) != CtxZC0            # one horizontal neighbour
    ctx, pred = C.c_int(), C.c_int()
    f = Flags(lib, 8, 8)
    cases = [[], [(3, 4, T1Sig)], [(3, 4, T1Sig | T1SignNeg)], [(3, 4, T1Sig), (5, 4, T1Sig)], [(3, 4, T1Sig | T1SignNeg), (5, 4, T1Sig)],
             [(3, 4, T1Sig | T1SignNeg), (5, 4, T1Sig), (4, 3, T1Sig | T1SignNeg), (4, 5, T1Sig)]]
    got = []
    for setup in cases:
        f.clear()
        for x, y, fl in setup:
            f.set(x, y, fl)
        f.call("orc_pin_sc_context", 4, 4, C.byref(ctx), C.byref(pred))
        assert CtxSC0 <= ctx.value <= CtxSC4 and pred.value in (0, 1)
        got.append((ctx.value - CtxSC0, pred.value))
    # what t1.go:387-460 gives for those six set-ups (hc, vc) = (0,0) (1,0) (-1,0) (2,0) (0,0) (0,0)
    assert got == [(0, 0), (2, 0), (2, 1), (3, 0), (0, 0), (0, 0)]
    zc_cases = [([], 0, 0), ([], 3, 0), ([(3, 4), (5, 4)], 0, 8), ([(3, 4), (5, 4)], 1, 4), ([(4, 3), (4, 5)], 2, 4), ([(3, 3), (5, 5)], 3, 2),
                ([(4 + dx, 4 + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if dx or dy], 3, 8)]
    for setup, band, exp in zc_cases:                                   # expectations follow t1_luts.go:34-110
        f.clear()
        for x, y in setup:
            f.set(x, y, T1Sig)
        assert f.call("orc_pin_zc_context", 4, 4, band) == exp, (setup, band)


# ---- ht_test.go:126-147 TestHTDecoderMinimalData: nil / 1 byte / {0x00, 0x02} -> a (zero) 16x16 block, never nil --------------
def test_ht_decoder_minimal_data(oracle):
    import os
    import pyref
    tabs = pyref.load_ht_tables(os.path.join(os.path.dirname(os.path.abspath(pyref.__file__)), "ht_tables.h"))
    for data in ([], [0x00], [0x00, 0x02]):
        out = oracle.ht_decode(np.array(data, np.uint8), 16, 16, num_bitplanes=8)
        assert out.shape == (16, 16)                                    # the reference's assertion: "not nil"
        if len(data) < 2:
            assert not out.any()                                        # ht.go:94-99: fewer than 2 bytes -> zeros
        # {0x00, 0x02}: scup = 2 = n passes ht.go:104-111 and the cleanup pass runs on an empty MagSgn segment (feeds 0xFF,
        # ht.go:407): a NON-zero block -- C oracle == pyref
        want = np.array(pyref.HTDecoder(16, 16, tabs).decode(bytes(data)), np.int32).reshape(16, 16)
        assert np.array_equal(out, want)


# ---- internal/mct/mct_test.go:157-169 TestConvertFloat64ToInt32 (6 vectors), :785-808 _EdgeCases (the empty slice + 7 vectors) -------
# by the round_half_away of orc_preprocess / orc_tcd_inverse_dwt (encoder.go:238-242 states mct.go:137-145 again)
@pytest.mark.parametrize("src,exp", [
    ([0.4, 0.5, 0.6, -0.4, -0.5, -0.6], [0, 1, 1, 0, -1, -1]),
    ([], []), ([0.0], [0]), ([0.49999], [0]), ([0.50001], [1]), ([-0.49999], [0]), ([-0.50001], [-1]), ([100.5, -100.5], [101, -101]),
])
def test_convert_float64_to_int32(lib, src, exp):
    s = np.array(src + [0.0], np.float64)                              # (one spare element: an empty array has no address to pass)
    d = np.full(len(src) + 1, 77, np.int32)
    lib.orc_pin_round_half_away(s.ctypes.data_as(C.POINTER(C.c_double)), d.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(len(src)))
    assert d[:len(src)].tolist() == exp and d[len(src)] == 77


# ---- ht_test.go:80-92 TestHTEncoderEmptyBlock, :8-77 TestHTEncoderDecoder (only a logged match rate) ---------------------------
def test_ht_encoder_reference_inputs(oracle):
    import pyref
    assert oracle.ht_encode(np.zeros(32 * 32, np.int32), 32, 32).size == 0          # "Empty block should produce nil"
    # the reference test's own input generator: data[i] = (i%64) - 32 on 64x64 (ht_test.go:12-20); it logs a match rate and
    # asserts nothing numeric -- pinned as C oracle == pyref, bytes and decoded samples
    x = ((np.arange(64 * 64) % 64) - 32).astype(np.int32)
    b = oracle.ht_encode(x, 64, 64)
    import os
    tabs = pyref.load_ht_tables(os.path.join(os.path.dirname(os.path.abspath(pyref.__file__)), "ht_tables.h"))
    assert bytes(b) == pyref.HTEncoder(64, 64, tabs).encode([int(v) for v in x])
    dec = pyref.HTDecoder(64, 64, tabs).decode(bytes(b))
    assert np.array_equal(np.array(dec, np.int32).reshape(64, 64), oracle.ht_decode(b, 64, 64, num_bitplanes=8))
