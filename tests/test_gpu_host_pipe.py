"""The pipelined host codec (j2k_pipe_*, codec.HostPipe) against the synchronous one-call forms it must equal byte for byte.

Frames are 200 x 72 with 64 x 64 tiles (partial tiles on both axes), 3 resolutions, 16 x 16 or 32 x 32 blocks.  Every expected value -- tile-parts,
out_len, tile_offs, lens, numbps, decoded pixels, the status of a refused frame -- comes from encode_pixels_host / decode_pixels_host on a SECOND
plan with the same parameters (those forms are pinned to the oracle by the other test modules), computed once per plan before any frame is
submitted; nothing expected comes from the pipe.  Damaged streams are of the kinds the readers already refuse cleanly (tests/stream_reader_cases.py:
a tile-part whose Psot reaches past the stream, packets whose header bits run out); no test provokes a device fault."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MQ, HT = 0, 1
GRAY8, GRAY16, RGBA8, RGBA64 = 0, 1, 2, 3
W, H = 200, 72
POISON = 0xA5
GUARD = 64
KW = dict(lossless=True, num_resolutions=3, tile=(64, 64))
# name -> (components, precision, pixel format, bytes per pixel, SOP / EPH, FramePlan keywords)
PLANS = {
    "cl_mq": (3, 8, RGBA8, 4, True, dict(KW, cb=(32, 32), coder=MQ, closed_loop=True)),
    "cl_ht": (1, 8, GRAY8, 1, False, dict(KW, cb=(16, 16), coder=HT, closed_loop=True)),
    "mallat_mq": (1, 16, GRAY16, 2, True, dict(KW, cb=(32, 32), coder=MQ, mallat=True)),
    "ref_mq": (3, 16, RGBA64, 8, False, dict(KW, cb=(32, 32), coder=MQ)),
    "ref_ht": (3, 8, RGBA8, 4, False, dict(KW, cb=(16, 16), coder=HT)),
}
NFRAMES = 7                                     # 2 * depth + 1 at the largest depth tested


def make_pixels(fmt, seed, stride=None):
    """a gradient plus low-amplitude noise in the Go Pix layout of `fmt` (opaque alpha), rows `stride` bytes apart, padding poisoned"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    ch = 1 if fmt in (GRAY8, GRAY16) else 4
    if fmt in (GRAY8, RGBA8):
        pix = np.full((H, W, ch), 255, np.uint8)
        for c in range(min(ch, 3)):
            pix[:, :, c] = np.clip((2 * x + 3 * y + 40 * c + 11 * seed) % 256 + rng.integers(-4, 5, size=(H, W)), 0, 255)
        rows = pix.reshape(H, W * ch)
    else:
        v = np.full((H, W, ch), 65535, np.uint16)
        for c in range(min(ch, 3)):
            v[:, :, c] = np.clip((331 * x + 197 * y + 4000 * c + 977 * seed) % 65536 + rng.integers(-64, 65, size=(H, W)), 0, 65535)
        rows = np.stack([(v >> 8).astype(np.uint8), (v & 255).astype(np.uint8)], axis=-1).reshape(H, W * ch * 2)      # big-endian samples
    if stride is None:
        return np.ascontiguousarray(rows)
    out = np.full((H, stride), POISON, np.uint8)
    out[:, :rows.shape[1]] = rows
    return out


class Env:
    def __init__(self):
        import torch  # noqa: F401
        from j2kgfx import Context, J2KError, _lib
        from j2kgfx import codec
        self.J2KError, self.lib, self.codec = J2KError, _lib, codec
        self.ctx = Context(0)
        self.plans, self.refs, self.want = {}, {}, {}

    def make(self, name, ctx=None):
        Cn, prec = PLANS[name][:2]
        return self.codec.FramePlan(W, H, Cn, precision=prec, ctx=ctx or self.ctx, **PLANS[name][5])

    def plan(self, name):
        """(the plan the pipes run on, what the one-call forms gave on a second plan with the same parameters)"""
        if name not in self.plans:
            Cn, prec, fmt, pb, marks, kw = PLANS[name]
            ref = self.make(name)
            frames = [make_pixels(fmt, s) for s in range(NFRAMES)]
            enc = [ref.encode_pixels_host(fmt, f, sop=marks, eph=marks) for f in frames]
            dec = [ref.decode_pixels_host(e["bytes"], (H, W * pb), sop=marks, eph=marks) for e in enc] if kw.get("closed_loop") or kw.get("mallat") else None
            self.refs[name] = ref
            self.want[name] = dict(frames=frames, enc=enc, dec=dec)
            self.plans[name] = self.make(name)
        return self.plans[name], self.want[name]

    def close(self):
        for p in list(self.plans.values()) + list(self.refs.values()):
            p.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def same_encode(got, want):
    assert got["bytes"].size == want["bytes"].size and np.array_equal(got["bytes"], want["bytes"])
    for k in ("tile_offs", "lens", "numbps"):
        assert np.array_equal(got[k], want[k]), k


def guarded(codec, nbytes, pinned, offset=0):
    """(the whole poisoned buffer, the window of nbytes at GUARD + offset inside it)"""
    n = nbytes + 2 * GUARD + offset
    buf = codec.pinned_empty(n) if pinned else np.empty(n, np.uint8)
    buf[:] = POISON
    return buf, buf[GUARD + offset:GUARD + offset + nbytes]


def guards_intact(buf, nbytes, offset=0):
    return bool(np.all(buf[:GUARD + offset] == POISON) and np.all(buf[GUARD + offset + nbytes:] == POISON))


# ---- 1. identity with the one-call forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("name", list(PLANS))
def test_identity_with_the_one_call_forms(env, name, depth):
    plan, want = env.plan(name)
    Cn, prec, fmt, pb, marks, kw = PLANS[name]
    n = 2 * depth + 1
    jobs = [("enc", i) for i in range(n)] + ([("dec", i) for i in range(n)] if want["dec"] is not None else [])

    def submit(pipe, job):
        kind, i = job
        if kind == "enc":
            return pipe.submit_encode(fmt, want["frames"][i], sop=marks, eph=marks)
        pix = np.full((H, W * pb), POISON, np.uint8)
        return pipe.submit_decode(want["enc"][i]["bytes"], pix, sop=marks, eph=marks)

    def check(pipe, job, ticket):
        kind, i = job
        got = pipe.wait(ticket)
        if kind == "enc":
            same_encode(got, want["enc"][i])
            assert pipe.encoded_len == want["enc"][i]["bytes"].size
        else:
            assert np.array_equal(got, want["dec"][i])

    with env.codec.HostPipe(plan, depth=depth) as pipe:
        # back to back, waited in order: the oldest ticket is waited when the un-waited limit is reached
        flight, expect_ticket = [], 1
        for job in jobs:
            if len(flight) == depth:
                check(pipe, *flight.pop(0))
            t = submit(pipe, job)
            assert t == expect_ticket
            expect_ticket += 1
            flight.append((job, t))
        while flight:
            check(pipe, *flight.pop(0))
        # once more, every window of `depth` frames waited in reverse order
        for k in range(0, len(jobs), depth):
            flight = [(job, submit(pipe, job)) for job in jobs[k:k + depth]]
            assert all(pipe.poll(t) in (False, True) for _, t in flight)
            for job, t in reversed(flight):
                check(pipe, job, t)


# ---- 2. memory cases --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cl_mq", "cl_ht"])
def test_memory_cases_give_identical_results_and_keep_the_poison(env, name):
    """every pinned / pageable combination of input and output; strides with padding (W * pb + 12, and W * pb + 4 resp. + 5: no multiple of 16); a pinned
    frame that starts 4 bytes into its allocation; a pinned frame whose address the device call does not take directly (2 bytes in, for RGBA rows)
    and so goes through the slot's device frame; row padding, the bytes behind out_len and the guard bytes around every buffer keep their poison"""
    plan, want = env.plan(name)
    Cn, prec, fmt, pb, marks, kw = PLANS[name]
    codec = env.codec
    row = W * pb
    strides = [row, row + 12, row + (4 if Cn != 1 else 5)]
    assert any(s % 16 for s in strides)
    frame, enc, dec = want["frames"][1], want["enc"][1], want["dec"][1]
    cap = enc["bytes"].size + 37
    with codec.HostPipe(plan, depth=2) as pipe:
        # encode: (input pinned?, output pinned?, stride)
        cases = [(pi, po, s) for s in strides for pi in (False, True) for po in (False, True)]
        flight = []

        def finish(item):
            t, ibuf, n_in, obuf = item
            got = pipe.wait(t)
            same_encode(got, enc)                                      # identical across every case: the padding is never part of the image
            assert guards_intact(obuf, cap) and np.all(obuf[GUARD + enc["bytes"].size:] == POISON)
            assert guards_intact(ibuf, n_in)
        for pi, po, s in cases:
            ibuf, iwin = guarded(codec, H * s, pi)
            pix = iwin.reshape(H, s)
            pix[:, :row] = frame
            obuf, owin = guarded(codec, cap, po)
            if len(flight) == 2:
                finish(flight.pop(0))
            flight.append((pipe.submit_encode(fmt, pix, sop=marks, eph=marks, cap=cap, out=owin), ibuf, H * s, obuf))
        while flight:
            finish(flight.pop(0))
        # decode: (stream pinned?, frame memory, stride); frame memory: pageable, pinned, pinned + 4 bytes, pinned + 2 bytes (RGBA: staged)
        kinds = [("page", False, 0), ("pin", True, 0), ("pin+4", True, 4), ("pin+2", True, 2)]
        cases = [(pc, k, s) for s in strides for pc in (False, True) for k in kinds]

        def finish_dec(item):
            t, pbuf, n_pix, off, pix, s = item
            got = pipe.wait(t)
            assert got is pix
            assert np.array_equal(pix[:, :row], dec), (s, off)
            assert np.all(pix[:-1, row:] == POISON)                    # the row padding, pixel for pixel beside the stored rows
            assert guards_intact(pbuf, n_pix, off)
        for pc, (kname, pp, off), s in cases:
            n_pix = (H - 1) * s + row                                  # (the last row has no padding: the guard starts right behind the image)
            pbuf, pwin = guarded(codec, n_pix, pp, off)
            pix = np.lib.stride_tricks.as_strided(pwin, shape=(H, s), strides=(s, 1)) if s != row else pwin.reshape(H, row)
            cs = enc["bytes"]
            if pc:
                cs = codec.pinned_empty(enc["bytes"].size)
                cs[:] = enc["bytes"]
            if len(flight) == 2:
                finish_dec(flight.pop(0))
            flight.append((pipe.submit_decode(cs, pix, sop=marks, eph=marks), pbuf, n_pix, off, pix, s))
        while flight:
            finish_dec(flight.pop(0))


# ---- 3. errors ------------------------------------------------------------------------------------------------------------------------------------
def damaged_streams(stream, tile_offs):
    """{kind: bytes}: the last tile-part's Psot one past the stream's end; its Psot cut to 15 and the stream with it (one byte of packets: the header
    bits run out)"""
    last = int(tile_offs[-2])
    past = bytearray(stream)
    past[last + 6:last + 10] = int(len(stream) - last + 1).to_bytes(4, "big")
    short = bytearray(stream[:last + 15])
    short[last + 6:last + 10] = int(15).to_bytes(4, "big")
    return {"psot_past_the_end": np.frombuffer(bytes(past), np.uint8), "header_bits_run_out": np.frombuffer(bytes(short), np.uint8)}


@pytest.mark.parametrize("pinned", [False, True])
def test_capacity_one_byte_short(env, pinned):
    plan, want = env.plan("cl_mq")
    Cn, prec, fmt, pb, marks, kw = PLANS["cl_mq"]
    enc = want["enc"]
    ref = env.refs["cl_mq"]
    need = enc[2]["bytes"].size
    with pytest.raises(env.J2KError) as e:                             # the one-call form says what the pipe must say
        ref.encode_pixels_host(fmt, want["frames"][2], sop=marks, eph=marks, cap=need - 1)
    assert e.value.status == env.lib.ERR_CAPACITY and ref.encoded_len == need
    with env.codec.HostPipe(plan, depth=3) as pipe:
        obuf, owin = guarded(env.codec, need - 1, pinned)
        t1 = pipe.submit_encode(fmt, want["frames"][1], sop=marks, eph=marks)
        t2 = pipe.submit_encode(fmt, want["frames"][2], sop=marks, eph=marks, cap=need - 1, out=owin)
        t3 = pipe.submit_encode(fmt, want["frames"][3], sop=marks, eph=marks)
        same_encode(pipe.wait(t1), enc[1])
        with pytest.raises(env.J2KError) as e:
            pipe.wait(t2)
        assert e.value.status == env.lib.ERR_CAPACITY and pipe.encoded_len == need
        assert np.all(obuf == POISON)                                  # out untouched
        same_encode(pipe.wait(t3), enc[3])


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("kind", ["psot_past_the_end", "header_bits_run_out"])
def test_a_damaged_stream_between_two_good_ones(env, kind, pinned, depth):
    plan, want = env.plan("cl_mq")
    Cn, prec, fmt, pb, marks, kw = PLANS["cl_mq"]
    bad = damaged_streams(want["enc"][2]["bytes"], want["enc"][2]["tile_offs"])[kind]
    ref = env.refs["cl_mq"]
    with pytest.raises(env.J2KError) as e:                             # the readers refuse it cleanly; the one-call form's status is the expected one
        ref.decode_pixels_host(bad, (H, W * pb), sop=marks, eph=marks)
    assert e.value.status == env.lib.ERR_INVALID_ARG
    with env.codec.HostPipe(plan, depth=depth) as pipe:
        bufs = [guarded(env.codec, H * W * pb, pinned) for _ in range(3)]
        streams = [want["enc"][1]["bytes"], bad, want["enc"][3]["bytes"]]
        tickets, results = [], {}

        def wait(i):
            try:
                results[i] = pipe.wait(tickets[i])
            except env.J2KError as err:
                results[i] = err.status
        for i in range(3):
            if i >= depth:
                wait(i - depth)
            tickets.append(pipe.submit_decode(streams[i], bufs[i][1].reshape(H, W * pb), sop=marks, eph=marks))
        for i in range(3):
            if i not in results:
                wait(i)
        assert tickets == [1, 2, 3]
        assert results[1] == env.lib.ERR_INVALID_ARG                   # from its own wait
        assert np.all(bufs[1][0] == POISON)                            # its pix untouched
        assert np.array_equal(results[0], want["dec"][1]) and np.array_equal(results[2], want["dec"][3])      # its neighbours bit-exact
        assert all(guards_intact(b[0], H * W * pb) for b in bufs)


def test_submit_time_refusals_consume_no_ticket(env):
    plan, want = env.plan("cl_mq")
    Cn, prec, fmt, pb, marks, kw = PLANS["cl_mq"]
    L, lib = env.ctx.L, env.lib
    frame, stream = want["frames"][0], want["enc"][0]["bytes"]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros(want["enc"][0]["bytes"].size + 64, np.uint8)
    pix = np.full((H, W * pb), POISON, np.uint8)
    with env.codec.HostPipe(plan, depth=2) as pipe:
        t = C.c_uint64(0)
        enc = lambda f, p, stride, o, tk: L.j2k_pipe_submit_encode(pipe.h, f, p, C.c_size_t(stride), 0, 0, o, C.c_size_t(out.size), None, None, None, tk)
        dec = lambda c, p, stride, tk: L.j2k_pipe_submit_decode(pipe.h, c, C.c_size_t(stream.size), 0, 0, p, C.c_size_t(stride), tk)
        assert enc(99, ptr(frame), W * pb, ptr(out), C.byref(t)) == lib.ERR_INVALID_ARG          # a bad format
        assert enc(GRAY8, ptr(frame), W * pb, ptr(out), C.byref(t)) == lib.ERR_INVALID_ARG       # a format of another component count
        assert enc(fmt, ptr(frame), W * pb - 1, ptr(out), C.byref(t)) == lib.ERR_INVALID_ARG     # a short stride
        assert enc(fmt, None, W * pb, ptr(out), C.byref(t)) == lib.ERR_INVALID_ARG               # NULL arguments
        assert enc(fmt, ptr(frame), W * pb, ptr(out), None) == lib.ERR_INVALID_ARG
        assert dec(None, ptr(pix), W * pb, C.byref(t)) == lib.ERR_INVALID_ARG
        assert dec(ptr(stream), None, W * pb, C.byref(t)) == lib.ERR_INVALID_ARG
        assert dec(ptr(stream), ptr(pix), W * pb, None) == lib.ERR_INVALID_ARG
        assert dec(ptr(stream), ptr(pix), W * pb - 1, C.byref(t)) == lib.ERR_INVALID_ARG         # a short stride
        assert dec(ptr(stream), ptr(pix), W * pb + 2, C.byref(t)) == lib.ERR_INVALID_ARG         # RGBA rows off 4-byte alignment (j2k_pack_pixels' rule)
        assert L.j2k_pipe_submit_encode(None, fmt, ptr(frame), C.c_size_t(W * pb), 0, 0, ptr(out), C.c_size_t(out.size), None, None, None, C.byref(t)) == lib.ERR_INVALID_ARG
        assert t.value == 0 and np.all(pix == POISON)
        done = C.c_int(0)
        assert L.j2k_pipe_wait(pipe.h, C.c_uint64(1), None) == lib.ERR_INVALID_ARG              # nothing was submitted: ticket 1 is unknown
        assert L.j2k_pipe_poll(pipe.h, C.c_uint64(1), C.byref(done)) == lib.ERR_INVALID_ARG
        t1 = pipe.submit_encode(fmt, frame)                                                     # the first frame accepted is ticket 1
        t2 = pipe.submit_decode(stream, pix, sop=marks, eph=marks)
        assert (t1, t2) == (1, 2)
        with pytest.raises(env.J2KError) as e:                                                  # depth + 1 without a wait
            pipe.submit_encode(fmt, frame)
        assert e.value.status == lib.ERR_INVALID_ARG
        assert L.j2k_pipe_wait(pipe.h, C.c_uint64(3), None) == lib.ERR_INVALID_ARG              # ... consumed no ticket
        pipe.wait(t1)
        assert pipe.submit_encode(fmt, frame) == 3
        with pytest.raises(env.J2KError) as e:                                                  # a stale ticket
            pipe.wait(t1)
        assert e.value.status == lib.ERR_INVALID_ARG
        assert np.array_equal(pipe.wait(t2), want["dec"][0])
        pipe.wait(3)
    # a decode on a reference-mode plan: J2K_ERR_UNSUPPORTED from the submit, as the one-call form
    rplan, rwant = env.plan("ref_mq")
    with pytest.raises(env.J2KError) as e:
        env.refs["ref_mq"].decode_pixels_host(rwant["enc"][0]["bytes"], (H, W * 8))
    assert e.value.status == lib.ERR_UNSUPPORTED
    with env.codec.HostPipe(rplan, depth=1) as pipe:
        with pytest.raises(env.J2KError) as e:
            pipe.submit_decode(rwant["enc"][0]["bytes"], np.zeros((H, W * 8), np.uint8))
        assert e.value.status == lib.ERR_UNSUPPORTED
        assert pipe.submit_encode(RGBA64, rwant["frames"][0]) == 1
        same_encode(pipe.wait(1), rwant["enc"][0])
    h = C.c_void_p()
    assert L.j2k_pipe_create(plan.h, 0, C.byref(h)) == lib.ERR_INVALID_ARG and L.j2k_pipe_create(plan.h, 9, C.byref(h)) == lib.ERR_INVALID_ARG
    assert L.j2k_pipe_create(None, 2, C.byref(h)) == lib.ERR_INVALID_ARG and not h.value


# ---- 4. lifecycle ---------------------------------------------------------------------------------------------------------------------------------
def test_drain_then_the_waits(env):
    plan, want = env.plan("cl_ht")
    Cn, prec, fmt, pb, marks, kw = PLANS["cl_ht"]
    with env.codec.HostPipe(plan, depth=3) as pipe:
        pixs = [env.codec.pinned_empty((H, W * pb)) for _ in range(2)]
        t1 = pipe.submit_encode(fmt, want["frames"][4])
        t2 = pipe.submit_decode(want["enc"][5]["bytes"], pixs[0])
        t3 = pipe.submit_decode(want["enc"][6]["bytes"], pixs[1])
        pipe.drain()
        assert pipe.poll(t1) and pipe.poll(t2) and pipe.poll(t3)       # all submitted work complete; the tickets stay waitable
        assert np.array_equal(pipe.wait(t3), want["dec"][6])
        same_encode(pipe.wait(t1), want["enc"][4])
        assert np.array_equal(pipe.wait(t2), want["dec"][5])
        pipe.drain()                                                   # an idle pipe drains too


def test_destroy_with_frames_in_flight_leaves_the_plan_to_the_one_call_forms(env):
    plan, want = env.plan("cl_mq")
    Cn, prec, fmt, pb, marks, kw = PLANS["cl_mq"]
    pipe = env.codec.HostPipe(plan, depth=3)
    pix = np.full((H, W * pb), POISON, np.uint8)
    bad = damaged_streams(want["enc"][2]["bytes"], want["enc"][2]["tile_offs"])["psot_past_the_end"]
    pipe.submit_encode(fmt, want["frames"][5], sop=marks, eph=marks)
    pipe.submit_decode(bad, pix, sop=marks, eph=marks)                # (a refused frame in flight: its status must not reach the plan's next call)
    pipe.submit_encode(fmt, want["frames"][6], sop=marks, eph=marks)
    pipe.close()
    same_encode(plan.encode_pixels_host(fmt, want["frames"][0], sop=marks, eph=marks), want["enc"][0])       # the recorded bytes
    assert np.array_equal(plan.decode_pixels_host(want["enc"][0]["bytes"], (H, W * pb), sop=marks, eph=marks), want["dec"][0])
    with env.codec.HostPipe(plan, depth=1) as again:                   # and a new pipe on the same plan
        same_encode(again.wait(again.submit_encode(fmt, want["frames"][1], sop=marks, eph=marks)), want["enc"][1])


def test_two_pipes_on_two_contexts_used_alternately(env):
    from j2kgfx import Context
    plan, want = env.plan("cl_mq")
    _, hwant = env.plan("cl_ht")
    Cn, prec, fmt, pb, marks, kw = PLANS["cl_mq"]
    ctx2 = Context(0)
    try:
        plan2 = env.make("cl_ht", ctx=ctx2)
        with env.codec.HostPipe(plan, depth=2) as a, env.codec.HostPipe(plan2, depth=2) as b:
            ta, tb = [], []
            for i in range(4):
                if i >= 2:
                    same_encode(a.wait(ta[i - 2]), want["enc"][i - 2])
                    same_encode(b.wait(tb[i - 2]), hwant["enc"][i - 2])
                ta.append(a.submit_encode(fmt, want["frames"][i], sop=marks, eph=marks))
                tb.append(b.submit_encode(GRAY8, hwant["frames"][i]))
            for i in (2, 3):
                same_encode(b.wait(tb[i]), hwant["enc"][i])
                same_encode(a.wait(ta[i]), want["enc"][i])
            pa, pb_ = np.zeros((H, W * pb), np.uint8), np.zeros((H, W), np.uint8)
            t1, t2 = a.submit_decode(want["enc"][3]["bytes"], pa, sop=marks, eph=marks), b.submit_decode(hwant["enc"][3]["bytes"], pb_)
            assert np.array_equal(b.wait(t2), hwant["dec"][3]) and np.array_equal(a.wait(t1), want["dec"][3])
        plan2.close()
    finally:
        ctx2.close()
