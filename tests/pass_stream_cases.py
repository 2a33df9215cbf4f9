"""The pass reader (j2k_plan_decode_tile_parts_pfloors: decode_tile_parts(pfloors=True), decode_frame_pixels(pass_cuts=True)) and the pass-stopped
block decoder (j2k_plan_decode_blocks_pfloors: the PASSCUT form of t1_decode64_kernel) on streams this library's encoder never writes, importable
without a GPU: tests/test_pass_stream_cases.py checks this file on the CPU, tests/test_gpu_pass_streams.py holds the device against it bit for bit.

decode_passes() is the reference decoder that stops f coding passes short of a block's last, written on the primitives of oracle/pyref.py; it keeps
an explicit record of which sample the partial plane touched and takes the midpoints from that record, so it does not share the device's shortcut
(t1_pass_mid reads the same from the magnitude's low bits).  pass_tables() adds pass-granular shortest-prefix tables to the geometries of
tests/stream_reader_cases.py; pass_family() makes cut families that neither rate_cases.allocate nor pass_cases.allocate_quality return;
pass_stream() composes them (pass_cases.compose_kept_passes); expected_coeffs() is what the device must decode from what the yardstick
(stream_reader_cases.read_tiles, its pfloor record) reads."""
import functools

import numpy as np

import coarse_cases as cc
import layer_cases as lc
import pass_cases as pc
import stream_reader_cases as sr


# ---- 1. the pass-stopped reference decoder --------------------------------------------------------------------------------------------------
def decode_passes(data, numbps, band, w, h, f):
    """int32 [h, w]: the block decoded f coding passes short of its last -- pass_cases.decode_plan(f): whole planes from numbps - 1 down to
    k = ceil(f / 3), then the first part = 3 k - f passes of plane k - 1 (its SigProp; with part = 2 its MagRef too) where 1 <= k <= numbps.
    Every sample takes the midpoint of what ITS passes left undecoded (pass_cases.floors_pass): floor k - 1 if the partial plane's SigProp turned it
    significant or its MagRef refined it -- taken from the record kept here, not from the magnitude -- else floor k; the value is
    coarse_cases.coarse(sample, floor).  f beyond the block's passes (k >= numbps): no pass runs, zeros.  numbps == 0: zeros; empty data: the
    MQ decoder reads its 0xFF fill, as oracle.t1_decode does.  f = 0 is oracle.t1_decode."""
    import pyref
    numbps, w, h, f = int(numbps), int(w), int(h), int(f)
    assert 0 <= numbps <= 31 and f >= 0
    t = pyref.T1(w, h)
    t.band = int(band)
    mq = pyref.MQDecoder(bytes(bytearray(data)))
    SIG, VISIT, REFINE, NEG = pyref.T1_SIG, pyref.T1_VISIT, pyref.T1_REFINE, pyref.T1_SIGN_NEG
    flags, mag = t.flags, t.data
    turned, refined = [False] * (w * h), [False] * (w * h)

    def dec_sign(x, y):
        ctx, pred = t.sc(x, y)
        if mq.decode(ctx) ^ pred:
            flags[t.fi(x, y)] |= NEG

    def sigprop(bit, record):
        for y in range(h):
            for x in range(w):
                i = t.fi(x, y)
                if flags[i] & SIG or not t.has_sig_neighbor(x, y):
                    continue
                if mq.decode(t.zc(x, y)):
                    mag[y * w + x] = bit
                    dec_sign(x, y)
                    flags[i] |= SIG
                    if record:
                        turned[y * w + x] = True
                flags[i] |= VISIT

    def magref(bit, record):
        for y in range(h):
            for x in range(w):
                i = t.fi(x, y)
                if flags[i] & SIG == 0 or flags[i] & VISIT:
                    continue
                if mq.decode(t.mr(x, y)):
                    mag[y * w + x] |= bit
                flags[i] |= REFINE
                if record:
                    refined[y * w + x] = True

    def cleanup(bit):
        for y in range(0, h, 4):
            for x in range(w):
                if t.can_rl(x, y):
                    if mq.decode(pyref.CTX_RL) == 0:
                        continue
                    pos = mq.decode(pyref.CTX_UNI) << 1
                    pos |= mq.decode(pyref.CTX_UNI)
                    mag[(y + pos) * w + x] = bit
                    dec_sign(x, y + pos)
                    flags[t.fi(x, y + pos)] |= SIG
                    for i in range(pos + 1, 4):
                        if y + i >= h:
                            break
                        if mq.decode(t.zc(x, y + i)):
                            mag[(y + i) * w + x] = bit
                            dec_sign(x, y + i)
                            flags[t.fi(x, y + i)] |= SIG
                    continue
                for yy in range(y, min(y + 4, h)):
                    i = t.fi(x, yy)
                    if flags[i] & VISIT:
                        flags[i] &= ~VISIT
                        continue
                    if flags[i] & SIG:
                        continue
                    if mq.decode(t.zc(x, yy)):
                        mag[yy * w + x] = bit
                        dec_sign(x, yy)
                        flags[i] |= SIG

    k, part = pc.decode_plan(f)
    for bp in range(numbps - 1, k - 1, -1):
        sigprop(1 << bp, False)
        magref(1 << bp, False)
        cleanup(1 << bp)
    if part > 0 and 1 <= k <= numbps:
        sigprop(1 << (k - 1), True)
        if part > 1:
            magref(1 << (k - 1), True)
    v = np.array([-m if flags[t.fi(i % w, i // w)] & NEG else m for i, m in enumerate(mag)], np.int64).reshape(h, w)
    if not v.any():
        return np.zeros((h, w), np.int32)
    lower = (np.array(turned, bool) | np.array(refined, bool)).reshape(h, w)
    out = np.where(lower, cc.coarse(v, max(k - 1, 0)), cc.coarse(v, k))
    return out.astype(np.int32)


@functools.lru_cache(None)
def decode_passes_cached(data, numbps, band, w, h, f):
    """decode_passes on bytes, computed once per argument tuple, read-only"""
    out = decode_passes(data, numbps, band, w, h, f)
    out.setflags(write=False)
    return out


def shortest_rates_pass(oracle, data, nb, band, v, sp, strict=True):
    """layer_cases.shortest_rates at pass granularity: R[q] = the shortest prefix not below R[q - 1] whose decode has every pass up to q right
    (pass_cases.prefix_ok_pass), R[0] = 0, R[3 nb - 2] = len(data).
    strict: ... and whose decode_passes, stopped behind pass q, IS coarse_pass(v, nb, q, sp).  prefix_ok_pass alone does not say that inside a plane:
    it looks at the prefix's FULL decode, where a sample that plane b's SigProp visits and leaves at 0 is compared at floor b + 1 -- a prefix that
    wrongly turns it to 2^b passes.  (The plane-granular check has no such sample: behind Cleanup every sample stands at floor b.)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    h, w = v.shape

    def ok(m, q):
        if not pc.prefix_ok_pass(oracle, data, m, nb, band, v, q, sp):
            return False
        return not strict or np.array_equal(decode_passes(data[:m], nb, band, w, h, pc.pfloor_of(nb, q)), pc.coarse_pass(v, nb, q, sp))
    R = [0]
    for q in range(1, pc.points(nb) + 1):
        m = R[-1]
        while m < len(data) and not ok(m, q):
            m += 1
        R.append(m)
    if nb:
        R[-1] = len(data)
    return R


# ---- 2. tables ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def pass_tables(name, big=False):
    """stream_reader_cases.tables(name, big) with what a pass cut needs: dict(tiles, datas, nbs, Rs (pass-granular, shortest_rates_pass), vs, sps,
    bands, ctiles); every array read-only"""
    import oracle as orc
    g = sr.GEOMETRIES[name]
    W, H, Cn, prec, tile, nres = g["case"]
    _, tiles, datas, nbs, _, ctiles = sr.tables(name, big)
    Rs, vs, sps, bands = [], [], [], []
    for ct in ctiles:
        for b in orc.enumerate_blocks(Cn, ct.shape[2], ct.shape[1], nres, g["cb"], g["cb"], 1):
            j = len(vs)
            v = lc.np_block(ct, b)
            sp = pc.sp_mask(v, nbs[j])
            Rs.append(shortest_rates_pass(orc, np.frombuffer(datas[j], np.uint8), nbs[j], int(b["band"]), v, sp))
            for a in (v, sp):
                a.setflags(write=False)
            vs.append(v); sps.append(sp); bands.append(int(b["band"]))
    assert len(vs) == len(nbs)
    return dict(tiles=tiles, datas=datas, nbs=nbs, Rs=Rs, vs=vs, sps=sps, bands=bands, ctiles=ctiles)


# ---- 3. cut families ------------------------------------------------------------------------------------------------------------------------
PASS_FAMILIES = ("P-random", "P-s1", "P-s2", "P-long", "P-claims")
FORCED = (0, 1, 2, -1, None)                                          # P-random's first blocks: q = 0, 1, 2, points - 1, points
BIG_CUTS = (1, 2, 3, 44, 45, 46, 89, 90, 91)
BIG_ROUNDS = 3                                                        # three blocks of 31 planes: nine cuts in three streams


def _inside(nb, s, rng):
    """a cut with s passes of a plane below p whole ones, where the block has two planes; else everything"""
    return 3 * int(rng.integers(1, nb)) - 2 + s if nb >= 2 else pc.points(nb)


@functools.lru_cache(None)
def pass_family(geom, fam):
    """-> dict(qs: the header's pass count per block, lengths: the body bytes per block, edits: {block: (passes added, ZeroBitPlanes added)},
    claims: {block: "passes" | "zbp"}, moved / fallback: P-long's counts).  None of them is a set of cuts an allocator returns:
    P-random  q random in 0 ... points(nb); 0, 1, 2, points - 1 and points on the first five blocks
    P-s1      every block with two planes cut behind a SigProp pass
    P-s2      every block with two planes cut behind a MagRef pass
    P-long    q random in 1 ... points(nb), the body data[:L] with L random in R[q] ... len(data): another encoder ends a pass elsewhere.  Where
              decode_passes of those bytes is not coarse_pass(v, nb, q, sp) L moves to the next length where it is (the whole codeword always is)
    P-claims  P-random's cuts, and in every packet the first block with bytes is whole and its header says one or two passes more than it has
              (s > 0 below plane 0: floor = 0, pfloor = 0, numbps = coded); in the frame's last packet that holds one, another block is cut at
              nb - 1 planes and a SigProp pass while its ZeroBitPlanes, two higher than its planes say, leave room for nb - 2 (mb - zbp < coded:
              floor = 0, pfloor = 0, numbps = coded = nb - 1 -- every one of them decoded to the end, from the bytes of the cut)"""
    T = pass_tables(geom)
    nbs, Rs, datas = T["nbs"], T["Rs"], T["datas"]
    rng = np.random.default_rng(9100 + sr.GEOMETRIES[geom]["seed"] + PASS_FAMILIES.index(fam))
    n = len(nbs)
    qs, edits, claims, moved, fallback = [], {}, {}, 0, 0
    for j, nb in enumerate(nbs):
        last = pc.points(nb)
        if fam in ("P-random", "P-claims"):
            q = int(rng.integers(0, last + 1))
            if j < len(FORCED):
                q = last if FORCED[j] is None else (max(last - 1, 0) if FORCED[j] < 0 else min(FORCED[j], last))
        elif fam == "P-s1":
            q = _inside(nb, 1, rng)
        elif fam == "P-s2":
            q = _inside(nb, 2, rng)
        elif fam == "P-long":
            q = int(rng.integers(1, last + 1)) if last else 0
        else:
            raise ValueError(fam)
        qs.append(q)
    lengths = [int(Rs[j][qs[j]]) if qs[j] else 0 for j in range(n)]
    if fam == "P-long":
        for j, nb in enumerate(nbs):
            if not lengths[j]:
                continue
            h, w = T["vs"][j].shape
            want = pc.coarse_pass(T["vs"][j], nb, qs[j], T["sps"][j])
            first = L = int(rng.integers(lengths[j], len(datas[j]) + 1))
            while L <= len(datas[j]) and not np.array_equal(decode_passes(datas[j][:L], nb, T["bands"][j], w, h, pc.pfloor_of(nb, qs[j])), want):
                L += 1
            if L > len(datas[j]):
                L = lengths[j]
                fallback += 1
            moved += int(L != first)
            lengths[j] = L
    if fam == "P-claims":
        lowered = None
        for packets in T["tiles"]:
            for pk in packets:
                have = [j for j in pk if nbs[j] >= 1 and len(datas[j])]
                if have:
                    a = have[0]
                    qs[a], lengths[a] = pc.points(nbs[a]) + 1 + len(claims) % 2, len(datas[a])
                    claims[a] = "passes"
                    two = [j for j in have[1:] if nbs[j] >= 2 and Rs[j][3 * nbs[j] - 4]]
                    if two:
                        lowered = two[-1]
        assert lowered is not None
        qs[lowered] = 3 * nbs[lowered] - 4                             # nb - 1 whole planes and a SigProp pass ...
        lengths[lowered], edits[lowered] = int(Rs[lowered][qs[lowered]]), (0, 2)       # ... under a header that leaves room for nb - 2 planes
        claims[lowered] = "zbp"
    return dict(qs=qs, lengths=lengths, edits=edits, claims=claims, moved=moved, fallback=fallback)


def big_family(rnd):
    """the 31-plane table set: its three blocks of 31 planes cut at BIG_CUTS[3 rnd ...], the blocks of one plane whole, the empty ones at 0"""
    T = pass_tables("b", True)
    qs, i = [], 0
    for nb in T["nbs"]:
        if nb == 31:
            qs.append(BIG_CUTS[(3 * rnd + i) % len(BIG_CUTS)])
            i += 1
        else:
            qs.append(pc.points(nb))
    assert i == 3
    return dict(qs=qs, lengths=[int(T["Rs"][j][q]) if q else 0 for j, q in enumerate(qs)], edits={}, claims={}, moved=0, fallback=0)


# ---- 4. streams -----------------------------------------------------------------------------------------------------------------------------
def tile_offsets(stream, ntiles):
    """[tiles + 1]: where every tile-part of a composed stream starts, by its Psot"""
    offs = [0]
    for _ in range(ntiles):
        offs.append(offs[-1] + int.from_bytes(stream[offs[-1] + 6:offs[-1] + 10], "big"))
    assert offs[-1] == len(stream)
    return offs


def compose_cut(t2ref, T, F, sop, eph):
    """pass_cases.compose_kept_passes of a family: the header's pass count F.qs[j], the body datas[j][:F.lengths[j]], and F.edits' header fields
    through stream_reader_cases.header_shim -> (stream, tile_offs)"""
    n = len(T["nbs"])
    Rs = [{F["qs"][j]: F["lengths"][j]} for j in range(n)]             # (compose_kept_passes reads R[j][q[j]] alone)
    order = [j for packets in T["tiles"] for pk in packets for j in pk]
    shim = sr.header_shim(t2ref, {order.index(j): e for j, e in F["edits"].items()})
    stream = pc.compose_kept_passes(shim, T["tiles"], T["datas"], T["nbs"], Rs, F["qs"], sop, eph)
    return stream, tile_offsets(stream, len(T["tiles"]))


@functools.lru_cache(None)
def pass_stream(geom, fam, marks):
    """(stream, tile_offs, the family) of a pass family on a geometry"""
    import t2ref
    F = pass_family(geom, fam)
    return compose_cut(t2ref, pass_tables(geom), F, marks, marks) + (F,)


@functools.lru_cache(None)
def big_stream(rnd, marks):
    import t2ref
    F = big_family(rnd)
    return compose_cut(t2ref, pass_tables("b", True), F, marks, marks) + (F,)


# ---- 5. what the device must make of a stream ---------------------------------------------------------------------------------------------------
def expected_coeffs(T, tab, skip_planes=0):
    """{block: int32 [h, w]}: decode_passes of every block's bytes in `tab` (stream_reader_cases.block_tables_pass: {block: (codeword, pfloor,
    numbps)}), max(3 skip_planes, pfloor) passes short; an empty or absent block: zeros"""
    out = {}
    for j, v in enumerate(T["vs"]):
        h, w = v.shape
        if j not in tab or not tab[j][0]:
            out[j] = np.zeros((h, w), np.int32)
            continue
        data, pfloor, numbps = tab[j]
        out[j] = decode_passes_cached(bytes(data), numbps, T["bands"][j], w, h, max(3 * skip_planes, pfloor))
    return out


def whole_plane_coeffs(T, tab):
    """the same for the older reader's tables ({block: (codeword, floor, numbps)}): floor whole planes short"""
    return expected_coeffs(T, {j: (d, 3 * fl, nb) for j, (d, fl, nb) in tab.items()})


def partial_blocks(tab):
    """the blocks of `tab` that the decoder stops inside a plane: bytes and a pfloor that is no multiple of 3"""
    return [j for j, (data, pfloor, numbps) in tab.items() if data and pfloor % 3]
