"""The closed-loop packet readers on streams this library's encoder never writes (j2k_plan_decode_tile_parts_floors: truncated=True;
j2k_plan_decode_tile_parts_layers: layers=k; j2k_plan_decode_tile_parts_pfloors: pfloors=True / pass_cuts=True, its streams in
tests/pass_stream_cases.py; j2k_plan_decode_frame_pixels_area on top of each), importable without a GPU:
tests/test_stream_reader_cases.py checks this file on the CPU, tests/test_gpu_stream_readers.py holds the device against it bit for bit.

Three small geometries (GEOMETRIES), their tables made as layer_cases.golden_tables makes them (codewords by the oracle, R by shortest_rates), a
fourth table set on geometry b whose blocks have 31, 1 and 0 bit planes; hand-made cut families (families()) that rate_cases.allocate never
returns; read_tiles(), the non-raising reader with a verdict per tile; damage(), the deterministic damage kinds; damaged_copies(), the very
copies both test files use."""
import functools

import numpy as np

import closed_loop_ref as ref
import layer_cases as lc
import mallat_cases as mc
import pass_cases as pc
import rate_cases as rc

# (W, H, components, precision, tile, resolutions), code-block size, seed
GEOMETRIES = {
    "a": dict(case=(40, 24, 1, 8, (16, 16), 3), cb=8, seed=511),       # 6 tiles, ragged last column and row, 42 blocks
    "b": dict(case=(48, 20, 1, 8, (0, 0), 2), cb=16, seed=512),        # one tile, two packets
    "c": dict(case=(33, 17, 3, 12, (32, 16), 3), cb=16, seed=513),     # components x resolutions in the packet order; tiles 1 wide / 1 high
}
LAYER_COUNTS = (1, 2, 6, 31, 32)                                        # the k a stream of L layers is read with: those <= L


@functools.lru_cache(None)
def tables(name, big=False):
    """(planes int32 [C, H, W], tiles, datas, nbs, Rs, the oracle's coefficient tiles) of a geometry.  big (geometry b only): the coefficient tile
    replaced so that the blocks have, by block number mod 3, 31 bit planes (one sample of magnitude >= 2^30 among small ones), 1 and 0"""
    import oracle as orc
    g = GEOMETRIES[name]
    W, H, Cn, prec, tile, nres = g["case"]
    planes = ref.frame_n(W, H, Cn, prec, g["seed"])
    ctiles = mc.forward_frame(orc, planes, tile, prec, nres, True, 0)
    if big:
        rng = np.random.default_rng(g["seed"] + 1000)
        ctiles = [np.zeros_like(ct) for ct in ctiles]
        for ct in ctiles:
            for j, b in enumerate(orc.enumerate_blocks(Cn, ct.shape[2], ct.shape[1], nres, g["cb"], g["cb"], 1)):
                w, h, c = int(b["w"]), int(b["h"]), int(b["comp"])
                v = np.zeros((h, w), np.int64)
                if j % 3 == 0:
                    v = rng.integers(-3, 4, (h, w)) * (rng.random((h, w)) < 0.2)
                    v[int(rng.integers(0, h)), int(rng.integers(0, w))] = (1 << 30) + int(rng.integers(0, 1 << 30))
                    v[h - 1, 0] = -((1 << 31) - 1)
                elif j % 3 == 1:
                    v = rng.integers(-1, 2, (h, w))
                    v[0, 0] = 1
                ct[c, int(b["y0"]):int(b["y0"]) + h, int(b["x0"]):int(b["x0"]) + w] = v.astype(np.int32)
    tiles, datas, nbs, Rs = [], [], [], []
    for ct in ctiles:
        jobs = orc.enumerate_blocks(Cn, ct.shape[2], ct.shape[1], nres, g["cb"], g["cb"], 1)
        tiles.append(lc.packets_of(jobs, len(datas)))
        for b in jobs:
            v = lc.np_block(ct, b)
            data, nb = orc.t1_encode(v, int(b["w"]), int(b["h"]), int(b["band"]))
            datas.append(bytes(bytearray(data))); nbs.append(int(nb))
            Rs.append(lc.shortest_rates(orc, data, nb, int(b["band"]), v))
    return planes, tiles, datas, nbs, Rs, ctiles


# ---- cut families ---------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("L32-mod5", "L1-random", "L2-empty0-tile", "L2-empty0-all", "L3-free-planes", "L32-all-in-0")


def family(fam, tiles, nbs, Rs, seed=0):
    """-> kept [L][n], cumulative and monotone in l, none of them a set of cuts rate_cases.allocate returns for budgets:
    L32-mod5        by block number mod 5: first contribution in layer 31 only; contributions in layers 0, 5 and 31 and in none between; never;
                    one more plane every layer until nb; three random (layer, plane) points
    L1-random       one layer, random cuts, 0 and nb among them: the truncated format (compose_kept)
    L2-empty0-tile  layer 0 empty for every block of tile 0 (random cuts elsewhere), layer 1 everything
    L2-empty0-all   layer 0 empty everywhere
    L3-free-planes  where the block has a plane p with R[p] == R[p - 1]: the cuts p - 1, p, another such plane -- what normalise folds away
    L32-all-in-0    every block complete in layer 0: the layers 1 ... 31 are empty packets"""
    rng = np.random.default_rng(9000 + seed + FAMILIES.index(fam))
    n = len(nbs)
    L = int(fam[1:fam.index("-")])
    kept = [[0] * n for _ in range(L)]
    tile0 = {j for pk in tiles[0] for j in pk}
    for j, nb in enumerate(nbs):
        if fam == "L32-mod5":
            m = j % 5
            if m == 0:
                col = [0] * 31 + [nb]
            elif m == 1:
                p1, p2 = (nb + 2) // 3, (2 * nb + 2) // 3
                col = [p1] * 5 + [p2] * 26 + [nb]
            elif m == 2:
                col = [0] * 32
            elif m == 3:
                col = [min(l + 1, nb) for l in range(32)]
            else:
                ls = sorted(int(x) for x in rng.choice(32, 3, replace=False))
                ps = sorted(int(x) for x in rng.integers(0, nb + 1, 3))
                col = [max([p for l_, p in zip(ls, ps) if l_ <= l], default=0) for l in range(32)]
        elif fam == "L1-random":
            col = [[0, nb, int(rng.integers(0, nb + 1))][j % 3 if j < 6 else 2]]
        elif fam == "L2-empty0-tile":
            col = [0 if j in tile0 else int(rng.integers(0, nb + 1)), nb]
        elif fam == "L2-empty0-all":
            col = [0, nb]
        elif fam == "L3-free-planes":
            free = [p for p in range(1, nb + 1) if Rs[j][p] == Rs[j][p - 1]]
            if free:                                                 # layer 1 adds the free plane p to layer 0's p - 1: passes without bytes
                p = int(rng.choice(free))
                col = [p - 1, p, max(p, int(rng.choice(free)))]
            else:
                col = sorted(int(x) for x in rng.integers(0, nb + 1, 3))
        else:
            col = [nb] * 32
        assert len(col) == L and all(a <= b for a, b in zip(col, col[1:])) and col[-1] <= nb
        for l in range(L):
            kept[l][j] = int(col[l])
    return kept


def expected(Rs, nbs, kept, k):
    """what a reader of the first k layers must find per block, from layer_cases.segments / rate_cases.floors_from_header alone:
    [(segment lengths, passes, floor, numbps, codeword bytes R[Q])]"""
    out = []
    L = len(kept)
    for j, nb in enumerate(nbs):
        segs, first = lc.segments(Rs[j], [kept[l][j] for l in range(L)])
        lens = [hi - lo for lo, hi, _ in segs[:k] if hi > lo]
        passes = sum(p for _, _, p in segs[:k])
        if lens:
            floor, numbps = rc.floors_from_header(31 - nb, passes)
        else:
            floor, numbps = 0, 0
        out.append((lens, passes, floor, numbps, sum(lens)))
    return out


# ---- the reader with a verdict per tile -------------------------------------------------------------------------------------------------------
def _tile_chain(stream, at, want_index):
    """the tile-part head at stream[at:] -> (first packet byte, end) or the reason it is refused (t2_tile_chain)"""
    n = len(stream)
    if at >= n or n - at < 14:
        return "head: no room for SOT + SOD"
    b = stream[at:at + 14]
    if b[0] != 0xFF or b[1] != 0x90:
        return "head: no SOT marker"
    lsot, isot, psot = b[2] << 8 | b[3], b[4] << 8 | b[5], int.from_bytes(bytes(b[6:10]), "big")
    if lsot != 10:
        return "head: Lsot is not 10"
    if isot != want_index & 0xFFFF:
        return "head: Isot is not the tile's number"
    stop = at + psot if psot else n
    if stop > n or stop < at + 14:
        return "head: Psot outside the stream or below 14"
    p = at + 12
    if b[12] == 0xFF and b[13] == 0x93:
        return p + 2, stop
    while True:
        if p + 2 > stop or stream[p] != 0xFF:
            return "head: the marker walk left the tile-part or met no marker"
        if stream[p + 1] == 0x93:
            return p + 2, stop
        if p + 4 > stop:
            return "head: a marker segment without a length"
        ln = stream[p + 2] << 8 | stream[p + 3]
        if ln < 2:
            return "head: a marker segment shorter than its length field"
        p += 2 + ln


def read_tiles(t2ref, stream, tile_offs, tiles, k, sop, eph, tile_first=0):
    """The first k layers of every tile-part of `stream` (the caller's bytes, cut to the length the device is told) -> one verdict per tile:
    dict(ok, why, blocks = {block: dict(zbp, passes, segs = [(offset in stream, length)], floor, numbps, pfloor, dropped)}).  It never raises.  k = 1
    on an L = 1 stream is the reader of the truncated format.  The field decoders are layer_cases.read_layers' (oracle/t2ref.py); on every
    stream that one accepts, this one accepts every tile and returns the same records.

    WHEN A TILE IS REFUSED (ok = False; `why` says which rule; the device reports J2K_ERR_INVALID_ARG for the frame and promises nothing about
    the refused tile's table entries beyond the invariants at the end):
      1. the tile-part head, at tile_offs[t], or without tile_offs at 0 for the first tile and at the end of the tile-part before for the others:
         fewer than 14 bytes left in the stream; no FF90; Lsot != 10; Isot != the tile's number (tile_first + t, 16 bits); the end
         stop = at + Psot (Psot = 0: the stream's end) beyond the stream or below at + 14; bytes 12, 13 are FF93 (SOD), or else marker segments
         are stepped over by their lengths from at + 12 until FF93 -- a byte that is not FF where a marker must stand, a marker or a length
         field that does not fit below `stop`, a length below 2 refuse.  TPsot and TNsot are not looked at.  The packets are the bytes
         from behind SOD to `stop`; nothing outside them is read.
      2. without tile_offs every tile-part behind a refused one is refused too (its place is not known); with tile_offs each is on its own.
      3. header bits run out: a field that needs a bit when the packets' bytes are used up (the presence bit of a packet that starts at
         `stop` included).
      4. body bytes run out: the lengths of a packet's contributing blocks add up to more than is left up to `stop`.
    SOP (6 bytes) and EPH (2 bytes) are stepped over where they stand and fit, and are not required.

    WHAT A READ TILE HOLDS.  Layer 0: unary value per block, 0 = contributes.  Layer l > 0: one bit.  ZeroBitPlanes follows iff the block has not
    contributed in an earlier layer; then the pass code and the 5-bit length-of-length and the length (at most 31 bits: with this field width a
    length wider than 32 bits cannot be written, and the sum of a block's segments stays below 2^32 for every stream shorter than 128 MiB -- the
    device's test on the sum cannot fire in these tests).  A CONTRIBUTION OF LENGTH 0 -- no writer makes one, the format of DESIGN.md 7 was silent --
    counts as a contribution for the ZeroBitPlanes rule and adds neither a segment nor its passes.  A block without a segment is empty:
    length 0, numbps = floor = pfloor = 0.  Otherwise (floor, numbps) = rate_cases.floors_from_header(zbp, sum of passes).
      5. a block whose floor + coded planes exceeds 31 (only possible with more than 91 passes) is DROPPED: it is empty in the tables (pfloor = 0 too), dropped = True,
         the frame's status is J2K_ERR_INVALID_ARG, and every other block of the tile and of the frame keeps its record.
    THE PASS READER (j2k_plan_decode_tile_parts_pfloors) reads the same fields and takes the pass count at its word: with coded = (passes + 2) // 3
    and s = (passes + 2) % 3 it is (pfloor, numbps) = pass_cases.pfloor_from_header(zbp, passes) -- the same numbps, pfloor = 3 floor - s passes left
    undecoded.  Two headers no writer of this library makes are settled here:
      a. floor == 0 with s > 0 -- a header that claims passes below plane 0: pfloor = 0 and numbps = coded; the decoder runs every one of the
         `coded` planes to its end.
      b. mb - zbp < coded -- more coded planes than ZeroBitPlanes leaves room for: floor = 0 (never negative), so pfloor = 0 and numbps = coded.
    The frame's status is J2K_OK iff every tile is read and no block is dropped (frame_ok).

    INVARIANTS of the device's tables on every input: offs + lens <= the dense buffer (layers) or the stream length (floors); numbps <= 31;
    floors <= numbps; lens == 0 implies numbps == floors == 0.  The pass reader: pfloors <= max(3 numbps - 3, 0) in the place of floors <= numbps;
    lens == 0 implies numbps == pfloors == 0."""
    out = []
    at, lost = 0, None
    for t, packets in enumerate(tiles):
        blocks = {j: dict(zbp=None, passes=0, segs=[], floor=0, numbps=0, pfloor=0, dropped=False) for pk in packets for j in pk}
        v = dict(ok=False, why=None, blocks=blocks, done=0, zero_len=0)   # done: packets read to their end (layer-major) before a refusal; zero_len: contributions of length 0
        out.append(v)
        if tile_offs is None and lost is not None:
            v["why"] = "behind a refused tile-part: " + lost
            continue
        head = _tile_chain(stream, int(tile_offs[t]) if tile_offs is not None else at, tile_first + t)
        if isinstance(head, str):
            v["why"] = lost = head
            continue
        start, stop = head
        at = stop
        dec = t2ref.PacketDecoder(bytes(stream[start:stop]), len_bits=5, seated=True)
        try:
            for l in range(k):
                for pk in packets:
                    if sop and dec.pos + 6 <= len(dec.buf) and dec.buf[dec.pos] == 0xFF and dec.buf[dec.pos + 1] == 0x91:
                        dec.pos += 6
                    dec.bio.rpos, dec.bio.cnt = dec.pos, 0
                    got = []
                    if dec.bio.read_bit() == 1:
                        for j in pk:
                            s = blocks[j]
                            inc = (dec.decode_tag_tree_value() == 0) if l == 0 else (dec.bio.read_bit() == 1)
                            if not inc:
                                continue
                            if s["zbp"] is None:
                                s["zbp"] = dec.decode_tag_tree_value()
                            got.append((j, dec.decode_num_passes(), dec.decode_length()))
                    dec.pos = dec.bio.rpos
                    if eph and dec.pos + 2 <= len(dec.buf) and dec.buf[dec.pos] == 0xFF and dec.buf[dec.pos + 1] == 0x92:
                        dec.pos += 2
                    if dec.pos + sum(ln for _, _, ln in got) > len(dec.buf):
                        raise t2ref.EOF("body bytes run out")
                    for j, npass, ln in got:
                        if ln:
                            blocks[j]["segs"].append((start + dec.pos, ln))
                            blocks[j]["passes"] += npass
                        else:
                            v["zero_len"] += 1
                        dec.pos += ln
                    v["done"] += 1
        except t2ref.EOF as e:
            v["why"] = lost = str(e) or "header bits run out"
            continue
        for s in blocks.values():
            if s["zbp"] is not None and s["segs"]:
                s["floor"], s["numbps"] = rc.floors_from_header(s["zbp"], s["passes"])
                s["pfloor"] = pc.pfloor_from_header(s["zbp"], s["passes"])[0]
                assert pc.pfloor_from_header(s["zbp"], s["passes"])[1] == s["numbps"]
                if s["numbps"] > 31:
                    s.update(floor=0, numbps=0, pfloor=0, dropped=True)
        v["ok"] = True
    return out


def frame_ok(verdicts):
    return all(v["ok"] and not any(s["dropped"] for s in v["blocks"].values()) for v in verdicts)


def block_tables(stream, verdicts, floor="floor"):
    """{block: (codeword bytes, floor, numbps)} of the tiles that were read -- a dropped block is empty"""
    out = {}
    for v in verdicts:
        if v["ok"]:
            for j, s in v["blocks"].items():
                data = b"" if s["dropped"] else b"".join(bytes(stream[o:o + ln]) for o, ln in s["segs"])
                out[j] = (data, s[floor], s["numbps"])
    return out


def block_tables_pass(stream, verdicts):
    """the pass reader's: {block: (codeword bytes, pfloor, numbps)}"""
    return block_tables(stream, verdicts, "pfloor")


# ---- damage ---------------------------------------------------------------------------------------------------------------------------------
KINDS = ("body", "header", "head64", "cut", "runs", "offs", "noise")


def damage(rng, stream, tile_offs, segs, kind):
    """a damaged copy of `stream` -> (bytes of the same length, the length the reader is told, tile_offs as Python ints); deterministic in rng.
    segs: [(offset, length)] of the body segments (read_layers' / read_tiles' records), used by `body` only"""
    bad = bytearray(stream)
    total = len(bad)
    n, offs = total, [int(x) for x in tile_offs]
    if kind == "body":                                               # bytes inside body segments only: the tables must not change
        segs = [s for s in segs if s[1] > 0]
        for _ in range(int(rng.integers(1, 4))):
            o, ln = segs[int(rng.integers(0, len(segs)))]
            bad[o + int(rng.integers(0, ln))] ^= int(rng.integers(1, 256))
    elif kind == "header":                                           # 1 to 3 random bytes anywhere
        for _ in range(int(rng.integers(1, 4))):
            bad[int(rng.integers(0, total))] = int(rng.integers(0, 256))
    elif kind == "head64":                                           # the first 64 bytes of one tile-part: SOT, SOD, the first packet headers
        t = int(rng.integers(0, len(offs) - 1))
        for _ in range(int(rng.integers(1, 8))):
            bad[min(offs[t] + int(rng.integers(0, 64)), total - 1)] = int(rng.integers(0, 256))
    elif kind == "cut":                                              # truncation
        n = int(rng.integers(0, total))
    elif kind == "runs":                                             # long unary values / stuffing everywhere
        a = int(rng.integers(0, max(total - 300, 1)))
        ln = int(rng.integers(8, 301))
        fill = 0x00 if int(rng.integers(0, 2)) else 0xFF
        for i in range(a, min(a + ln, total)):
            bad[i] = fill
    elif kind == "offs":                                             # tile-part positions from a hostile caller
        offs[int(rng.integers(0, len(offs)))] = [0, total, total + 12345, 2 ** 62, 2 ** 64 - 1 - int(rng.integers(0, 16))][int(rng.integers(0, 5))]
    elif kind == "noise":                                            # everything random
        bad = bytearray(rng.integers(0, 256, total).astype(np.uint8).tobytes())
    else:
        raise ValueError(kind)
    return bytes(bad), n, offs


# the readers' damaged copies, all on geometry a: (cut family, layers read, copies).  pfloors: the pass reader on pass_stream_cases' random pass cuts
READERS = {"layers32": ("L32-mod5", 32), "layers2": ("L2-empty0-tile", 2), "floors": ("L1-random", 1), "pfloors": ("P-random", 1)}
COPIES = 120
DAMAGE_SEED = {"layers32": 7301, "layers2": 7302, "floors": 7303, "pfloors": 7304}


@functools.lru_cache(None)
def base_stream(geom, fam, marks):
    """(stream, tile_offs, layer_offs, kept) of a family on a geometry's tables, by layer_cases.compose; a pass family (P-...: one layer, kept[0] the
    pass counts) by pass_stream_cases.pass_stream"""
    import t2ref
    if fam.startswith("P-"):
        import pass_stream_cases as ps
        stream, toffs, F = ps.pass_stream(geom, fam, marks)
        return stream, toffs, toffs[1:], [list(F["qs"])]
    _, tiles, datas, nbs, Rs, _ = tables(geom)
    kept = family(fam, tiles, nbs, Rs)
    return lc.compose(t2ref, tiles, datas, nbs, Rs, kept, marks, marks) + (kept,)


def header_shim(t2ref, edits):
    """oracle/t2ref.py's packet writer with single header fields changed: edits = {number of the CodeBlock call, from 0: (passes added,
    ZeroBitPlanes added)} -- well-formed streams whose headers claim what the block does not hold"""
    made = []

    class Shim:
        PacketEncoder, Precinct = t2ref.PacketEncoder, t2ref.Precinct

        @staticmethod
        def CodeBlock(data, incl, zbp, npass):
            dp, dz = edits.get(len(made), (0, 0))
            made.append(None)
            return t2ref.CodeBlock(data, incl, zbp + dz, npass + dp)
    return Shim


def compose_passes(t2ref, tiles, datas, nbs, Rs, kept, sop, eph, block, extra):
    """layer_cases.compose with ONE field changed: the header of block `block`'s first contribution says `extra` passes more than the block has
    -- a well-formed stream whose block claims more than 31 bit planes (rule 5 of read_tiles)"""
    L = len(kept)
    first = lc.segments(Rs[block], [kept[l][block] for l in range(L)])[1]
    assert first < L
    order = [(l, j) for packets in tiles for l in range(L) for pk in packets for j in pk]      # compose's order of CodeBlock calls
    return lc.compose(header_shim(t2ref, {order.index((first, block)): (extra, 0)}), tiles, datas, nbs, Rs, kept, sop, eph)


CRAFTED = 2                     # copies behind the random ones, kind "passes" (compose_passes): random damage did not produce rule 5 in 36000 copies


@functools.lru_cache(None)
def damaged_copies(reader):
    """the COPIES damaged copies of a reader's stream and CRAFTED more, the same in both test files: [dict(it, kind, marks, stream, n, offs, with_offs,
    verdicts)].  Copy `it` < COPIES has kind KINDS[it % 7], SOP + EPH iff (it // 7) is odd, and is read with tile_offs iff its kind is `offs` or
    `it` is odd.  The CRAFTED ones are intact but for one pass count (+ 100 in a block's first contribution)."""
    import t2ref
    fam, k = READERS[reader]
    _, tiles, datas, nbs, Rs, _ = tables("a")
    rng = np.random.default_rng(DAMAGE_SEED[reader])
    out = []
    for it in range(COPIES):
        kind, marks = KINDS[it % len(KINDS)], bool((it // len(KINDS)) & 1)
        stream, toffs, loffs, kept = base_stream("a", fam, marks)
        intact = read_tiles(t2ref, stream, toffs, tiles, k, marks, marks)
        segs = [s for v in intact for b in v["blocks"].values() for s in b["segs"]]
        bad, n, offs = damage(rng, stream, toffs, segs, kind)
        with_offs = kind == "offs" or bool(it & 1)
        verdicts = read_tiles(t2ref, bad[:n], offs if with_offs else None, tiles, k, marks, marks)
        out.append(dict(it=it, kind=kind, marks=marks, stream=bad, n=n, offs=offs, with_offs=with_offs, verdicts=verdicts))
    for c in range(CRAFTED):
        marks = bool(c & 1)
        kept = base_stream("a", fam, marks)[3]
        if fam.startswith("P-"):
            import pass_stream_cases as ps
            F = dict(ps.pass_family("a", fam))
            contributing = [j for j in range(len(nbs)) if F["lengths"][j]]
            block = contributing[(7 + 11 * c) % len(contributing)]
            F["edits"] = {block: (100, 0)}
            bad, offs = ps.compose_cut(t2ref, ps.pass_tables("a"), F, marks, marks)
        else:
            contributing = [j for j in range(len(nbs)) if lc.segments(Rs[j], [kept[l][j] for l in range(len(kept))])[1] < min(k, len(kept))]
            block = contributing[(7 + 11 * c) % len(contributing)]
            bad, offs, _ = compose_passes(t2ref, tiles, datas, nbs, Rs, kept, marks, marks, block, 100)
        verdicts = read_tiles(t2ref, bad, None if marks else offs, tiles, k, marks, marks)
        out.append(dict(it=COPIES + c, kind="passes", marks=marks, stream=bad, n=len(bad), offs=offs, with_offs=not marks, verdicts=verdicts, block=block))
    return out
