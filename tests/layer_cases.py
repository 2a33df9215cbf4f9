"""The yardstick of the quality layers of the closed-loop MQ codec (the j2k_*_layers calls), importable without a GPU: tests/test_layer_cases.py
checks it on the CPU, tests/test_gpu_layers.py holds the device against it bit for bit.  DESIGN.md 7 has the format in words.

Block j has nb planes, the rate table R[0 ... nb] of tests/rate_cases.py and its codeword `data`.  An L-layer stream gives it cumulative cuts
P_0 <= ... <= P_(L-1) <= nb (planes kept up to and including layer l), normalised so that no layer adds passes without bytes:

    Q_(-1) = 0,   Q_l = P_l if R[P_l] > R[Q_(l-1)] else Q_(l-1)

In layer l the block contributes iff Q_l > Q_(l-1): the bytes data[R[Q_(l-1)] : R[Q_l]] and passes_of(Q_l) - passes_of(Q_(l-1)) passes.
first = its first contributing layer, or L.

Tile-part: SOT | SOD (14 bytes), then the tile's packet sequence (one packet per (component, resolution) with blocks) once per layer, the layer
outermost, all written by ONE oracle/t2ref.PacketEncoder(len_bits=5) fed per-layer CodeBlocks (data = the increment, included_in_layers = first,
zero_bit_planes = 31 - nb, num_passes = the increment's).  That encoder then writes, per block of a packet that holds data: at layer 0
unary(first); above it one bit "contributes"; for a contributing block unary(31 - nb) iff l == first, the pass code and the length of the
increment.  SOP carries the layer in its sequence field.

Reader (read_layers): the reference's decode_packet_header cannot read this (it expects ZeroBitPlanes at every inclusion above layer 0 and takes
bodies at the first inclusion only), so the header walk is restated here on t2ref's ByteStuffingReader and PacketDecoder's field decoders.
first comes from layer 0's unary where layer 0's packet holds data; a layer-0 packet WITHOUT data (presence bit 0) carries no unary at all, so
the rule that covers both is: at l > 0, ZeroBitPlanes follows the "contributes" bit iff the block has not contributed in an earlier layer --
on every stream the composer writes that is exactly l == first.  A unary value >= the layers being read just means "not in what is read".
Passes and lengths accumulate; every contributing (layer, block) is one body segment; a contribution of length 0, which no writer makes, counts
for the ZeroBitPlanes rule and adds neither a segment nor its passes; floor and plane count are rate_cases.floors_from_header on the sums.
tests/stream_reader_cases.py has the same reader with a verdict per tile in the place of an exception."""
import rate_cases as rc

MAX_LAYERS = 32


# ---- cuts -----------------------------------------------------------------------------------------------------------------------------------
def normalise(R, cuts):
    """cumulative cuts P_0 ... P_(L-1) of one block -> Q_0 ... Q_(L-1)"""
    out, q = [], 0
    for p in cuts:
        p = int(p)
        if int(R[p]) > int(R[q]):
            assert p > q, "R is non-decreasing"
            q = p
        out.append(q)
    return out


def segments(R, cuts):
    """-> ([(lo, hi, passes) per layer; lo == hi: the block does not contribute], first contributing layer or L)"""
    Q = normalise(R, cuts)
    segs, first, q = [], len(Q), 0
    for l, ql in enumerate(Q):
        if ql > q:
            segs.append((int(R[q]), int(R[ql]), rc.passes_of(ql) - rc.passes_of(q)))
            first = min(first, l)
        else:
            segs.append((int(R[q]), int(R[q]), 0))
        q = ql
    return segs, first


def allocate_layers(Rs, Ds, nbs, ws, budgets):
    """layer l = rate_cases.allocate(..., budgets[l]) unchanged -> (kept [L][n], chosen [L]).  Budgets are cumulative and non-decreasing; "the
    smallest lambda that fits" then makes the cuts monotone in l, asserted here."""
    assert 1 <= len(budgets) <= MAX_LAYERS and all(b >= 0 for b in budgets) and all(a <= b for a, b in zip(budgets, budgets[1:]))
    kept, chosen = [], []
    for b in budgets:
        ps, c = rc.allocate(Rs, Ds, nbs, ws, int(b))
        if kept:
            assert all(p >= q for p, q in zip(ps, kept[-1])), "cuts fell with a larger budget"
        kept.append([int(p) for p in ps]); chosen.append(int(c))
    return kept, chosen


# ---- streams --------------------------------------------------------------------------------------------------------------------------------
def tile_head(index, psot):
    return bytes([0xFF, 0x90, 0x00, 0x0A, (index >> 8) & 0xFF, index & 0xFF, (psot >> 24) & 0xFF, (psot >> 16) & 0xFF, (psot >> 8) & 0xFF, psot & 0xFF,
                  0x00, 0x01, 0xFF, 0x93])


def compose(t2ref, tiles, datas, nbs, Rs, kept, sop, eph, tile_first=0):
    """tiles: per tile its packets, a packet = the list of its block numbers (the plan's job order); datas[j]: block j's codeword; kept[l][j]:
    the cumulative cuts.  -> (stream bytes, tile_offs [tiles + 1], layer_offs [tiles * L]: where layer l of tile t ENDS)"""
    L = len(kept)
    segs = {j: segments(Rs[j], [kept[l][j] for l in range(L)]) for pk_t in tiles for pk in pk_t for j in pk}
    out, tile_offs, layer_offs = bytearray(), [], []
    for t, packets in enumerate(tiles):
        enc = t2ref.PacketEncoder(len_bits=5)
        ends = []
        for l in range(L):
            for pk in packets:
                blocks = []
                for j in pk:
                    (lo, hi, npass), first = segs[j][0][l], segs[j][1]
                    blocks.append(t2ref.CodeBlock(bytes(bytearray(datas[j][lo:hi])), first, max(31 - int(nbs[j]), 0), npass))
                enc.encode_packet(t2ref.Precinct([blocks]), l, sop, eph)
            ends.append(14 + len(enc.out))
        tile_offs.append(len(out))
        layer_offs += [len(out) + e for e in ends]
        out += tile_head(tile_first + t, 14 + len(enc.out)) + bytes(enc.out)
    tile_offs.append(len(out))
    return bytes(out), tile_offs, layer_offs


def compose_kept(t2ref, tiles, datas, nbs, Rs, ps, sop, eph, tile_first=0):
    """the EXISTING closed-loop composition of one set of cuts (j2k_plan_encode_tile_parts_kept; closed_loop_ref.oracle_frame's packet loop with the
    blocks cut): body data[:R[p]], 3 p - 2 passes, "in no layer" = 1 for a block without bytes"""
    out = bytearray()
    for t, packets in enumerate(tiles):
        enc = t2ref.PacketEncoder(len_bits=5)
        for pk in packets:
            blocks = []
            for j in pk:
                ln = int(Rs[j][ps[j]]) if ps[j] > 0 else 0
                blocks.append(t2ref.CodeBlock(bytes(bytearray(datas[j][:ln])), 1 if ln == 0 else 0, max(31 - int(nbs[j]), 0), rc.passes_of(ps[j]) if ln else 0))
            enc.encode_packet(t2ref.Precinct([blocks]), 0, sop, eph)
        out += tile_head(tile_first + t, 14 + len(enc.out)) + bytes(enc.out)
    return bytes(out)


def read_layers(t2ref, stream, tile_offs, tiles, k, sop, eph, tile_first=0):
    """the first k layers of every tile-part -> {block: dict(zbp, passes, segs = [(offset in stream, length)], floor, numbps)}.  The tile-part's
    end comes from Psot; what follows layer k - 1 is not looked at.  Raises t2ref.EOF where header bits or body bytes run out."""
    out = {}
    for t, packets in enumerate(tiles):
        a = int(tile_offs[t])
        head = bytes(stream[a:a + 14])
        psot = int.from_bytes(head[6:10], "big")
        assert head[:4] == b"\xff\x90\x00\x0a" and int.from_bytes(head[4:6], "big") == (tile_first + t) & 0xFFFF and head[12:] == b"\xff\x93"
        assert a + psot <= len(stream) and psot >= 14
        dec = t2ref.PacketDecoder(bytes(stream[a + 14:a + psot]), len_bits=5, seated=True)
        st = {j: dict(zbp=None, passes=0, segs=[]) for pk in packets for j in pk}
        for l in range(k):
            for pk in packets:
                if sop and dec.pos + 6 <= len(dec.buf) and dec.buf[dec.pos] == 0xFF and dec.buf[dec.pos + 1] == 0x91:
                    dec.pos += 6
                dec.bio.rpos, dec.bio.cnt = dec.pos, 0
                lens = []
                if dec.bio.read_bit() == 1:
                    for j in pk:
                        s = st[j]
                        if l == 0:
                            inc = dec.decode_tag_tree_value() == 0
                        else:
                            inc = dec.bio.read_bit() == 1
                        if not inc:
                            continue
                        if s["zbp"] is None:                         # its first contribution: ZeroBitPlanes
                            s["zbp"] = dec.decode_tag_tree_value()
                        npass = dec.decode_num_passes()
                        lens.append((j, dec.decode_length()))
                        if lens[-1][1]:                              # a contribution of length 0 (no writer makes one) adds no passes: DESIGN.md 7
                            s["passes"] += npass
                dec.pos = dec.bio.rpos
                if eph and dec.pos + 2 <= len(dec.buf) and dec.buf[dec.pos] == 0xFF and dec.buf[dec.pos + 1] == 0x92:
                    dec.pos += 2
                for j, n in lens:
                    if dec.pos + n > len(dec.buf):
                        raise t2ref.EOF("unexpected end of packet data")
                    if n:
                        st[j]["segs"].append((a + 14 + dec.pos, n))
                    dec.pos += n
        for j, s in st.items():
            if s["zbp"] is None or not s["segs"]:
                s["floor"], s["numbps"] = 0, 0
            else:
                s["floor"], s["numbps"] = rc.floors_from_header(s["zbp"], s["passes"])
        out.update(st)
    return out


def keep_layers(stream, tile_offs, layer_offs, L, k):
    """the stream cut to its first k layers: every tile-part ends after layer k - 1, Psot patched -> (bytes, tile_offs)"""
    assert 1 <= k <= L and len(layer_offs) == (len(tile_offs) - 1) * L
    out, offs = bytearray(), []
    for t in range(len(tile_offs) - 1):
        a, b = int(tile_offs[t]), int(layer_offs[t * L + k - 1])
        part = bytearray(stream[a:b])
        part[6:10] = (b - a).to_bytes(4, "big")
        offs.append(len(out))
        out += part
    offs.append(len(out))
    return bytes(out), offs


# ---- geometry and tables without a device --------------------------------------------------------------------------------------------------
def packets_of(jobs, first=0):
    """oracle.enumerate_blocks' jobs of ONE tile -> its packets (lists of block numbers from `first` on): a new packet where the component or the
    resolution changes"""
    out = []
    for i, b in enumerate(jobs):
        if i == 0 or (int(b["comp"]), int(b["res"])) != (int(jobs[i - 1]["comp"]), int(jobs[i - 1]["res"])):
            out.append([])
        out[-1].append(first + i)
    return out


def shortest_rates(oracle, data, nb, band, v):
    """a rate table with the prefix property made on the CPU: R[p] = the shortest prefix not below R[p - 1] whose decode has the first p planes
    right (rate_cases.prefix_ok), R[0] = 0, R[nb] = len(data).  (The device's own table is its encoder's business; this one lets CPU tests and the
    golden streams have cuts without a device.)"""
    R = [0]
    for p in range(1, nb + 1):
        m = R[-1]
        while m < len(data) and not rc.prefix_ok(oracle, data, m, nb, band, v, p):
            m += 1
        R.append(m)
    if nb:
        R[nb] = len(data)
    return R


# ---- the pinned streams (tests/golden/closed_loop_layers_v1.json) ----------------------------------------------------------------------------
# small gray frames with 8 x 8 / 16 x 16 blocks, so that shortest_rates stays cheap: (W, H, components, precision, tile, resolutions), cb, budgets
# as fractions of the uncut body bytes (None: 2^62), markers
GOLDEN_FILE = "closed_loop_layers_v1.json"
GOLDEN_CASES = [
    dict(name="layers3_gray_40x24_bare", case=(40, 24, 1, 8, (0, 0), 3), cb=8, budgets=(0.15, 0.5, None), marks=False, seed=401),
    dict(name="layers2_empty_first_gray_48x20_tiled_sop_eph", case=(48, 20, 1, 8, (32, 16), 2), cb=16, budgets=(0.0, None), marks=True, seed=402),
]


def golden_tables(case, orc):
    """(pix uint8 [H, W], tiles, datas, nbs, Rs, Ds, ws, the oracle's coefficient tiles) of a golden case: Mallat coefficients and codewords by the oracle, R by shortest_rates"""
    import closed_loop_ref as ref
    import mallat_cases as mc
    W, H, Cn, prec, tile, nres = case["case"]
    pix, _, _, planes = ref.pixel_frame(mc.PIX_FORMAT[(Cn, prec)], W, H, case["seed"], orc, noise=(1 << prec) // 16)
    ctiles = mc.forward_frame(orc, planes, tile, prec, nres, True, 0)
    wts = rc.default_weights(Cn, nres, True)
    tiles, datas, nbs, Rs, Ds, ws = [], [], [], [], [], []
    for ct in ctiles:
        jobs = orc.enumerate_blocks(Cn, ct.shape[2], ct.shape[1], nres, case["cb"], case["cb"], 1)
        tiles.append(packets_of(jobs, len(datas)))
        for b in jobs:
            v = np_block(ct, b)
            data, nb = orc.t1_encode(v, int(b["w"]), int(b["h"]), int(b["band"]))
            datas.append(bytes(bytearray(data))); nbs.append(int(nb))
            Rs.append(shortest_rates(orc, data, nb, int(b["band"]), v))
            Ds.append(rc.distortion(v, nb))
            ws.append(float(wts[int(b["comp"]), int(b["res"]), int(b["band"])]))
    return pix, tiles, datas, nbs, Rs, Ds, ws, ctiles


def np_block(ct, b):
    import numpy as np
    return np.ascontiguousarray(ct[int(b["comp"]), int(b["y0"]):int(b["y0"]) + int(b["h"]), int(b["x0"]):int(b["x0"]) + int(b["w"])]).astype(np.int32)


def golden_budgets(case, Rs, nbs):
    total = sum(int(R[nb]) for R, nb in zip(Rs, nbs))
    return [1 << 62 if f is None else int(total * f) for f in case["budgets"]]


def golden_stream(case, orc, t2ref):
    """-> (pix, tables, kept, (stream, tile_offs, layer_offs))"""
    tab = golden_tables(case, orc)
    pix, tiles, datas, nbs, Rs, Ds, ws, _ = tab
    kept, _ = allocate_layers(Rs, Ds, nbs, ws, golden_budgets(case, Rs, nbs))
    return pix, tab, kept, compose(t2ref, tiles, datas, nbs, Rs, kept, case["marks"], case["marks"])
