// j2k_frame.cpp -- Tier-2 on device buffers and the closed-loop frame codec (C ABI of libj2kgfx.so, include/j2kgfx.h; shared declarations: j2k_host.h): the packet
// and tile-part stage calls, the ONE frame encoder (plan_encode_frame_from_coeff: every encode form is an EncodeRequest) and the ONE frame decoder
// (plan_decode_frame: every decode form is a DecodeRequest), and the device entry points of both -- each checks, fills its request and calls them
#include "j2k_host.h"

using namespace j2k;

// ---- Tier-2 packets on device buffers (t2dev.hip) -------------------------------------------------------------------
extern "C" int j2k_t2_encode_packets_device(j2k_ctx *ctx, const j2k_t2_dev_packet *d_packets, size_t npackets, const j2k_t2_dev_cb *d_cbs, size_t ncbs,
                                            const uint8_t *d_data, int sop, int eph, uint8_t *bio_delay, uint8_t *d_out, size_t cap,
                                            uint64_t *d_offs, size_t *total) {
    if (!ctx || !bio_delay || !d_offs || !total || (npackets && !d_packets) || (ncbs && !d_cbs) || (cap && !d_out)) return J2K_ERR_INVALID_ARG;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "a synchronising call while the context captures a graph");
    if (npackets > ((size_t)1 << 31)) return fail(ctx, J2K_ERR_INVALID_ARG, "too many packets");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t ws = j2k::t2_dev_workspace((long)npackets);
    int r = stage_reserve(ctx, 1, ws + 64);
    if (r != J2K_OK) return r;
    uint64_t *d_res = reinterpret_cast<uint64_t *>((uint8_t *)ctx->stage[1] + ((ws + 15) & ~size_t(15)));
    HIPCHK(ctx, hipMemsetAsync(d_res, 0, 3 * sizeof(uint64_t), ctx->stream));
    HIPCHK(ctx, j2k::launch_t2_encode_packets(ctx->stream, d_packets, (long)npackets, d_cbs, (uint64_t)ncbs, d_data, sop, eph, *bio_delay ? 1 : 0, d_out, (uint64_t)cap,
                                              d_offs, ctx->stage[1], d_res));
    uint64_t res[3] = {0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(res, d_res, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (res[2]) return fail(ctx, J2K_ERR_GO_PANIC, "packet coder: a tag tree of width 0 (the reference divides by it, t2.go:328,348), or a packet whose code-blocks lie outside the table");
    *total = (size_t)res[0];
    if (res[0] > cap) return fail(ctx, J2K_ERR_CAPACITY, "packet coder: the output buffer is smaller than the packets");
    *bio_delay = res[1] ? 1 : 0;
    return J2K_OK;
}

// one packet per (tile-component, resolution) that has code-blocks: a new one where the plane or the resolution changes.  (A
// resolution whose bands are all empty -- a 1-sample-wide tile has no HL / HH -- has no jobs and so no packet: nothing the
// reference's iterator would have produced stands for it, this table is the library's own.)  Closed-loop plans get the
// J2K_T2_* flags: a new coder object at every tile's first packet.
void plan_t2_packets(const j2k_plan *P, int layer, std::vector<j2k_t2_dev_packet> &out, std::vector<int> *tile_packet0) {
    const size_t n = P->blocks.size();
    const int cl = P->spec.closed_loop ? (J2K_T2_WIDE_LEN | J2K_T2_SEATED) : 0;
    for (size_t j = 0; j < n; j++) {
        const j2k_block &b = P->blocks[j];
        const bool new_tile = j == 0 || P->block_tile[j] != P->block_tile[j - 1];
        const bool fresh = new_tile || b.plane != P->blocks[j - 1].plane || P->block_res[j] != P->block_res[j - 1];
        if (new_tile && tile_packet0) while ((int)tile_packet0->size() <= P->block_tile[j]) tile_packet0->push_back((int)out.size());
        if (fresh) {
            int cols = 0;                                      // block columns of the precinct's first band
            for (size_t k = j; k < n && P->blocks[k].plane == b.plane && P->block_res[k] == P->block_res[j] && P->blocks[k].band == b.band && P->blocks[k].y0 == b.y0; k++) cols++;
            out.push_back(j2k_t2_dev_packet{layer, cols, cols, cl | ((cl && new_tile) ? J2K_T2_FRESH : 0), (int64_t)j, 0});
        }
        out.back().ncb++;
    }
    if (tile_packet0) while ((int)tile_packet0->size() <= P->tile_count) tile_packet0->push_back((int)out.size());
}
extern "C" int j2k_plan_t2_packets(const j2k_plan *P, int layer, j2k_t2_dev_packet *packets, size_t cap, size_t *count) {
    if (!P || !count || (cap && !packets)) return J2K_ERR_INVALID_ARG;
    std::vector<j2k_t2_dev_packet> out;
    plan_t2_packets(P, layer, out, nullptr);
    *count = out.size();
    if (cap < out.size()) return J2K_ERR_CAPACITY;
    if (!out.empty()) memcpy(packets, out.data(), out.size() * sizeof(j2k_t2_dev_packet));
    return J2K_OK;
}

extern "C" int j2k_plan_t2_fill_cbs(j2k_plan *P, int mb, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps, j2k_t2_dev_cb *d_cbs) {
    graph_note_plan(P);
    if (!P || !d_offs || !d_lens || !d_numbps || !d_cbs) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, j2k::launch_t2_fill_cbs(ctx->stream, (long)P->blocks.size(), d_offs, d_lens, d_numbps, mb,
                                        (P->spec.coder == J2K_CODER_HT ? 1 : 0) | (P->spec.closed_loop ? 2 : 0), d_cbs));
    return J2K_OK;
}

// PacketDecoder.DecodePacket for a run of packets by one decoder object (t2dec.hip)
extern "C" int j2k_t2_decode_packets_device(j2k_ctx *ctx, const j2k_t2_dev_packet *d_packets, size_t npackets, j2k_t2_dev_cb *d_cbs, size_t ncbs,
                                            const uint8_t *d_data, size_t len, int sop, int eph, j2k_t2_dec_state *st, size_t *packets_done) {
    if (!ctx || !st || !packets_done || (npackets && !d_packets) || (ncbs && !d_cbs) || (len && !d_data)) return J2K_ERR_INVALID_ARG;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "a synchronising call while the context captures a graph");
    if (npackets > ((size_t)1 << 31)) return fail(ctx, J2K_ERR_INVALID_ARG, "too many packets");
    *packets_done = 0;
    if (!npackets) return J2K_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t cb = (j2k::t2_chain_bytes() + 15) & ~size_t(15);
    int r = stage_reserve(ctx, 1, cb + npackets * 8 + 64);
    if (r != J2K_OK) return r;
    std::vector<uint8_t> h(cb);
    j2k::t2_make_chain(h.data(), (uint64_t)len, (long)npackets, *st);
    HIPCHK(ctx, hipMemcpyAsync(ctx->stage[1], h.data(), cb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, j2k::launch_t2_decode_packets(ctx->stream, ctx->stage[1], 1, d_packets, (long)npackets, d_cbs, (uint64_t)ncbs, d_data, sop, eph, 0,
                                              reinterpret_cast<uint64_t *>((uint8_t *)ctx->stage[1] + cb), nullptr));
    HIPCHK(ctx, hipMemcpyAsync(h.data(), ctx->stage[1], cb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    int status = J2K_OK;
    long done = 0;
    j2k::t2_read_chain(h.data(), *st, status, done);
    *packets_done = (size_t)done;
    if (status != J2K_OK) return fail(ctx, status, status == J2K_ERR_GO_PANIC ? "packet decoder: a tag tree of width 0 (the reference divides by it, t2.go:524,547)"
                                                                              : "packet decoder: out of header bits or body bytes, or a packet whose code-blocks lie outside the table");
    return J2K_OK;
}

// ---- the closed-loop frame codec (j2k_params.closed_loop) -------------------------------------------------------------------
int cl_prepare(j2k_plan *P) {
    j2k_ctx *ctx = P->ctx;
    if (!P->spec.closed_loop) return fail(ctx, J2K_ERR_UNSUPPORTED, "the plan was not made with j2k_params.closed_loop: the reference's code-block windows overlap and its packets cannot be read back");
    if (P->d_t2_packets) return J2K_OK;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: the frame codec's tables are made at its first call -- run it once before j2k_ctx_capture_begin");
    std::vector<j2k_t2_dev_packet> pk;
    std::vector<int> tp0;
    plan_t2_packets(P, 0, pk, &tp0);
    const size_t n = P->blocks.size(), np = pk.size();
    std::vector<int32_t> ptile(np ? np : 1, 0);                     // packet -> its tile (packet p ends up 14 (ptile[p] + 1) bytes behind its place among the packets)
    for (int t = 0; t < P->tile_count; t++)
        for (int q = tp0[t]; q < tp0[t + 1]; q++) ptile[(size_t)q] = t;
    int r = upload(ctx, &P->d_tile_packet0, tp0);
    if (r == J2K_OK) r = upload(ctx, &P->d_t2_ptile, ptile);
    auto alloc = [&](void **p, size_t bytes) { first_use_alloc(ctx, r, p, bytes, "hipMalloc (frame codec)"); };
    alloc((void **)&P->d_t2_cbs, n * sizeof(j2k_t2_dev_cb));
    alloc((void **)&P->d_t2_poffs, (np + 1) * 8);
    alloc(&P->d_t2_ws, ((j2k::t2_dev_workspace((long)np) + 15) & ~size_t(15)) + 64);
    alloc(&P->d_t2_chains, (size_t)P->tile_count * j2k::t2_chain_bytes());
    alloc((void **)&P->d_t2_body_base, np * 8);
    alloc(&P->d_t2_par, j2k::t2_par_workspace((long)np, P->tile_count));
    if (r == J2K_OK) { hipError_t e = hipMemsetAsync(P->d_t2_par, 0, j2k::t2_par_workspace((long)np, P->tile_count), ctx->stream); if (e != hipSuccess) r = fail_hip(ctx, e, "hipMemsetAsync"); }
    alloc((void **)&P->d_frame_status, 64);
    if (r == J2K_OK) { hipError_t e = hipMemsetAsync(P->d_frame_status, 0, 64, ctx->stream); if (e != hipSuccess) r = fail_hip(ctx, e, "hipMemsetAsync"); }
    P->t2_npackets = (int)np;
    int max_ncb = 1;
    for (const j2k_t2_dev_packet &q : pk) max_ncb = std::max(max_ncb, (int)q.ncb);
    P->t2_body_slices = std::min(32, max_ncb);                      // wavefronts that share the bodies of one packet (t2_body_kernel)
    if (r == J2K_OK) r = upload(ctx, &P->d_t2_packets, pk);      // (last: its presence says the tables are complete)
    return r;
}

extern "C" size_t j2k_plan_frame_bound(const j2k_plan *P) {
    if (!P || !P->spec.closed_loop) return 0;
    std::vector<j2k_t2_dev_packet> pk;
    plan_t2_packets(P, 0, pk, nullptr);
    return (size_t)P->bytes_cap + 16 * P->blocks.size() + 16 * pk.size() + 14 * (size_t)P->tile_count + 64;
}

// the packets of a frame written where they end up (t2dev.hip: launch_t2_encode_tile_parts).  d_stream + d_offs: the dense block stream, or
// d_offs == NULL: d_stream is the plan's slot buffer as plan_encode_private_slots left it and every block is gathered from its slot
int encode_tile_parts_impl(j2k_plan *P, const uint8_t *d_data, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
                           int sop, int eph, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, const uint8_t *d_kept, const uint32_t *d_rate, int passes) {
    j2k_ctx *ctx = P->ctx;
    const long n = (long)P->blocks.size(), np = P->t2_npackets;
    const int ht = P->spec.coder == J2K_CODER_HT ? 1 : 0;
    uint64_t *d_res = reinterpret_cast<uint64_t *>((uint8_t *)P->d_t2_ws + ((j2k::t2_dev_workspace(np) + 15) & ~size_t(15)));
    HIPCHK(ctx, j2k::launch_t2_fill_cbs(ctx->stream, n, d_offs, d_lens, d_numbps, 31, ht | 2, P->d_t2_cbs, d_res, d_kept, d_rate, passes));
    HIPCHK(ctx, j2k::launch_t2_encode_tile_parts(ctx->stream, P->d_t2_packets, np, P->d_t2_cbs, (uint64_t)n, d_data, sop, eph, d_out, (uint64_t)cap, P->d_t2_poffs,
                                                 P->d_t2_ws, d_res, P->d_t2_ptile, P->d_tile_packet0, P->tile_count, P->tile_first, d_tile_offs, P->d_frame_status,
                                                 d_offs ? nullptr : (P->d_bjobs_alias ? P->d_bjobs_alias : P->d_bjobs), d_offs ? nullptr : (ht ? P->d_maglens : nullptr), ht, P->t2_body_slices));
    return J2K_OK;
}

extern "C" int j2k_plan_encode_tile_parts(j2k_plan *P, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
                                          int sop, int eph, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (!d_stream || !d_offs || !d_lens || !d_numbps || !d_out || !d_tile_offs) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int r = cl_prepare(P);
    if (r != J2K_OK) return r;
    return encode_tile_parts_impl(P, d_stream, d_offs, d_lens, d_numbps, sop, eph, d_out, cap, d_tile_offs);
}

// j2k_plan_encode_tile_parts with every block cut after its first d_kept[j] bit planes (j2k_plan_rate_allocate): its bytes are the prefix
// d_rate[j * 32 + d_kept[j]] of what the block coder wrote, its passes the 3 p - 2 of those planes (none, and no bytes, for p = 0), ZeroBitPlanes
// as before.  Compaction, bodies, tile-parts, SOP and EPH are unchanged; d_kept[j] = numBPS everywhere gives j2k_plan_encode_tile_parts' bytes.
extern "C" int j2k_plan_encode_tile_parts_kept(j2k_plan *P, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
                                               const uint8_t *d_kept, const uint32_t *d_rate, int sop, int eph, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (!d_stream || !d_offs || !d_lens || !d_numbps || !d_kept || !d_rate || !d_out || !d_tile_offs) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    int r = rate_check(P, "j2k_plan_encode_tile_parts_kept");
    if (r != J2K_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    r = cl_prepare(P);
    if (r != J2K_OK) return r;
    return encode_tile_parts_impl(P, d_stream, d_offs, d_lens, d_numbps, sop, eph, d_out, cap, d_tile_offs, d_kept, d_rate);
}

// the tile-part chains and the packet read (t2dec.hip); d_floors (or null): also every block's floor (the _floors calls)
static int decode_tile_parts_launch(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, uint64_t *d_offs, uint32_t *d_lens,
                                    uint8_t *d_numbps, uint8_t *d_floors, uint8_t *d_pfloors = nullptr) {
    j2k_ctx *ctx = P->ctx;
    HIPCHK(ctx, j2k::launch_t2_tile_chains(ctx->stream, d_cs, (uint64_t)len, d_tile_offs, P->tile_count, P->tile_first, P->d_tile_packet0, P->d_t2_chains));
    // (SOP + EPH streams: a tile's packets side by side, checked against the serial rule and redone by it where a guess was off -- t2dec.hip)
    HIPCHK(ctx, j2k::launch_t2_decode_tiles(ctx->stream, P->d_t2_chains, P->tile_count, P->d_tile_packet0, P->d_t2_packets, P->t2_npackets, P->d_t2_cbs,
                                            (uint64_t)P->blocks.size(), d_cs, (uint64_t)len, sop, eph, P->d_t2_body_base, P->d_frame_status, ctx->t2_parallel ? P->d_t2_par : nullptr,
                                            P->spec.coder == J2K_CODER_HT ? 1 : 0, 31, d_offs, d_lens, d_numbps, d_floors, d_pfloors));
    return J2K_OK;
}
int decode_tile_parts_impl(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                           uint64_t *d_offs, uint32_t *d_lens, uint8_t *d_numbps, uint8_t *d_floors, uint8_t *d_pfloors) {
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (!d_cs || !d_offs || !d_lens || !d_numbps) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int r = cl_prepare(P);
    if (r != J2K_OK) return r;
    return decode_tile_parts_launch(P, d_cs, len, d_tile_offs, sop, eph, d_offs, d_lens, d_numbps, d_floors, d_pfloors);
}
extern "C" int j2k_plan_decode_tile_parts(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                          uint64_t *d_offs, uint32_t *d_lens, uint8_t *d_numbps) {
    graph_note_plan(P);
    return decode_tile_parts_impl(P, d_cs, len, d_tile_offs, sop, eph, d_offs, d_lens, d_numbps, nullptr);
}
// ... for streams whose blocks may be cut at bit planes (j2k_plan_encode_tile_parts_kept): also each block's floor, and numbps counts the planes
// from the block's top down to bit 0 -- d_floors[j] = max(31 - ZeroBitPlanes - (passes + 2) / 3, 0), d_numbps[j] = (passes + 2) / 3 + d_floors[j];
// j2k_plan_decode_blocks_floors decodes them.  An uncut stream gives floors 0 and j2k_plan_decode_tile_parts' tables.  MQ plans only.
extern "C" int j2k_plan_decode_tile_parts_floors(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                                 uint64_t *d_offs, uint32_t *d_lens, uint8_t *d_numbps, uint8_t *d_floors) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!d_floors) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    if (P->spec.coder != J2K_CODER_MQ) return fail(P->ctx, J2K_ERR_UNSUPPORTED, "j2k_plan_decode_tile_parts_floors: per-block floors need the MQ coder");
    { const int rr = raw_magref_refuse(P, "j2k_plan_decode_tile_parts_floors"); if (rr != J2K_OK) return rr; }
    return decode_tile_parts_impl(P, d_cs, len, d_tile_offs, sop, eph, d_offs, d_lens, d_numbps, d_floors);
}

extern "C" int j2k_plan_frame_parallel_tiles(j2k_plan *P, long *tiles) {
    graph_note_plan(P);
    if (!P || !tiles) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "a synchronising call while the context captures a graph");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    *tiles = 0;
    if (!P->d_frame_status) return J2K_OK;
    int n = 0;
    HIPCHK(ctx, hipMemcpyAsync(&n, P->d_frame_status + 1, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(P->d_frame_status + 1, 0, sizeof n, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *tiles = n;
    return J2K_OK;
}

extern "C" int j2k_plan_place_blocks(j2k_plan *P, const int32_t *d_decoded, int32_t *d_coeff) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (!d_decoded || !d_coeff) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    if (!P->spec.closed_loop) return fail(ctx, J2K_ERR_UNSUPPORTED, "the plan was not made with j2k_params.closed_loop: the reference's code-block windows overlap");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, j2k::launch_place_blocks(ctx->stream, P->d_bjobs, P->d_djobs, (int)P->blocks.size(), P->max_block_h, d_decoded, d_coeff));
    return J2K_OK;
}

extern "C" int j2k_plan_frame_status(j2k_plan *P) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "a synchronising call while the context captures a graph");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!P->d_frame_status) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); return J2K_OK; }
    int st = 0;
    HIPCHK(ctx, hipMemcpyAsync(&st, P->d_frame_status, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(P->d_frame_status, 0, sizeof st, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return frame_status_result(ctx, st);
}
int frame_status_result(j2k_ctx *ctx, int st) {
    if (st == J2K_ERR_CAPACITY) return fail(ctx, st, "frame codec: the output buffer is smaller than the tile-parts (the last entry of d_tile_offs says what they take)");
    if (st == J2K_ERR_GO_PANIC) return fail(ctx, st, "frame codec: a palette index >= len(Palette) in the image (Go: index out of range)");
    if (st != J2K_OK) return fail(ctx, st, "frame codec: a malformed tile-part or packet (SOT fields, header bits or body bytes running out)");
    return J2K_OK;
}

int cl_workspaces(j2k_plan *P) {
    j2k_ctx *ctx = P->ctx;
    if (P->d_cl_coeff) return J2K_OK;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: the frame codec's workspaces are made at its first call");
    int r = J2K_OK;
    const size_t n = P->blocks.size();
    auto alloc = [&](void **p, size_t bytes) { first_use_alloc(ctx, r, p, bytes, "hipMalloc (frame codec)"); };
    if (P->spec.coder != J2K_CODER_HT) alloc((void **)&P->d_cl_decoded, (size_t)P->decoded_elems * 4);     // (HT: decoded in place, below)
    alloc((void **)&P->d_cl_offs, (n + 1) * 8);
    alloc((void **)&P->d_cl_lens, n * 4 + 16);
    alloc((void **)&P->d_cl_numbps, n + 16);
    // HT plans: the decoder's coefficient planes, its own (the encoder's forward transform writes d_cl_coeff) and zeroed once --
    // the frame decoder relies on it
    if (P->spec.coder == J2K_CODER_HT) {
        alloc((void **)&P->d_cl_coeff_dec, (size_t)P->coeff_elems * 4);
        if (r == J2K_OK) { hipError_t e = hipMemsetAsync(P->d_cl_coeff_dec, 0, std::max<size_t>((size_t)P->coeff_elems * 4, 64), ctx->stream); if (e != hipSuccess) r = fail_hip(ctx, e, "hipMemsetAsync"); }
    }
    alloc((void **)&P->d_cl_coeff, (size_t)P->coeff_elems * 4);     // (last: its presence says the workspaces are complete)
    return r;
}

// the rate tables, the cuts and the floors of a frame, one allocation made at the first rate-limited call
int cl_rate_workspace(j2k_plan *P, ClRate &W, bool passes) {
    j2k_ctx *ctx = P->ctx;
    const size_t n = P->blocks.size(), nr = (n + 255) & ~size_t(255);
    // (chosen and achieved: [layer][frame] of a batch plan whose frames are allocated alone, 32 x F words each -- sized for the plan's frames whether
    // or not the setting is on, so that j2k_plan_set_rate_per_frame after the first call finds room)
    const size_t F = P->spec.frame_h > 0 && P->spec.frame_h < P->spec.H ? (size_t)(P->spec.H / P->spec.frame_h) : 1, lf = 256 * F;
    const size_t bytes = nr * 32 * 8 + nr * 32 * 4 + 3 * nr + 2 * lf;
    if (!P->d_cl_rate) {
        if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: the frame codec's workspaces are made at its first call");
        HIPCHK(ctx, hipMalloc(&P->d_cl_rate, bytes));
    }
    uint8_t *b = (uint8_t *)P->d_cl_rate;
    W.dist = (uint64_t *)b; b += nr * 32 * 8;
    W.rate = (uint32_t *)b; b += nr * 32 * 4;
    W.chosen = (uint64_t *)b; b += lf;
    W.kept = b; W.floors = b + nr; W.floors_r = b + 2 * nr;
    W.achieved = (double *)(b + 3 * nr);                             // (nr is a multiple of 256: aligned)
    W.spmask = nullptr;
    if (passes) {                                                    // the pass tables: 96 entries per block, and the SigProp masks
        if (!P->d_cl_prate) {
            if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: the frame codec's workspaces are made at its first call");
            HIPCHK(ctx, hipMalloc(&P->d_cl_prate, nr * 96 * 8 + nr * 64 * 8 + nr * 96 * 4 + 256));
        }
        uint8_t *pb = (uint8_t *)P->d_cl_prate;
        W.dist = (uint64_t *)pb; pb += nr * 96 * 8;
        W.spmask = (uint64_t *)pb; pb += nr * 64 * 8;
        W.rate = (uint32_t *)pb;
    }
    return J2K_OK;
}

// ---- the one frame encoder --------------------------------------------------------------------------------------------------------------------
// Block coding into the plan's slots, then every block's bytes ONCE: from its slot to its place in its packet in its tile-part (the stage calls
// j2k_plan_encode_stream + j2k_plan_encode_tile_parts copy them twice: dense stream, tile-parts).  A request that cuts: the block coder also fills
// the rate tables, the distortion launch (with the rectangle, if there is one) the distortion tables, ONE allocation launch chooses every block's
// planes -- the only launch that differs between the forms -- and the packets hold the kept prefixes, or per layer the increments.
int plan_encode_frame_from_coeff(j2k_plan *P, const int32_t *d_coeff, uint32_t *d_lens, uint8_t *d_numbps, const EncodeRequest &q, int sop, int eph, uint8_t *d_out,
                                 size_t cap, uint64_t *d_tile_offs, uint64_t *d_layer_offs) {
    j2k_ctx *ctx = P->ctx;
    int r;
    if (q.kind == EncodeRequest::NONE) {
        r = cl_prepare(P);
        if (r == J2K_OK) r = plan_encode_private_slots(P, d_coeff, d_lens, d_numbps);
        if (r == J2K_OK) r = encode_tile_parts_impl(P, (const uint8_t *)P->d_slots, nullptr, d_lens, d_numbps, sop, eph, d_out, cap, d_tile_offs);
        return r;
    }
    if ((r = rate_check(P, "rate-limited frame encode")) != J2K_OK) return r;     // (j2k_encode_pixels_host_rate has not asked)
    ClRate W{};
    LayerTab *T = nullptr;
    r = cl_prepare(P);
    if (r == J2K_OK) r = cl_rate_workspace(P, W, q.passes);
    if (r == J2K_OK && q.layered) r = layer_tab(P, q.nlayers, &T);
    if (r == J2K_OK && (!P->d_slots || (T && !T->d_kept))) {
        if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: run the same calls once before j2k_ctx_capture_begin");
        if (!P->d_slots) HIPCHK(ctx, hipMalloc(&P->d_slots, (size_t)P->bytes_cap + 64));
        if (T && !T->d_kept) HIPCHK(ctx, hipMalloc((void **)&T->d_kept, std::max<size_t>(P->blocks.size() * (size_t)q.nlayers, 64)));
    }
    if (r == J2K_OK && q.passes) r = plan_encode_blocks_passes(P, d_coeff, (uint8_t *)P->d_slots, d_lens, d_numbps, W.rate, W.dist, W.spmask);
    else if (r == J2K_OK) r = plan_encode_blocks_planes_roi(P, d_coeff, (uint8_t *)P->d_slots, d_lens, d_numbps, W.rate, W.dist, q.roi, q.roi_gain);   // (roi == NULL: j2k_plan_encode_blocks_planes)
    if (r == J2K_OK) r = rate_upload_weights(P);
    if (r != J2K_OK) return r;
    uint8_t *d_kept = T ? T->d_kept : W.kept;
    // the one launch that differs between the forms (rate_allocate_launch, j2k_rate.cpp); W.chosen / W.achieved: [layer][frame of the batch]
    if ((r = rate_allocate_launch(P, q, W.rate, W.dist, d_numbps, d_kept, W.chosen, q.d_achieved ? q.d_achieved : W.achieved)) != J2K_OK) return r;
    if (q.passes)        // the same stage order on the pass tables: one budget or one target, the kept-prefix stream with pass counts
        return encode_tile_parts_impl(P, (const uint8_t *)P->d_slots, nullptr, d_lens, d_numbps, sop, eph, d_out, cap, d_tile_offs, d_kept, W.rate, 1);
    if (T) return encode_tile_parts_layers_launch(P, *T, q.nlayers, (const uint8_t *)P->d_slots, nullptr, d_lens, d_numbps, d_kept, W.rate, sop, eph, d_out, cap, d_tile_offs, d_layer_offs);
    return encode_tile_parts_impl(P, (const uint8_t *)P->d_slots, nullptr, d_lens, d_numbps, sop, eph, d_out, cap, d_tile_offs, d_kept, W.rate);
}

int plan_encode_frame_cl(j2k_plan *P, const EncodeRequest &q, const std::function<int(int32_t *)> &forward, int sop, int eph, uint8_t *d_out, size_t cap,
                         uint64_t *d_tile_offs, uint64_t *d_layer_offs) {
    int r = cl_prepare(P);
    if (r == J2K_OK) r = cl_workspaces(P);
    if (r == J2K_OK && q.roi) r = area_tables(P, false);
    if (r == J2K_OK) r = forward(P->d_cl_coeff);
    if (r == J2K_OK) r = plan_encode_frame_from_coeff(P, P->d_cl_coeff, P->d_cl_lens, P->d_cl_numbps, q, sop, eph, d_out, cap, d_tile_offs, d_layer_offs);
    return r;
}

// the device forms of the pixel encode: their own refusals (before the first launch), their request, the one encoder
static int encode_frame_pixels(j2k_plan *P, int format, const void *d_pix, size_t stride, const EncodeRequest &q, int sop, int eph, uint8_t *d_out, size_t cap,
                               uint64_t *d_tile_offs, uint64_t *d_layer_offs) {
    return plan_encode_frame_cl(P, q, [&](int32_t *d_coeff) { return j2k_plan_forward_pixels(P, format, d_pix, stride, d_coeff); }, sop, eph, d_out, cap, d_tile_offs, d_layer_offs);
}
extern "C" int j2k_plan_encode_frame_pixels(j2k_plan *P, int format, const void *d_pix, size_t stride, int sop, int eph, uint8_t *d_out, size_t cap,
                                            uint64_t *d_tile_offs) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!d_out || !d_tile_offs) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    return encode_frame_pixels(P, format, d_pix, stride, EncodeRequest(), sop, eph, d_out, cap, d_tile_offs, nullptr);
}
// the same chain from an image.YCbCr / CMYK / Paletted (j2k_image.cpp): a palette index >= npal is the frame status's J2K_ERR_GO_PANIC
extern "C" int j2k_plan_encode_frame_image(j2k_plan *P, const j2k_image *d_img, int sop, int eph, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs) {
    graph_note_plan(P);
    if (!P || !d_img) return J2K_ERR_INVALID_ARG;
    if (!d_out || !d_tile_offs) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    return plan_encode_frame_cl(P, EncodeRequest(), [&](int32_t *d_coeff) { return plan_forward_image_impl(P, d_img, d_coeff, P->d_frame_status); }, sop, eph, d_out, cap,
                                d_tile_offs, nullptr);
}
// ... with at most max_body_bytes of code-block bodies (packet and tile-part headers come on top: the last entry of d_tile_offs says what the
// frame took).  A budget that cuts nothing gives j2k_plan_encode_frame_pixels' bytes.
extern "C" int j2k_plan_encode_frame_pixels_rate(j2k_plan *P, int format, const void *d_pix, size_t stride, int sop, int eph, int64_t max_body_bytes,
                                                 uint8_t *d_out, size_t cap, uint64_t *d_tile_offs) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!d_out || !d_tile_offs) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    EncodeRequest q;
    const int r = encode_request(P, "j2k_plan_encode_frame_pixels_rate", &max_body_bytes, nullptr, 1, false, false, nullptr, 1, nullptr, q);
    if (r != J2K_OK) return r;
    return encode_frame_pixels(P, format, d_pix, stride, q, sop, eph, d_out, cap, d_tile_offs, nullptr);
}
extern "C" int j2k_plan_encode_frame_pixels_layers(j2k_plan *P, int format, const void *d_pix, size_t stride, int sop, int eph, const int64_t *layer_bytes, int nlayers,
                                                   uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, uint64_t *d_layer_offs) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!d_out || !d_tile_offs || !d_layer_offs) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    EncodeRequest q;
    const int r = encode_request(P, "j2k_plan_encode_frame_pixels_layers", layer_bytes, nullptr, nlayers, true, false, nullptr, 1, nullptr, q);
    if (r != J2K_OK) return r;
    return encode_frame_pixels(P, format, d_pix, stride, q, sop, eph, d_out, cap, d_tile_offs, d_layer_offs);
}
// Region-of-interest encode, one call for both budget forms: nlayers = 1 with d_layer_offs == NULL is j2k_plan_encode_frame_pixels_rate with
// max_body_bytes = layer_bytes[0], anything else j2k_plan_encode_frame_pixels_layers; the only new step is the distortion launch, which takes the
// rectangle and the gain (rate.hip).
extern "C" int j2k_plan_encode_frame_pixels_roi(j2k_plan *P, int format, const void *d_pix, size_t stride, int sop, int eph, const int64_t *layer_bytes, int nlayers,
                                                const j2k_rect *roi, int roi_gain, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, uint64_t *d_layer_offs) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!d_out || !d_tile_offs) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    EncodeRequest q;
    const int r = encode_request(P, "j2k_plan_encode_frame_pixels_roi", layer_bytes, nullptr, nlayers, d_layer_offs != nullptr, true, roi, roi_gain, nullptr, q);
    if (r != J2K_OK) return r;
    return encode_frame_pixels(P, format, d_pix, stride, q, sop, eph, d_out, cap, d_tile_offs, d_layer_offs);
}
// Quality-targeted encode, one call for both forms as the _roi call: distortion targets in the place of the budgets, roi nullable
extern "C" int j2k_plan_encode_frame_pixels_quality(j2k_plan *P, int format, const void *d_pix, size_t stride, int sop, int eph, const double *targets, int nlayers,
                                                    const j2k_rect *roi, int roi_gain, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, uint64_t *d_layer_offs,
                                                    double *d_achieved) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!d_out || !d_tile_offs) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    EncodeRequest q;
    const int r = encode_request(P, "j2k_plan_encode_frame_pixels_quality", nullptr, targets, nlayers, d_layer_offs != nullptr, roi != nullptr, roi, roi_gain, d_achieved, q);
    if (r != J2K_OK) return r;
    return encode_frame_pixels(P, format, d_pix, stride, q, sop, eph, d_out, cap, d_tile_offs, d_layer_offs);
}
// A budget (frame_bytes) or a target (frame_targets) of its own for every frame of a batch plan with j2k_plan_set_rate_per_frame, exactly one of the
// two; pass_cuts: at coding-pass ends.  One layer, the kept-prefix stream.  The values are read before the call returns and reach the kernel by
// value: a captured call replays them.  d_achieved ([frames], may be null): what every frame's choice reached of its target.
extern "C" int j2k_plan_encode_frame_pixels_rate_frames(j2k_plan *P, int format, const void *d_pix, size_t stride, int sop, int eph, const int64_t *frame_bytes,
                                                        const double *frame_targets, int nframes, int pass_cuts, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs,
                                                        double *d_achieved) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!d_out || !d_tile_offs) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    EncodeRequest q;
    const int r = frame_values_request(P, "j2k_plan_encode_frame_pixels_rate_frames", frame_bytes, frame_targets, nframes, q);
    if (r != J2K_OK) return r;
    q.passes = pass_cuts != 0;
    q.d_achieved = frame_targets ? d_achieved : nullptr;
    return encode_frame_pixels(P, format, d_pix, stride, q, sop, eph, d_out, cap, d_tile_offs, nullptr);
}

// ---- the one frame decoder --------------------------------------------------------------------------------------------------------------------
// (a) the packet parse into the plan's block tables: plain, with every block's floor (a kept-prefix stream), or the LAYERED read, which also
// gathers the blocks' segments into the plan's dense buffer -- the block decoder then reads that in the place of the codestream.  (b) with a
// rectangle: the entries of the blocks it does not need emptied.  (c) block decode and placement: the plan's jobs, or (reduce > 0) the subset of
// the resolutions it keeps -- every packet was parsed, a tile's later ones cannot be found otherwise -- down to max(skip_planes, floor).  (d) the
// inverse transform to pixels, stopped at level `reduce`; with a rectangle into the plan's staging frame, whose window is packed.  The status
// word guards the launches that write d_pix: a stream that was refused leaves the caller's frame alone.
int plan_decode_frame(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, const DecodeRequest &q, const AreaOut *out, void *d_pix,
                      size_t stride) {
    j2k_ctx *ctx = P->ctx;
    const PlanSpec &S = P->spec;
    ReducedTab *R = nullptr;
    int r;
    if (q.reduce != 0 && (r = plan_reduced(P, q.reduce, &R)) != J2K_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LayerTab *T = nullptr;
    r = cl_prepare(P);
    if (r == J2K_OK) r = cl_workspaces(P);
    if (r == J2K_OK && q.area) r = area_tables(P, true);
    if (r == J2K_OK && q.layers > 0) r = layer_tab(P, q.layers, &T);
    if (r != J2K_OK) return r;
    if (!d_cs || !d_pix) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    // (a)
    const size_t n = P->blocks.size(), nr = (n + 255) & ~size_t(255);
    const uint8_t *d_data = d_cs;
    uint8_t *d_floors = nullptr, *d_floors_r = nullptr;
    bool pfl = false;                                    // d_floors holds floors in coding passes (a _passes call)
    if (T) {
        if (!P->d_cl_dense || P->cl_dense_bytes < len + 64 || !P->d_cl_lfloors) {
            if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: the dense buffer grows with the stream -- run the call once on a stream at least as long before j2k_ctx_capture_begin");
            if ((r = ensure_sized(P, &P->d_cl_dense, &P->cl_dense_bytes, len + 64)) != J2K_OK) return r;
            if (!P->d_cl_lfloors) HIPCHK(ctx, hipMalloc((void **)&P->d_cl_lfloors, 2 * nr + 64));
        }
        d_floors = P->d_cl_lfloors; d_floors_r = P->d_cl_lfloors + nr;
        d_data = (const uint8_t *)P->d_cl_dense;
        r = decode_tile_parts_layers_launch(P, *T, q.layers, d_cs, len, d_tile_offs, sop, eph, (uint8_t *)P->d_cl_dense, P->cl_dense_bytes, P->d_cl_offs, P->d_cl_lens,
                                            P->d_cl_numbps, d_floors);
    } else {
        if (q.truncated) {
            ClRate W{};
            if ((r = cl_rate_workspace(P, W)) != J2K_OK) return r;
            d_floors = W.floors; d_floors_r = W.floors_r;
            pfl = q.passes;
        }
        // (the pass floors travel through the area and subset steps as the plane floors do: both only edit one byte per block)
        r = decode_tile_parts_launch(P, d_cs, len, d_tile_offs, sop, eph, P->d_cl_offs, P->d_cl_lens, P->d_cl_numbps, pfl ? nullptr : d_floors, pfl ? d_floors : nullptr);
    }
    if (r != J2K_OK) return r;
    // (b)
    if (q.area && (r = area_launch(P, q.area, q.reduce, nullptr, P->d_cl_lens, P->d_cl_numbps, d_floors)) != J2K_OK) return r;
    // (c)  HT plans: straight into the windows of the decoder's own zeroed planes, coded rows only (the reference's HT decoder writes one row in four,
    // SURVEY fact 3; closed-loop windows partition the plane, and nothing else writes those planes): a quarter of the stores, no placement copy.
    // The windows a reduced decode leaves out keep what an earlier full decode wrote -- no level >= reduce reads them.
    const bool ht = S.coder == J2K_CODER_HT;
    int32_t *coeff = ht ? P->d_cl_coeff_dec : P->d_cl_coeff;
    const BlockJob *bjobs = P->d_bjobs, *djobs = P->d_djobs, *placed = P->d_djobs_placed;
    const uint64_t *offs = P->d_cl_offs;
    const uint32_t *lens = P->d_cl_lens;
    const uint8_t *numbps = P->d_cl_numbps, *floors = d_floors;
    int njobs = (int)n, max_h = P->max_block_h;
    if (R) {
        // the subset's tables, and (the same kernel, the floors in the place of the plane counts) its floors
        if (d_floors) HIPCHK(ctx, launch_select_blocks(ctx->stream, R->d_ids, R->njobs, P->d_cl_offs, P->d_cl_lens, d_floors, R->d_offs, R->d_lens, d_floors_r));
        HIPCHK(ctx, launch_select_blocks(ctx->stream, R->d_ids, R->njobs, P->d_cl_offs, P->d_cl_lens, P->d_cl_numbps, R->d_offs, R->d_lens, R->d_numbps));
        bjobs = R->d_bjobs; djobs = R->d_djobs; placed = R->d_placed; njobs = R->njobs; max_h = R->max_block_h;
        offs = R->d_offs; lens = R->d_lens; numbps = R->d_numbps; floors = d_floors ? d_floors_r : nullptr;
    }
    r = plan_decode_blocks_jobs(P, djobs, njobs, d_data, offs, lens, numbps, ht ? coeff : P->d_cl_decoded, ht ? placed : nullptr, q.skip_planes, pfl ? nullptr : floors,
                                pfl ? floors : nullptr);
    if (r != J2K_OK) return r;
    if (!ht) HIPCHK(ctx, launch_place_blocks(ctx->stream, bjobs, djobs, njobs, max_h, P->d_cl_decoded, coeff));
    // (d)
    if (!q.area) return R ? plan_inverse_pixels_reduced_impl(P, coeff, q.reduce, d_pix, stride, P->d_frame_status) : plan_inverse_pixels_impl(P, coeff, d_pix, stride, P->d_frame_status);
    if ((r = j2k_plan_inverse_reduced(P, coeff, q.reduce, P->d_area_frame)) != J2K_OK) return r;
    const int Wr = (int)reduced_rows(S.W, q.reduce), Hr = (int)reduced_rows(S.H, q.reduce);
    HIPCHK(ctx, launch_pack_pixels_window(ctx->stream, P->d_area_frame, S.C, S.precision, Wr, Hr, out->x0, out->y0, out->w, out->h, (uint8_t *)d_pix, stride, P->d_frame_status));
    return J2K_OK;
}

// the device forms of the decode: their own refusals, in their own order (before the first launch), their request, the one decoder
extern "C" int j2k_plan_decode_frame_pixels(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, void *d_pix,
                                            size_t stride) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    return plan_decode_frame(P, d_cs, len, d_tile_offs, sop, eph, DecodeRequest(), nullptr, d_pix, stride);
}
// Both scalability axes in one call: resolution (`reduce`: Mallat plans; 0 on any closed-loop plan) and quality (`skip_planes`: every MQ block
// decoder stops after that bit plane)
extern "C" int j2k_plan_decode_frame_pixels_coarse(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, int reduce,
                                                   int skip_planes, void *d_pix, size_t stride) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    const int r = check_skip_planes(P->ctx, P->spec.coder, skip_planes, "j2k_plan_decode_frame_pixels_coarse");
    if (r != J2K_OK) return r;
    DecodeRequest q;
    q.reduce = reduce; q.skip_planes = skip_planes;
    return plan_decode_frame(P, d_cs, len, d_tile_offs, sop, eph, q, nullptr, d_pix, stride);
}
// ... to a reduced resolution alone (reduce = 0 too asks for a Mallat plan)
extern "C" int j2k_plan_decode_frame_pixels_reduced(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, int reduce,
                                                    void *d_pix, size_t stride) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    ReducedTab *R = nullptr;
    const int r = plan_reduced(P, reduce, &R);
    if (r != J2K_OK) return r;
    return j2k_plan_decode_frame_pixels_coarse(P, d_cs, len, d_tile_offs, sop, eph, reduce, 0, d_pix, stride);
}
// j2k_plan_decode_frame_pixels_coarse for streams whose blocks may be cut at bit planes: every block runs from its own top plane down to
// max(skip_planes, its floor from the packet header).  An uncut stream decodes as with the _coarse call.
extern "C" int j2k_plan_decode_frame_pixels_rate(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, int reduce,
                                                 int skip_planes, void *d_pix, size_t stride) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    int r = check_skip_planes(ctx, P->spec.coder, skip_planes, "j2k_plan_decode_frame_pixels_rate");
    if (r != J2K_OK) return r;
    if (P->spec.coder != J2K_CODER_MQ) return fail(ctx, J2K_ERR_UNSUPPORTED, "j2k_plan_decode_frame_pixels_rate: per-block floors need the MQ coder");
    if ((r = raw_magref_refuse(P, "j2k_plan_decode_frame_pixels_rate")) != J2K_OK) return r;
    if (!d_pix) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    DecodeRequest q;
    q.truncated = true; q.reduce = reduce; q.skip_planes = skip_planes;
    return plan_decode_frame(P, d_cs, len, d_tile_offs, sop, eph, q, nullptr, d_pix, stride);
}
// the first `layers` layers of every tile-part of a layered stream
extern "C" int j2k_plan_decode_frame_pixels_layers(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, int layers, int reduce,
                                                   int skip_planes, void *d_pix, size_t stride) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    int r = check_skip_planes(ctx, P->spec.coder, skip_planes, "j2k_plan_decode_frame_pixels_layers");
    if (r == J2K_OK) r = layers_check(P, layers, "j2k_plan_decode_frame_pixels_layers");
    if (r != J2K_OK) return r;
    if (!d_cs || !d_pix) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    DecodeRequest q;
    q.layers = layers; q.reduce = reduce; q.skip_planes = skip_planes;
    return plan_decode_frame(P, d_cs, len, d_tile_offs, sop, eph, q, nullptr, d_pix, stride);
}

extern "C" int j2k_plan_get_decoded_offsets(const j2k_plan *P, uint64_t *offs, size_t cap) {
    if (!P || !offs) return J2K_ERR_INVALID_ARG;
    if (cap < P->dec_off.size()) return J2K_ERR_CAPACITY;
    if (!P->dec_off.empty()) memcpy(offs, P->dec_off.data(), P->dec_off.size() * sizeof(uint64_t));
    return J2K_OK;
}

extern "C" int j2k_plan_get_ht_decode_leaders(const j2k_plan *P, int32_t *leaders, size_t cap) {
    if (!P || !leaders) return J2K_ERR_INVALID_ARG;
    if (P->spec.coder != J2K_CODER_HT) return J2K_ERR_UNSUPPORTED;
    if (cap < P->ht_dec_rep.size()) return J2K_ERR_CAPACITY;
    if (!P->ht_dec_rep.empty()) memcpy(leaders, P->ht_dec_rep.data(), P->ht_dec_rep.size() * sizeof(int32_t));
    return J2K_OK;
}

extern "C" int j2k_plan_get_ht_decode_walk_order(const j2k_plan *P, int32_t *order, size_t cap, int32_t *n_leaders) {
    if (!P || !order) return J2K_ERR_INVALID_ARG;
    if (P->spec.coder != J2K_CODER_HT) return J2K_ERR_UNSUPPORTED;
    if (cap < P->ht_walk_order.size()) return J2K_ERR_CAPACITY;
    if (!P->ht_walk_order.empty()) memcpy(order, P->ht_walk_order.data(), P->ht_walk_order.size() * sizeof(int32_t));
    if (n_leaders) *n_leaders = (int32_t)P->ht_walk_nlead;
    return J2K_OK;
}

