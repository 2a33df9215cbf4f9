// j2k_layers.cpp -- quality layers of the closed-loop MQ codec behind the C ABI: one encode yields one stream whose tile-parts are layer-major,
// so a byte prefix of every tile-part is a lower-quality version of the frame.  include/j2kgfx.h has the contract, DESIGN.md 7 the format,
// tests/layer_cases.py the definition.  Kernels: rate.hip (the allocation of L budgets), t2dev.hip (the layer table, the layer ends), t2dec.hip
// (the LAYERED packet read, the segment gather).  Here: the tables of a layer count, the refusals of every encode request (encode_request), the
// layered stage calls and the host forms of the layered, roi and quality encodes; the frame encoder and decoder that run them are in j2k_frame.cpp,
// the host drivers in j2k_hostcalls.cpp.  The host-only j2k_tile_parts_keep_layers is in assemble.cpp.
#include "j2k_host.h"

using namespace j2k;

static void free_layer_tab(LayerTab &T) {
    void *ptrs[] = {T.d_packets, T.d_tile_packet0, T.d_ptile, T.d_end_packet, T.d_cbs, T.d_poffs, T.d_ws, T.d_body_base, T.d_kept};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    T = LayerTab();
}
void free_layer_tabs(j2k_plan *P) {
    for (LayerTab &T : P->layer_tabs) free_layer_tab(T);
    P->layer_tabs.clear();
}

// what every layer call needs: the plan rate_check accepts, a layer count in range
int layers_check(j2k_plan *P, int nlayers, const char *who) {
    const int r = rate_check(P, who);
    if (r != J2K_OK) return r;
    if (nlayers < 1 || nlayers > J2K_MAX_LAYERS) return fail(P->ctx, J2K_ERR_INVALID_ARG, (std::string(who) + ": the layer count is 1 ... 32").c_str());
    return J2K_OK;
}
// every refusal of an encode request, in the order the entry points have always made them (j2k_host.h), and the request
int encode_request(j2k_plan *P, const char *who, const int64_t *layer_bytes, const double *targets, int nlayers, bool layered, bool check_roi, const j2k_rect *roi,
                   int roi_gain, double *d_achieved, EncodeRequest &q) {
    j2k_ctx *ctx = P->ctx;
    const std::string w(who);
    int r = layers_check(P, nlayers, who);
    if (r == J2K_OK && check_roi) r = roi_check(P, roi, roi_gain, who);
    if (r != J2K_OK) return r;
    if (targets) {
        if ((r = targets_check(ctx, targets, nlayers, who)) != J2K_OK) return r;
        std::copy(targets, targets + nlayers, q.targets);
    } else {
        // cumulative budgets: none negative, none below the one before
        if (!layer_bytes) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": no budgets").c_str());
        for (int l = 0; l < nlayers; l++) {
            if (layer_bytes[l] < 0) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": a negative budget").c_str());
            if (l && layer_bytes[l] < layer_bytes[l - 1]) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": the budgets are cumulative -- none may be below the one before").c_str());
            q.budgets[l] = (uint64_t)layer_bytes[l];
        }
    }
    if (!layered && nlayers != 1) return fail(ctx, J2K_ERR_INVALID_ARG, (w + (targets ? ": more than one target" : ": more than one budget") + " needs the layer ends (layer_offs)").c_str());
    q.kind = targets ? EncodeRequest::DISTORTION : EncodeRequest::BYTES;
    q.nlayers = nlayers; q.layered = layered; q.roi = roi; q.roi_gain = roi_gain; q.d_achieved = d_achieved;
    return J2K_OK;
}

// the tables of layer count L, made at its first use
int layer_tab(j2k_plan *P, int L, LayerTab **out) {
    j2k_ctx *ctx = P->ctx;
    if (P->layer_tabs.empty()) P->layer_tabs.resize(J2K_MAX_LAYERS + 1);
    LayerTab &T = P->layer_tabs[(size_t)L];
    *out = &T;
    if (T.built) return J2K_OK;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: the tables of a layer count are made at its first use -- run the call once before j2k_ctx_capture_begin");
    std::vector<j2k_t2_dev_packet> base, pk;
    std::vector<int> tp0;
    plan_t2_packets(P, 0, base, &tp0);
    const size_t n = P->blocks.size(), nt = (size_t)P->tile_count;
    std::vector<int> tpl(nt + 1, 0), endp(nt * (size_t)L + 1, 0);
    std::vector<int32_t> ptile;
    for (size_t t = 0; t < nt; t++) {
        tpl[t] = (int)pk.size();
        for (int l = 0; l < L; l++) {
            for (int q = tp0[t]; q < tp0[t + 1]; q++) {
                j2k_t2_dev_packet p = base[(size_t)q];
                p.layer = l;
                p.cb0 += (int64_t)l * (int64_t)n;
                p.flags = (p.flags & ~J2K_T2_FRESH) | J2K_T2_LAYERED | (l == 0 ? (base[(size_t)q].flags & J2K_T2_FRESH) : 0);   // one coder object per tile, over all its layers
                pk.push_back(p);
                ptile.push_back((int32_t)t);
            }
            endp[t * (size_t)L + (size_t)l] = (int)pk.size();
        }
    }
    tpl[nt] = (int)pk.size();
    if (ptile.empty()) ptile.push_back(0);
    const size_t np = pk.size();
    int r = upload(ctx, &T.d_tile_packet0, tpl);
    if (r == J2K_OK) r = upload(ctx, &T.d_ptile, ptile);
    if (r == J2K_OK) r = upload(ctx, &T.d_end_packet, endp);
    auto alloc = [&](void **p, size_t bytes) { first_use_alloc(ctx, r, p, bytes, "hipMalloc (quality layers)"); };
    alloc((void **)&T.d_cbs, n * (size_t)L * sizeof(j2k_t2_dev_cb));
    alloc((void **)&T.d_poffs, (np + 1) * 8);
    alloc(&T.d_ws, ((j2k::t2_dev_workspace((long)np) + 15) & ~size_t(15)) + 64);
    alloc((void **)&T.d_body_base, np * 8);
    if (r == J2K_OK) r = upload(ctx, &T.d_packets, pk);
    if (r != J2K_OK) { free_layer_tab(T); return r; }
    T.npackets = (int)np;
    T.built = true;
    return J2K_OK;
}

extern "C" size_t j2k_plan_frame_bound_layers(const j2k_plan *P, int nlayers) {
    if (!P || !P->spec.closed_loop || nlayers < 1 || nlayers > J2K_MAX_LAYERS) return 0;
    std::vector<j2k_t2_dev_packet> pk;
    plan_t2_packets(P, 0, pk, nullptr);
    // (a block's share of a layer's header: at most 32 + 1 + 32 + 16 + 5 + 31 = 117 bits against the 128 counted.  Stuffing -- a byte behind 0xFF
    // holds seven bits -- cannot use up the rest: the two long runs are zeros, only the pass code and the length fields, 52 bits, can form 0xFF
    // bytes: at most 6 of them, 6 bits more.  A packet's markers and padding: 9 bytes.)
    return (size_t)P->bytes_cap + (size_t)nlayers * (16 * P->blocks.size() + 16 * pk.size()) + 14 * (size_t)P->tile_count + 64;
}

extern "C" int j2k_plan_rate_allocate_layers(j2k_plan *P, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps, const int64_t *layer_bytes,
                                             int nlayers, uint8_t *d_kept, uint64_t *d_chosen) {
    graph_note_plan(P);
    if (!P || !d_rate || !d_dist || !d_numbps || !d_kept || !d_chosen) return J2K_ERR_INVALID_ARG;
    EncodeRequest q;
    int r = encode_request(P, "j2k_plan_rate_allocate_layers", layer_bytes, nullptr, nlayers, true, false, nullptr, 1, nullptr, q);
    if (r != J2K_OK) return r;
    return rate_allocate_launch(P, q, d_rate, d_dist, d_numbps, d_kept, d_chosen, nullptr);
}

// the layer table from the cuts, then the packet coder as it is (its kernels write exactly the layered header from these entries: t2_fields,
// t2_contributes), then the layer ends.  d_offs == NULL: d_data is the plan's slot buffer and block j's codeword starts at its slot.
int encode_tile_parts_layers_launch(j2k_plan *P, LayerTab &T, int L, const uint8_t *d_data, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
                                         const uint8_t *d_kept, const uint32_t *d_rate, int sop, int eph, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs,
                                         uint64_t *d_layer_offs) {
    j2k_ctx *ctx = P->ctx;
    const long n = (long)P->blocks.size(), np = T.npackets;
    uint64_t *d_res = reinterpret_cast<uint64_t *>((uint8_t *)T.d_ws + ((j2k::t2_dev_workspace(np) + 15) & ~size_t(15)));
    HIPCHK(ctx, launch_t2_fill_layer_cbs(ctx->stream, n, L, d_offs, d_offs ? nullptr : P->d_bjobs, d_lens, d_numbps, 31, d_kept, d_rate, T.d_cbs, d_res));
    HIPCHK(ctx, launch_t2_encode_tile_parts(ctx->stream, T.d_packets, np, T.d_cbs, (uint64_t)n * (uint64_t)L, d_data, sop, eph, d_out, (uint64_t)cap, T.d_poffs, T.d_ws, d_res,
                                            T.d_ptile, T.d_tile_packet0, P->tile_count, P->tile_first, d_tile_offs, P->d_frame_status, nullptr, nullptr, 0, P->t2_body_slices));
    HIPCHK(ctx, launch_t2_layer_ends(ctx->stream, P->tile_count * L, L, T.d_end_packet, T.d_poffs, d_layer_offs));
    return J2K_OK;
}

extern "C" int j2k_plan_encode_tile_parts_layers(j2k_plan *P, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
                                                 const uint8_t *d_kept, const uint32_t *d_rate, int nlayers, int sop, int eph, uint8_t *d_out, size_t cap,
                                                 uint64_t *d_tile_offs, uint64_t *d_layer_offs) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (!d_stream || !d_offs || !d_lens || !d_numbps || !d_kept || !d_rate || !d_out || !d_tile_offs || !d_layer_offs) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    int r = layers_check(P, nlayers, "j2k_plan_encode_tile_parts_layers");
    if (r != J2K_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LayerTab *T = nullptr;
    r = cl_prepare(P);
    if (r == J2K_OK) r = layer_tab(P, nlayers, &T);
    if (r != J2K_OK) return r;
    return encode_tile_parts_layers_launch(P, *T, nlayers, d_stream, d_offs, d_lens, d_numbps, d_kept, d_rate, sop, eph, d_out, cap, d_tile_offs, d_layer_offs);
}

int decode_tile_parts_layers_launch(j2k_plan *P, LayerTab &T, int layers, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
                                         uint8_t *d_dense, size_t dense_cap, uint64_t *d_offs, uint32_t *d_lens, uint8_t *d_numbps, uint8_t *d_floors) {
    j2k_ctx *ctx = P->ctx;
    HIPCHK(ctx, j2k::launch_t2_tile_chains(ctx->stream, d_cs, (uint64_t)len, d_tile_offs, P->tile_count, P->tile_first, T.d_tile_packet0, P->d_t2_chains));
    HIPCHK(ctx, j2k::launch_t2_decode_tiles_layers(ctx->stream, P->d_t2_chains, P->tile_count, T.d_packets, T.npackets, T.d_cbs, (long)P->blocks.size(), layers, d_cs,
                                                   (uint64_t)len, sop, eph, T.d_body_base, P->d_frame_status, 31, d_dense, (uint64_t)dense_cap, d_offs, d_lens, d_numbps,
                                                   d_floors));
    return J2K_OK;
}

extern "C" int j2k_plan_decode_tile_parts_layers(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, int layers,
                                                 uint8_t *d_dense, size_t dense_cap, uint64_t *d_offs, uint32_t *d_lens, uint8_t *d_numbps, uint8_t *d_floors) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (!d_cs || !d_dense || !d_offs || !d_lens || !d_numbps || !d_floors) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    int r = layers_check(P, layers, "j2k_plan_decode_tile_parts_layers");
    if (r != J2K_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LayerTab *T = nullptr;
    r = cl_prepare(P);
    if (r == J2K_OK) r = layer_tab(P, layers, &T);
    if (r != J2K_OK) return r;
    return decode_tile_parts_layers_launch(P, *T, layers, d_cs, len, d_tile_offs, sop, eph, d_dense, dense_cap, d_offs, d_lens, d_numbps, d_floors);
}

// ---- host memory in, host memory out: the layered, roi and quality forms (the driver: j2k_hostcalls.cpp) ------------------------------------------
// d_host_io holds the larger of the two streams for the forms that can write either (roi, quality: layer_offs == NULL asks for the kept-prefix one)
extern "C" int j2k_encode_pixels_host_layers(j2k_plan *P, int format, const void *pix, size_t stride, int sop, int eph, const int64_t *layer_bytes, int nlayers,
                                             uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs, uint64_t *layer_offs, uint32_t *lens, uint8_t *numbps) {
    graph_note_plan(P);
    EncodeRequest q;
    int r = host_call_check(P, pix, out_len);
    if (r == J2K_OK) r = encode_request(P, "j2k_encode_pixels_host_layers", layer_bytes, nullptr, nlayers, true, false, nullptr, 1, nullptr, q);
    if (r != J2K_OK) return r;
    return encode_pixels_host(P, format, pix, stride, q, true, j2k_plan_frame_bound_layers(P, nlayers), sop, eph, out, cap, out_len, tile_offs, layer_offs, lens, numbps, nullptr);
}
// the synchronous host-memory form of j2k_plan_encode_frame_pixels_roi (layer_offs == NULL with nlayers = 1: the single-budget stream)
extern "C" int j2k_encode_pixels_host_roi(j2k_plan *P, int format, const void *pix, size_t stride, int sop, int eph, const int64_t *layer_bytes, int nlayers,
                                          const j2k_rect *roi, int roi_gain, uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs, uint64_t *layer_offs,
                                          uint32_t *lens, uint8_t *numbps) {
    graph_note_plan(P);
    EncodeRequest q;
    int r = host_call_check(P, pix, out_len);
    if (r == J2K_OK) r = encode_request(P, "j2k_encode_pixels_host_roi", layer_bytes, nullptr, nlayers, layer_offs != nullptr, true, roi, roi_gain, nullptr, q);
    if (r != J2K_OK) return r;
    return encode_pixels_host(P, format, pix, stride, q, true, std::max(j2k_plan_frame_bound_layers(P, nlayers), j2k_plan_frame_bound(P)), sop, eph, out, cap, out_len, tile_offs,
                              layer_offs, lens, numbps, nullptr);
}
// the synchronous host-memory form of j2k_plan_encode_frame_pixels_quality (layer_offs == NULL with nlayers = 1: the kept-stream format; roi nullable)
extern "C" int j2k_encode_pixels_host_quality(j2k_plan *P, int format, const void *pix, size_t stride, int sop, int eph, const double *targets, int nlayers,
                                              const j2k_rect *roi, int roi_gain, uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs, uint64_t *layer_offs,
                                              uint32_t *lens, uint8_t *numbps, double *achieved) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!targets) return fail(P->ctx, J2K_ERR_INVALID_ARG, "j2k_encode_pixels_host_quality: no targets");
    EncodeRequest q;
    int r = host_call_check(P, pix, out_len);
    if (r == J2K_OK) r = encode_request(P, "j2k_encode_pixels_host_quality", nullptr, targets, nlayers, layer_offs != nullptr, roi != nullptr, roi, roi_gain, nullptr, q);
    if (r != J2K_OK) return r;
    return encode_pixels_host(P, format, pix, stride, q, true, std::max(j2k_plan_frame_bound_layers(P, nlayers), j2k_plan_frame_bound(P)), sop, eph, out, cap, out_len, tile_offs,
                              layer_offs, lens, numbps, achieved);
}

extern "C" int j2k_decode_pixels_host_layers(j2k_plan *P, const uint8_t *cs, size_t len, int sop, int eph, int layers, int reduce, int skip_planes, void *pix,
                                             size_t stride) {
    graph_note_plan(P);
    int r = host_call_check(P, cs, pix);
    if (r != J2K_OK) return r;
    r = check_skip_planes(P->ctx, P->spec.coder, skip_planes, "j2k_decode_pixels_host_layers");
    if (r == J2K_OK) r = layers_check(P, layers, "j2k_decode_pixels_host_layers");
    int32_t wr = 0, hr = 0;
    if (r == J2K_OK && reduce != 0) r = j2k_plan_reduced_size(P, reduce, &wr, &hr);
    if (r != J2K_OK) return r;
    return decode_host(P, cs, len, reduced_rows(P->spec.H, reduce) * stride, pix, false, [&](const uint8_t *d_cs, void *d_pix) {
        return j2k_plan_decode_frame_pixels_layers(P, d_cs, len, nullptr, sop, eph, layers, reduce, skip_planes, d_pix, stride);
    });
}
