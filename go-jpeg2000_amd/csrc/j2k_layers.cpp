// j2k_layers.cpp -- quality layers of the closed-loop MQ codec behind the C ABI: one encode yields one stream whose tile-parts are layer-major,
// so a byte prefix of every tile-part is a lower-quality version of the frame.  include/j2kgfx.h has the contract, DESIGN.md 7 the format,
// tests/layer_cases.py the definition.  Kernels: rate.hip (the allocation of L budgets), t2dev.hip (the layer table, the layer ends), t2dec.hip
// (the LAYERED packet read, the segment gather).  The host-only j2k_tile_parts_keep_layers is in assemble.cpp.
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
static int layers_check(j2k_plan *P, int nlayers, const char *who) {
    const int r = rate_check(P, who);
    if (r != J2K_OK) return r;
    if (nlayers < 1 || nlayers > J2K_MAX_LAYERS) return fail(P->ctx, J2K_ERR_INVALID_ARG, (std::string(who) + ": the layer count is 1 ... 32").c_str());
    return J2K_OK;
}
// cumulative budgets: none negative, none below the one before
static int budgets_check(j2k_ctx *ctx, const int64_t *layer_bytes, int nlayers, uint64_t *out, const char *who) {
    if (!layer_bytes) return fail(ctx, J2K_ERR_INVALID_ARG, (std::string(who) + ": no budgets").c_str());
    for (int l = 0; l < nlayers; l++) {
        if (layer_bytes[l] < 0) return fail(ctx, J2K_ERR_INVALID_ARG, (std::string(who) + ": a negative budget").c_str());
        if (l && layer_bytes[l] < layer_bytes[l - 1]) return fail(ctx, J2K_ERR_INVALID_ARG, (std::string(who) + ": the budgets are cumulative -- none may be below the one before").c_str());
        out[l] = (uint64_t)layer_bytes[l];
    }
    return J2K_OK;
}

// the tables of layer count L, made at its first use
static int layer_tab(j2k_plan *P, int L, LayerTab **out) {
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
    auto alloc = [&](void **p, size_t bytes) { if (r == J2K_OK) { hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 64)); if (e != hipSuccess) r = fail_hip(ctx, e, "hipMalloc (quality layers)"); } };
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
    if (!P || !d_rate || !d_dist || !d_numbps || !d_kept || !d_chosen) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    int r = layers_check(P, nlayers, "j2k_plan_rate_allocate_layers");
    if (r != J2K_OK) return r;
    uint64_t budgets[J2K_MAX_LAYERS];
    r = budgets_check(ctx, layer_bytes, nlayers, budgets, "j2k_plan_rate_allocate_layers");
    if (r != J2K_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    r = rate_upload_weights(P);
    if (r != J2K_OK) return r;
    HIPCHK(ctx, launch_rate_allocate_layers(ctx->stream, (int)P->blocks.size(), d_rate, d_dist, d_numbps, P->d_rate_wj, budgets, nlayers, P->d_rate_ws, d_kept, d_chosen));
    return J2K_OK;
}

// the layer table from the cuts, then the packet coder as it is (its kernels write exactly the layered header from these entries: t2_fields,
// t2_contributes), then the layer ends.  d_offs == NULL: d_data is the plan's slot buffer and block j's codeword starts at its slot.
static int encode_tile_parts_layers_impl(j2k_plan *P, LayerTab &T, int L, const uint8_t *d_data, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
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
    return encode_tile_parts_layers_impl(P, *T, nlayers, d_stream, d_offs, d_lens, d_numbps, d_kept, d_rate, sop, eph, d_out, cap, d_tile_offs, d_layer_offs);
}

static int decode_tile_parts_layers_impl(j2k_plan *P, LayerTab &T, int layers, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph,
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
    return decode_tile_parts_layers_impl(P, *T, layers, d_cs, len, d_tile_offs, sop, eph, d_dense, dense_cap, d_offs, d_lens, d_numbps, d_floors);
}

// coefficients -> layered tile-parts: block coding into the plan's slots with the tables, the allocation of the L budgets in one launch, then every
// block's increments from its slot into its L packets (d_lens / d_numbps: the caller's tables, filled with the UNCUT lengths and plane counts).
// targets != NULL (the _quality calls): the L distortion targets in the place of the budgets -- the allocation launch is the only one that differs;
// d_achieved (device, or null): the weighted distortion of every layer's choice
static int encode_frame_from_coeff_layers(j2k_plan *P, const int32_t *d_coeff, uint32_t *d_lens, uint8_t *d_numbps, const uint64_t *budgets, int L, int sop, int eph,
                                          uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, uint64_t *d_layer_offs, const j2k_rect *roi = nullptr, int roi_gain = 1,
                                          const double *targets = nullptr, double *d_achieved = nullptr) {
    j2k_ctx *ctx = P->ctx;
    ClRate W{};
    LayerTab *T = nullptr;
    int r = cl_prepare(P);
    if (r == J2K_OK) r = cl_rate_workspace(P, W);
    if (r == J2K_OK) r = layer_tab(P, L, &T);
    if (r == J2K_OK && (!P->d_slots || !T->d_kept)) {
        if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: run the same calls once before j2k_ctx_capture_begin");
        if (!P->d_slots) HIPCHK(ctx, hipMalloc(&P->d_slots, (size_t)P->bytes_cap + 64));
        if (!T->d_kept) HIPCHK(ctx, hipMalloc((void **)&T->d_kept, std::max<size_t>(P->blocks.size() * (size_t)L, 64)));
    }
    if (r == J2K_OK) r = plan_encode_blocks_planes_roi(P, d_coeff, (uint8_t *)P->d_slots, d_lens, d_numbps, W.rate, W.dist, roi, roi_gain);   // (roi == NULL: j2k_plan_encode_blocks_planes)
    if (r == J2K_OK) r = rate_upload_weights(P);
    if (r != J2K_OK) return r;
    if (targets)
        HIPCHK(ctx, launch_rate_allocate_quality(ctx->stream, (int)P->blocks.size(), W.rate, W.dist, d_numbps, P->d_rate_wj, targets, L, P->d_rate_ws, T->d_kept, W.chosen,
                                                 d_achieved ? d_achieved : W.achieved));
    else
        HIPCHK(ctx, launch_rate_allocate_layers(ctx->stream, (int)P->blocks.size(), W.rate, W.dist, d_numbps, P->d_rate_wj, budgets, L, P->d_rate_ws, T->d_kept, W.chosen));      // (W.chosen: 32 words, one per layer)
    return encode_tile_parts_layers_impl(P, *T, L, (const uint8_t *)P->d_slots, nullptr, d_lens, d_numbps, T->d_kept, W.rate, sop, eph, d_out, cap, d_tile_offs, d_layer_offs);
}

extern "C" int j2k_plan_encode_frame_pixels_layers(j2k_plan *P, int format, const void *d_pix, size_t stride, int sop, int eph, const int64_t *layer_bytes, int nlayers,
                                                   uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, uint64_t *d_layer_offs) {
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (!d_out || !d_tile_offs || !d_layer_offs) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    int r = layers_check(P, nlayers, "j2k_plan_encode_frame_pixels_layers");
    if (r != J2K_OK) return r;
    uint64_t budgets[J2K_MAX_LAYERS];
    r = budgets_check(ctx, layer_bytes, nlayers, budgets, "j2k_plan_encode_frame_pixels_layers");
    if (r != J2K_OK) return r;
    r = cl_prepare(P);
    if (r == J2K_OK) r = cl_workspaces(P);
    if (r == J2K_OK) r = j2k_plan_forward_pixels(P, format, d_pix, stride, P->d_cl_coeff);
    if (r == J2K_OK) r = encode_frame_from_coeff_layers(P, P->d_cl_coeff, P->d_cl_lens, P->d_cl_numbps, budgets, nlayers, sop, eph, d_out, cap, d_tile_offs, d_layer_offs);
    return r;
}

// Region-of-interest encode, one call for both budget forms: nlayers = 1 with d_layer_offs == NULL is j2k_plan_encode_frame_pixels_rate with
// max_body_bytes = layer_bytes[0], anything else j2k_plan_encode_frame_pixels_layers; the only new step is the distortion launch, which takes the
// rectangle and the gain (rate.hip).  Every refusal comes before the first launch.
static int roi_frame_check(j2k_plan *P, const int64_t *layer_bytes, int nlayers, bool layered, const j2k_rect *roi, int roi_gain, uint64_t *budgets, const char *who) {
    int r = layers_check(P, nlayers, who);
    if (r == J2K_OK) r = roi_check(P, roi, roi_gain, who);
    if (r == J2K_OK) r = budgets_check(P->ctx, layer_bytes, nlayers, budgets, who);
    if (r == J2K_OK && !layered && nlayers != 1) r = fail(P->ctx, J2K_ERR_INVALID_ARG, (std::string(who) + ": more than one budget needs the layer ends (layer_offs)").c_str());
    return r;
}
extern "C" int j2k_plan_encode_frame_pixels_roi(j2k_plan *P, int format, const void *d_pix, size_t stride, int sop, int eph, const int64_t *layer_bytes, int nlayers,
                                                const j2k_rect *roi, int roi_gain, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, uint64_t *d_layer_offs) {
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (!d_out || !d_tile_offs) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    uint64_t budgets[J2K_MAX_LAYERS];
    int r = roi_frame_check(P, layer_bytes, nlayers, d_layer_offs != nullptr, roi, roi_gain, budgets, "j2k_plan_encode_frame_pixels_roi");
    if (r != J2K_OK) return r;
    r = cl_prepare(P);
    if (r == J2K_OK) r = cl_workspaces(P);
    if (r == J2K_OK) r = area_tables(P, false);
    if (r == J2K_OK) r = j2k_plan_forward_pixels(P, format, d_pix, stride, P->d_cl_coeff);
    if (r != J2K_OK) return r;
    if (!d_layer_offs) return plan_encode_frame_from_coeff_rate(P, P->d_cl_coeff, P->d_cl_lens, P->d_cl_numbps, layer_bytes[0], sop, eph, d_out, cap, d_tile_offs, roi, roi_gain);
    return encode_frame_from_coeff_layers(P, P->d_cl_coeff, P->d_cl_lens, P->d_cl_numbps, budgets, nlayers, sop, eph, d_out, cap, d_tile_offs, d_layer_offs, roi, roi_gain);
}

// Quality-targeted encode, one call for both forms as the _roi call: nlayers = 1 with d_layer_offs == NULL writes the kept-stream format of
// j2k_plan_encode_frame_pixels_rate, anything else the layered stream; the distortion launch (roi or not), the packets and the tile-parts are
// theirs.  Every refusal comes before the first launch.
static int quality_frame_check(j2k_plan *P, const double *targets, int nlayers, bool layered, const j2k_rect *roi, int roi_gain, const char *who) {
    int r = layers_check(P, nlayers, who);
    if (r == J2K_OK && roi) r = roi_check(P, roi, roi_gain, who);
    if (r == J2K_OK) r = targets_check(P->ctx, targets, nlayers, who);
    if (r == J2K_OK && !layered && nlayers != 1) r = fail(P->ctx, J2K_ERR_INVALID_ARG, (std::string(who) + ": more than one target needs the layer ends (layer_offs)").c_str());
    return r;
}
extern "C" int j2k_plan_encode_frame_pixels_quality(j2k_plan *P, int format, const void *d_pix, size_t stride, int sop, int eph, const double *targets, int nlayers,
                                                    const j2k_rect *roi, int roi_gain, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, uint64_t *d_layer_offs,
                                                    double *d_achieved) {
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (!d_out || !d_tile_offs) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    int r = quality_frame_check(P, targets, nlayers, d_layer_offs != nullptr, roi, roi_gain, "j2k_plan_encode_frame_pixels_quality");
    if (r != J2K_OK) return r;
    r = cl_prepare(P);
    if (r == J2K_OK) r = cl_workspaces(P);
    if (r == J2K_OK && roi) r = area_tables(P, false);
    if (r == J2K_OK) r = j2k_plan_forward_pixels(P, format, d_pix, stride, P->d_cl_coeff);
    if (r != J2K_OK) return r;
    if (!d_layer_offs)
        return plan_encode_frame_from_coeff_quality(P, P->d_cl_coeff, P->d_cl_lens, P->d_cl_numbps, targets[0], sop, eph, d_out, cap, d_tile_offs, roi, roi_gain, d_achieved);
    return encode_frame_from_coeff_layers(P, P->d_cl_coeff, P->d_cl_lens, P->d_cl_numbps, nullptr, nlayers, sop, eph, d_out, cap, d_tile_offs, d_layer_offs, roi, roi_gain, targets,
                                          d_achieved);
}

// the first `layers` layers of every tile-part -> pixels: the LAYERED packet read, the blocks' segments gathered into the plan's dense buffer, then
// the decode of j2k_plan_decode_frame_pixels_rate on that buffer in the place of the codestream
extern "C" int j2k_plan_decode_frame_pixels_layers(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, int layers, int reduce,
                                                   int skip_planes, void *d_pix, size_t stride) {
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    int r = check_skip_planes(ctx, P->spec.coder, skip_planes, "j2k_plan_decode_frame_pixels_layers");
    if (r == J2K_OK) r = layers_check(P, layers, "j2k_plan_decode_frame_pixels_layers");
    if (r != J2K_OK) return r;
    if (!d_cs || !d_pix) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    ReducedTab *R = nullptr;
    if (reduce != 0) { r = plan_reduced(P, reduce, &R); if (r != J2K_OK) return r; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LayerTab *T = nullptr;
    r = cl_prepare(P);
    if (r == J2K_OK) r = cl_workspaces(P);
    if (r == J2K_OK) r = layer_tab(P, layers, &T);
    if (r != J2K_OK) return r;
    const size_t n = P->blocks.size(), nr = (n + 255) & ~size_t(255);
    if (!P->d_cl_dense || P->cl_dense_bytes < len + 64 || !P->d_cl_lfloors) {
        if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: the dense buffer grows with the stream -- run the call once on a stream at least as long before j2k_ctx_capture_begin");
        if ((r = ensure_sized(ctx, &P->d_cl_dense, &P->cl_dense_bytes, len + 64)) != J2K_OK) return r;
        if (!P->d_cl_lfloors) HIPCHK(ctx, hipMalloc((void **)&P->d_cl_lfloors, 2 * nr + 64));
    }
    r = decode_tile_parts_layers_impl(P, *T, layers, d_cs, len, d_tile_offs, sop, eph, (uint8_t *)P->d_cl_dense, P->cl_dense_bytes, P->d_cl_offs, P->d_cl_lens, P->d_cl_numbps,
                                      P->d_cl_lfloors);
    if (r != J2K_OK) return r;
    return plan_decode_frame_tables(P, (const uint8_t *)P->d_cl_dense, R, reduce, skip_planes, P->d_cl_lfloors, P->d_cl_lfloors + nr, d_pix, stride);
}

// ---- host memory in, host memory out ---------------------------------------------------------------------------------------------------------
// with_roi: j2k_encode_pixels_host_roi, whose layer_offs == NULL asks for the single-budget (_rate) stream
static int encode_pixels_host_layers_impl(j2k_plan *P, int format, const void *pix, size_t stride, int sop, int eph, const int64_t *layer_bytes, int nlayers,
                                          bool with_roi, const j2k_rect *roi, int roi_gain, uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs,
                                          uint64_t *layer_offs, uint32_t *lens, uint8_t *numbps, const char *who, const double *targets = nullptr,
                                          double *achieved = nullptr) {          // targets: the _quality form (roi nullable), achieved: nlayers doubles or null
    if (!P || !pix || !out_len) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "a synchronising call while the context captures a graph");
    uint64_t budgets[J2K_MAX_LAYERS];
    int r;
    if (targets) r = quality_frame_check(P, targets, nlayers, layer_offs != nullptr, roi, roi_gain, who);
    else if (with_roi) r = roi_frame_check(P, layer_bytes, nlayers, layer_offs != nullptr, roi, roi_gain, budgets, who);
    else {
        r = layers_check(P, nlayers, who);
        if (r == J2K_OK) r = budgets_check(ctx, layer_bytes, nlayers, budgets, who);
    }
    if (r != J2K_OK) return r;
    const PlanSpec &S = P->spec;
    const int pb = format == J2K_PIX_GRAY8 ? 1 : format == J2K_PIX_GRAY16 ? 2 : (format == J2K_PIX_RGBA8 || format == J2K_PIX_NRGBA8) ? 4 :
                   (format == J2K_PIX_RGBA64 || format == J2K_PIX_NRGBA64) ? 8 : 0;
    if (!pb || stride < (size_t)S.W * pb) return fail(ctx, J2K_ERR_INVALID_ARG, "pixel format / stride");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = P->blocks.size(), nt = (size_t)P->tile_count;
    size_t nl = nt * (size_t)nlayers;
    const size_t bound = with_roi ? std::max(j2k_plan_frame_bound_layers(P, nlayers), j2k_plan_frame_bound(P)) : j2k_plan_frame_bound_layers(P, nlayers);
    const size_t toff_at = (bound + 64 + 15) & ~size_t(15);                                  // the tile-parts, and behind them their offsets and the layer ends
    if ((r = ensure_sized(ctx, &P->d_host_pix, &P->host_pix_bytes, (size_t)S.H * stride)) != J2K_OK) return r;
    if ((r = ensure_sized(ctx, &P->d_host_io, &P->host_io_bytes, toff_at + (nt + 1 + nl + 2 + J2K_MAX_LAYERS) * 8)) != J2K_OK) return r;
    uint64_t *d_toffs = reinterpret_cast<uint64_t *>((uint8_t *)P->d_host_io + toff_at), *d_loffs = d_toffs + nt + 1;
    double *d_ach = reinterpret_cast<double *>(d_loffs + nl + 2);                            // (the _quality form: every layer's weighted distortion)
    HIPCHK(ctx, hipMemcpyAsync(P->d_host_pix, pix, (size_t)S.H * stride, hipMemcpyHostToDevice, ctx->stream));
    if (targets) r = j2k_plan_encode_frame_pixels_quality(P, format, P->d_host_pix, stride, sop, eph, targets, nlayers, roi, roi_gain, (uint8_t *)P->d_host_io, bound, d_toffs,
                                                          layer_offs ? d_loffs : nullptr, d_ach);
    else if (with_roi) r = j2k_plan_encode_frame_pixels_roi(P, format, P->d_host_pix, stride, sop, eph, layer_bytes, nlayers, roi, roi_gain, (uint8_t *)P->d_host_io, bound, d_toffs,
                                                       layer_offs ? d_loffs : nullptr);
    else r = j2k_plan_encode_frame_pixels_layers(P, format, P->d_host_pix, stride, sop, eph, layer_bytes, nlayers, (uint8_t *)P->d_host_io, bound, d_toffs, d_loffs);
    if (r != J2K_OK) return r;
    if (with_roi && !layer_offs) nl = 0;                                                     // (the single-budget stream has no layer ends)
    std::vector<uint64_t> offs(nt + 1 + nl, 0);
    HIPCHK(ctx, hipMemcpyAsync(offs.data(), d_toffs, offs.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (lens && nb) HIPCHK(ctx, hipMemcpyAsync(lens, P->d_cl_lens, nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (numbps && nb) HIPCHK(ctx, hipMemcpyAsync(numbps, P->d_cl_numbps, nb, hipMemcpyDeviceToHost, ctx->stream));
    if (targets && achieved) HIPCHK(ctx, hipMemcpyAsync(achieved, d_ach, (size_t)nlayers * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if ((r = check_fault(ctx)) != J2K_OK) return r;
    if ((r = j2k_plan_frame_status(P)) != J2K_OK) return r;
    const size_t total = (size_t)offs[nt];
    *out_len = total;
    if (tile_offs) memcpy(tile_offs, offs.data(), (nt + 1) * 8);
    if (layer_offs && nl) memcpy(layer_offs, offs.data() + nt + 1, nl * 8);
    if (total > cap || (total && !out)) return fail(ctx, J2K_ERR_CAPACITY, "out too small (*out_len says what the tile-parts take)");
    if (total) HIPCHK(ctx, hipMemcpy(out, P->d_host_io, total, hipMemcpyDeviceToHost));
    return J2K_OK;
}

extern "C" int j2k_encode_pixels_host_layers(j2k_plan *P, int format, const void *pix, size_t stride, int sop, int eph, const int64_t *layer_bytes, int nlayers,
                                             uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs, uint64_t *layer_offs, uint32_t *lens, uint8_t *numbps) {
    return encode_pixels_host_layers_impl(P, format, pix, stride, sop, eph, layer_bytes, nlayers, false, nullptr, 1, out, cap, out_len, tile_offs, layer_offs, lens, numbps,
                                          "j2k_encode_pixels_host_layers");
}
// the synchronous host-memory form of j2k_plan_encode_frame_pixels_roi (layer_offs == NULL with nlayers = 1: the single-budget stream)
extern "C" int j2k_encode_pixels_host_roi(j2k_plan *P, int format, const void *pix, size_t stride, int sop, int eph, const int64_t *layer_bytes, int nlayers,
                                          const j2k_rect *roi, int roi_gain, uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs, uint64_t *layer_offs,
                                          uint32_t *lens, uint8_t *numbps) {
    if (!P) return J2K_ERR_INVALID_ARG;
    return encode_pixels_host_layers_impl(P, format, pix, stride, sop, eph, layer_bytes, nlayers, true, roi, roi_gain, out, cap, out_len, tile_offs, layer_offs, lens, numbps,
                                          "j2k_encode_pixels_host_roi");
}

// the synchronous host-memory form of j2k_plan_encode_frame_pixels_quality (layer_offs == NULL with nlayers = 1: the kept-stream format; roi nullable)
extern "C" int j2k_encode_pixels_host_quality(j2k_plan *P, int format, const void *pix, size_t stride, int sop, int eph, const double *targets, int nlayers,
                                              const j2k_rect *roi, int roi_gain, uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs, uint64_t *layer_offs,
                                              uint32_t *lens, uint8_t *numbps, double *achieved) {
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!targets) return fail(P->ctx, J2K_ERR_INVALID_ARG, "j2k_encode_pixels_host_quality: no targets");
    return encode_pixels_host_layers_impl(P, format, pix, stride, sop, eph, nullptr, nlayers, true, roi, roi_gain, out, cap, out_len, tile_offs, layer_offs, lens, numbps,
                                          "j2k_encode_pixels_host_quality", targets, achieved);
}

extern "C" int j2k_decode_pixels_host_layers(j2k_plan *P, const uint8_t *cs, size_t len, int sop, int eph, int layers, int reduce, int skip_planes, void *pix,
                                             size_t stride) {
    if (!P || !cs || !pix) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "a synchronising call while the context captures a graph");
    int r = check_skip_planes(ctx, P->spec.coder, skip_planes, "j2k_decode_pixels_host_layers");
    if (r == J2K_OK) r = layers_check(P, layers, "j2k_decode_pixels_host_layers");
    if (r != J2K_OK) return r;
    const PlanSpec &S = P->spec;
    if (reduce != 0) {
        int32_t wr = 0, hr = 0;
        r = j2k_plan_reduced_size(P, reduce, &wr, &hr);
        if (r != J2K_OK) return r;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t rows = reduce > 0 ? (size_t)(((int64_t)S.H + (((int64_t)1 << reduce) - 1)) >> reduce) : (size_t)S.H;
    const size_t pixbytes = rows * stride;
    if ((r = ensure_sized(ctx, &P->d_host_pix, &P->host_pix_bytes, pixbytes)) != J2K_OK) return r;
    if ((r = ensure_sized(ctx, &P->d_host_io, &P->host_io_bytes, len + 64)) != J2K_OK) return r;
    HIPCHK(ctx, hipMemcpyAsync(P->d_host_io, cs, len, hipMemcpyHostToDevice, ctx->stream));
    r = j2k_plan_decode_frame_pixels_layers(P, (const uint8_t *)P->d_host_io, len, nullptr, sop, eph, layers, reduce, skip_planes, P->d_host_pix, stride);
    if (r != J2K_OK) return r;
    HIPCHK(ctx, hipMemcpyAsync(pix, P->d_host_pix, pixbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return j2k_plan_frame_status(P);
}
