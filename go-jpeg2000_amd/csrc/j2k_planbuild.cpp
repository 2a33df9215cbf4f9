// j2k_planbuild.cpp -- plans: a frame geometry compiled into device job tables (C ABI of libj2kgfx.so, include/j2kgfx.h; shared declarations: j2k_host.h)
// The tables themselves are made by build_plan_tables (plan_tables.cpp, no HIP in it); this file uploads them and owns the device memory.
#include "j2k_host.h"

using namespace j2k;

// ------------------------------------------------------------------------------
// the device tables of a plan: THE list of (device pointer, host vector) pairs.  build_plan uploads along it, j2k_plan_destroy frees along
// it (with no tables: `f` then sees empty vectors), so a table added here cannot be uploaded and never freed.
// ------------------------------------------------------------------------------
template <class F>
static void level_device_tables(LevelTab &D, const LevelTables &T, F f) { f(D.d_planes, T.planes); f(D.d_jobs, T.jobs); f(D.d_pjobs, T.pjobs); }
template <class F>
static void plan_device_tables(j2k_plan &P, const PlanTables &T, F f) {
    static const LevelTables no_level;
    static const std::vector<int32_t> none;
    for (int cls = 0; cls < 2; cls++) {
        for (size_t l = 0; l < P.fwd[cls].size(); l++) level_device_tables(P.fwd[cls][l], l < T.fwd[cls].size() ? T.fwd[cls][l] : no_level, f);
        for (size_t l = 0; l < P.inv[cls].size(); l++) level_device_tables(P.inv[cls][l], l < T.inv[cls].size() ? T.inv[cls][l] : no_level, f);
    }
    f(P.d_tail, T.tail); f(P.d_deep_planes, T.deep_planes); f(P.d_deep_jobs, T.deep_jobs); f(P.d_deep_jobs_inv, T.deep_jobs_inv);
    f(P.d_mega_fwd_jobs, T.mega_fwd_jobs); f(P.d_mega_inv_jobs, T.mega_inv_jobs); f(P.d_fwd_top_jobs, T.fwd_top_jobs); f(P.d_inv_top_jobs, T.inv_top_jobs);
    f(P.d_fwd_pix_jobs, T.fwd_pix_jobs); f(P.d_fwd_wg_jobs, T.fwd_wg_jobs); f(P.d_inv_wg_jobs, T.inv_wg_jobs);
    f(P.d_fwd_wg2_jobs, T.fwd_wg2_jobs); f(P.d_fwd_wg_rest_jobs, T.fwd_wg_rest_jobs); f(P.d_fwd97_wg_jobs, T.fwd97_wg_jobs); f(P.d_inv97_wg_jobs, T.inv97_wg_jobs);
    f(P.d_tile_job0, T.tile_job0); f(P.d_bjobs, T.bjobs); f(P.d_djobs, T.djobs); f(P.d_djobs_placed, T.djobs_placed);
    f(P.d_ht_ujobs, T.ht_ujobs); f(P.d_ht_alias_next, T.ht_alias_next); f(P.d_bjobs_alias, T.bjobs_alias);
    // (the leaders and the walk's order: the host keeps them in any HT plan; device tables only when some job has a follower)
    f(P.d_ht_dec_rep, T.ht_dec_any ? T.ht_dec_rep : none); f(P.d_ht_dec_fol, T.ht_dec_fol);
    f(P.d_ht_walk_order, T.ht_dec_any ? T.ht_walk_order : none); f(P.d_ht_walk_pos, T.ht_walk_pos);
}

// ------------------------------------------------------------------------------
// plan construction: the tables (plan_tables.cpp), their upload, the scratch buffers
// ------------------------------------------------------------------------------
int build_plan(j2k_ctx *ctx, const PlanSpec &S, j2k_plan **out) {
    PlanTables T;
    const char *why = "";
    int r = build_plan_tables(*ctx, PlanLimits{ht_fast_max_samples(), ht_walk_max_pairs()}, S, T, &why);
    if (r != J2K_OK) return fail(ctx, r, why);
    j2k_plan *P = new j2k_plan();
    P->ctx = ctx;
    P->serial = ctx->guard.plan_created();
    P->spec = S;
    for (int cls = 0; cls < 2; cls++) {
        P->fwd[cls].resize(T.fwd[cls].size()); P->inv[cls].resize(T.inv[cls].size());
        for (size_t l = 0; l < T.fwd[cls].size(); l++) { static_cast<LevelInfo &>(P->fwd[cls][l]) = T.fwd[cls][l]; static_cast<LevelInfo &>(P->inv[cls][l]) = T.inv[cls][l]; }
    }
    plan_device_tables(*P, T, [&](auto *&d, const auto &v) { if (r == J2K_OK) r = upload(ctx, &d, v); });
    static_cast<PlanScalars &>(*P) = std::move(static_cast<PlanScalars &>(T));
    const size_t esz = S.wavelet == W97 ? 8 : 4;
    auto alloc = [&](void **p, size_t bytes, const char *what) {
        if (r != J2K_OK || !bytes) return;
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) r = fail_hip(ctx, e, what);
    };
    alloc(&P->d_scrA, (size_t)P->scrA_elems * esz, "hipMalloc scratch A");
    alloc(&P->d_scrB, (size_t)P->scrB_elems * esz, "hipMalloc scratch B");
    if (P->scr16_inv) alloc((void **)&P->d_scr16_fmt, (size_t)P->scrA_elems / 8 + 16, "hipMalloc scratch format table");
    if (r != J2K_OK) { j2k_plan_destroy(P); return r; }
    *out = P;
    return J2K_OK;
}

// ------------------------------------------------------------------------------
// Mallat plans, reduced-resolution decode: the tables of one `reduce` (plan_tables.cpp: build_reduced_tables)
// ------------------------------------------------------------------------------
template <class F>
static void reduced_device_tables(ReducedTab &D, const ReducedTables &T, F f) {
    for (int cls = 0; cls < 2; cls++) level_device_tables(D.inv[cls], T.inv[cls], f);
    f(D.d_ll, T.ll); f(D.d_ids, T.ids); f(D.d_bjobs, T.bjobs); f(D.d_djobs, T.djobs); f(D.d_placed, T.placed);
}
static void free_reduced(ReducedTab &R) {
    reduced_device_tables(R, ReducedTables(), [](auto *&d, const auto &) { if (d) (void)hipFree(d); });
    void *rp[] = {R.d_offs, R.d_lens, R.d_numbps};
    for (void *p : rp) if (p) (void)hipFree(p);
    R = ReducedTab();
}

int plan_reduced(j2k_plan *P, int reduce, ReducedTab **out) {
    j2k_ctx *ctx = P->ctx;
    const char *why = "";
    int r = check_reduce(P->spec, reduce, &why);
    if (r != J2K_OK) return fail(ctx, r, why);
    *out = nullptr;
    if (reduce == 0) return J2K_OK;      // exactly the call without it: nothing is built (so nothing stands in the way of a capture)
    if (P->reduced.empty()) P->reduced.resize((size_t)P->spec.levels + 1);
    ReducedTab &R = P->reduced[(size_t)reduce];
    *out = &R;
    if (R.built) return J2K_OK;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: the tables of a `reduce` are made at its first use -- run the call once before j2k_ctx_capture_begin");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ReducedTables T;
    if ((r = build_reduced_tables(*ctx, P->spec, *P, reduce, T, &why)) != J2K_OK) return fail(ctx, r, why);
    static_cast<ReducedInfo &>(R) = T;
    for (int cls = 0; cls < 2; cls++) static_cast<LevelInfo &>(R.inv[cls]) = T.inv[cls];
    reduced_device_tables(R, T, [&](auto *&d, const auto &v) { if (r == J2K_OK) r = upload(ctx, &d, v); });
    const size_t m = T.ids.size();
    auto alloc = [&](void **p, size_t bytes) { if (r == J2K_OK) { hipError_t e = hipMalloc(p, bytes); if (e != hipSuccess) r = fail_hip(ctx, e, "hipMalloc (reduced decode)"); } };
    alloc((void **)&R.d_offs, (m + 1) * 8 + 16);
    alloc((void **)&R.d_lens, m * 4 + 16);
    alloc((void **)&R.d_numbps, m + 16);
    if (r != J2K_OK) { free_reduced(R); return r; }      // (a later call starts again from nothing)
    R.built = true;
    return J2K_OK;
}

extern "C" int j2k_plan_reduced_size(const j2k_plan *P, int reduce, int32_t *width, int32_t *height) {
    if (!P || !width || !height) return J2K_ERR_INVALID_ARG;
    const PlanSpec &S = P->spec;
    if (!S.mallat) return fail(P->ctx, J2K_ERR_UNSUPPORTED, "reduced-resolution decode needs a Mallat plan (j2k_params.closed_loop = J2K_CLOSED_LOOP_MALLAT)");
    if (reduce < 0 || reduce > S.levels) return fail(P->ctx, J2K_ERR_INVALID_ARG, "reduce outside 0 ... decomposition levels");
    const int64_t m = ((int64_t)1 << reduce) - 1;
    *width = (int32_t)(((int64_t)S.W + m) >> reduce);          // decoder.go:289-295: (w + 1) / 2 per step
    *height = (int32_t)(((int64_t)S.H + m) >> reduce);
    return J2K_OK;
}

extern "C" void j2k_plan_destroy(j2k_plan *P) {
    if (!P) return;
    if (P->ctx) { (void)hipSetDevice(P->ctx->device); (void)hipStreamSynchronize(P->ctx->stream); }
    // every graph that recorded a call of this plan is stale from here on (graph_guard.h, cause (c)): everything below is freed.  The serial is
    // not given out again, so a plan made later at this address does not bring those graphs back.  (Not graph_note_plan: nothing is recorded.)
    if (P->ctx) P->ctx->guard.plan_destroyed(P->serial);
    for (ReducedTab &R : P->reduced) free_reduced(R);
    free_layer_tabs(P);
    plan_device_tables(*P, PlanTables(), [](auto *&d, const auto &) { if (d) (void)hipFree(d); d = nullptr; });
    // the buffers of build_plan and the first-use tables and workspaces of the other files
    void *ptrs[] = {P->d_scrA, P->d_scrB, P->d_scr16_fmt, P->d_bigsym_off, P->d_frame, P->d_coeff, P->d_slots, P->d_stream, P->d_lens, P->d_numbps, P->d_offs, P->d_status, P->d_maglens, P->d_mels, P->d_toffs,
                    P->d_t2_packets, P->d_tile_packet0, P->d_t2_cbs, P->d_t2_poffs, P->d_t2_ptile, P->d_t2_ws, P->d_t2_chains, P->d_t2_body_base, P->d_t2_par, P->d_frame_status,
                    P->d_cl_decoded, P->d_cl_coeff, P->d_cl_coeff_dec, P->d_cl_numbps, P->d_cl_offs, P->d_cl_lens, P->d_host_io, P->d_host_pix,
                    P->d_rate_wj, P->d_rate_ws, P->d_rate_frames, P->d_rate_fvals, P->d_cl_rate, P->d_cl_prate, P->d_cl_dense, P->d_cl_lfloors,
                    P->d_area_blocks, P->d_area_planes, P->d_area_frame};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    delete P;
}

static int spec_from_params(j2k_ctx *ctx, const j2k_params *p, PlanSpec &S) {
    if (!p) return fail(ctx, J2K_ERR_INVALID_ARG, "params == NULL");
    if (p->precision < 1 || p->precision > 31) return fail(ctx, J2K_ERR_INVALID_ARG, "precision out of range");
    S.W = p->width; S.H = p->height; S.C = p->ncomp;
    S.frame_h = p->frame_rows > 0 ? p->frame_rows : p->height;
    if (S.frame_h > 0 && p->height % S.frame_h) return fail(ctx, J2K_ERR_INVALID_ARG, "height is not a whole number of frames (frame_rows)");
    S.tile_w = p->tile_w; S.tile_h = p->tile_h;
    S.levels = p->num_resolutions - 1;
    if (S.levels <= 0) S.levels = 5;                                  // encoder.go:249-252
    S.wavelet = p->lossless ? W53 : W97;
    S.precision = p->precision;
    S.dc_shift = (int)((uint32_t)1 << (p->precision - 1));            // mct.go:97: encoder.preprocess ALWAYS shifts (encoder.go:218-220)
    S.dc_shift_inv = p->is_signed ? 0 : S.dc_shift;                   // decoder.go:344-348: only the decode side skips it for signed components
    S.mct = p->ncomp >= 3;                                            // encoder.go:223
    S.quant = p->lossless ? Q_NONE : Q_ENCODER;
    S.quality = p->quality > 0 ? p->quality : 100;                    // encoder.go:265-268
    S.num_res_jobs = p->num_resolutions > 0 ? p->num_resolutions : 6; // encoder.go:601-604
    S.cb_w = p->cb_w > 0 ? p->cb_w : 64;                              // encoder.go:608-613
    S.cb_h = p->cb_h > 0 ? p->cb_h : 64;
    S.coder = p->coder;
    S.tile_first = p->tile_first; S.tile_count = p->tile_count;
    S.closed_loop = p->closed_loop != 0;
    S.mallat = p->closed_loop == J2K_CLOSED_LOOP_MALLAT;
    if (S.coder != J2K_CODER_MQ && S.coder != J2K_CODER_HT) return fail(ctx, J2K_ERR_INVALID_ARG, "coder");
    if (S.coder == J2K_CODER_MQ && !ctx->counted_mq) { ctx->counted_mq = true; g_mq_ctxs.fetch_add(1, std::memory_order_relaxed); }
    return J2K_OK;
}

extern "C" int j2k_plan_create(j2k_ctx *ctx, const j2k_params *params, j2k_plan **out) {
    if (!ctx || !out) return J2K_ERR_INVALID_ARG;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PlanSpec S;
    int r = spec_from_params(ctx, params, S);
    if (r != J2K_OK) return r;
    return build_plan(ctx, S, out);
}

extern "C" int j2k_plan_get_info(const j2k_plan *P, j2k_plan_info *info) {
    if (!P || !info) return J2K_ERR_INVALID_ARG;
    info->tiles = P->tile_count;
    info->planes = (int64_t)P->plane_desc.size() / 7;
    info->blocks = (int64_t)P->blocks.size();
    info->coeff_elems = P->coeff_elems;
    info->bytes_cap = P->bytes_cap;
    info->dwt_bytes = P->dwt_bytes;
    info->dwt_level0_bytes = P->dwt_level0_bytes;
    info->block_samples = P->block_samples;
    info->decoded_elems = P->decoded_elems;
    return J2K_OK;
}
extern "C" int j2k_plan_get_blocks(const j2k_plan *P, j2k_block *blocks, size_t cap) {
    if (!P || (!blocks && cap)) return J2K_ERR_INVALID_ARG;
    if (cap < P->blocks.size()) return J2K_ERR_CAPACITY;
    if (!P->blocks.empty()) memcpy(blocks, P->blocks.data(), P->blocks.size() * sizeof(j2k_block));
    return J2K_OK;
}
extern "C" int j2k_plan_get_planes(const j2k_plan *P, int64_t *desc7, size_t cap_planes) {
    if (!P || !desc7) return J2K_ERR_INVALID_ARG;
    if (cap_planes * 7 < P->plane_desc.size()) return J2K_ERR_CAPACITY;
    memcpy(desc7, P->plane_desc.data(), P->plane_desc.size() * sizeof(int64_t));
    return J2K_OK;
}
