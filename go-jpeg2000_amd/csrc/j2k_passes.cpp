// j2k_passes.cpp -- pass-level rate control behind the C ABI: MQ blocks cut at coding-pass ends, not only at bit-plane ends (kernels: t1.hip's PASSES
// and PASSCUT instantiations, rate.hip's pass tables, the pass forms of t2dev.hip / t2dec.hip).  include/j2kgfx.h has the contract,
// tests/pass_cases.py the definition, DESIGN.md 7 the argument.  Every call here is a sibling of a plane-cut call and refuses what that refuses.
#include <cmath>

#include "j2k_host.h"

using namespace j2k;

// ---- stage calls ----------------------------------------------------------------------------------------------------------------------------
int plan_encode_blocks_passes(j2k_plan *P, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps, uint32_t *d_rate, uint64_t *d_dist,
                              uint64_t *d_spmask) {
    int r = plan_encode_blocks_impl(P, d_coeff, d_slots, d_lens, d_numbps, d_rate, d_spmask);
    if (r != J2K_OK) return r;
    j2k_ctx *ctx = P->ctx;
    HIPCHK(ctx, launch_rate_distortion_passes(ctx->stream, P->d_bjobs, (int)P->blocks.size(), d_coeff, d_numbps, d_spmask, d_dist));
    return J2K_OK;
}

extern "C" int j2k_plan_encode_blocks_passes(j2k_plan *P, const int32_t *d_coeff, uint8_t *d_slots, uint32_t *d_lens, uint8_t *d_numbps, uint32_t *d_rate,
                                             uint64_t *d_dist, uint64_t *d_spmask) {
    graph_note_plan(P);
    if (!P || !d_coeff || !d_slots || !d_lens || !d_numbps || !d_rate || !d_dist || !d_spmask) return J2K_ERR_INVALID_ARG;
    const int r = rate_check(P, "j2k_plan_encode_blocks_passes");
    if (r != J2K_OK) return r;
    return plan_encode_blocks_passes(P, d_coeff, d_slots, d_lens, d_numbps, d_rate, d_dist, d_spmask);
}

extern "C" int j2k_plan_rate_allocate_passes(j2k_plan *P, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps, int64_t max_body_bytes,
                                             uint8_t *d_kept, uint64_t *d_chosen) {
    graph_note_plan(P);
    if (!P || !d_rate || !d_dist || !d_numbps || !d_kept || !d_chosen) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    int r = rate_check(P, "j2k_plan_rate_allocate_passes");
    if (r != J2K_OK) return r;
    if (max_body_bytes < 0) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_plan_rate_allocate_passes: a negative budget");
    EncodeRequest q;
    q.kind = EncodeRequest::BYTES;
    q.budgets[0] = (uint64_t)max_body_bytes;
    q.passes = true;
    return rate_allocate_launch(P, q, d_rate, d_dist, d_numbps, d_kept, d_chosen, nullptr);
}

extern "C" int j2k_plan_rate_allocate_quality_passes(j2k_plan *P, const uint32_t *d_rate, const uint64_t *d_dist, const uint8_t *d_numbps, double target,
                                                     uint8_t *d_kept, uint64_t *d_chosen, double *d_achieved) {
    graph_note_plan(P);
    if (!P || !d_rate || !d_dist || !d_numbps || !d_kept || !d_chosen || !d_achieved) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    int r = rate_check(P, "j2k_plan_rate_allocate_quality_passes");
    if (r == J2K_OK) r = targets_check(ctx, &target, 1, "j2k_plan_rate_allocate_quality_passes");
    if (r != J2K_OK) return r;
    EncodeRequest q;
    q.kind = EncodeRequest::DISTORTION;
    q.targets[0] = target;
    q.passes = true;
    return rate_allocate_launch(P, q, d_rate, d_dist, d_numbps, d_kept, d_chosen, d_achieved);
}

// j2k_plan_encode_tile_parts_kept with d_kept[j] a pass count q <= 3 numBPS - 2: the block's bytes are the prefix d_rate[j * 96 + q], its header carries q
// passes (none, and no bytes, for q = 0), ZeroBitPlanes as before.  d_kept[j] = 3 numBPS - 2 everywhere gives j2k_plan_encode_tile_parts' bytes.
extern "C" int j2k_plan_encode_tile_parts_kept_passes(j2k_plan *P, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
                                                      const uint8_t *d_kept, const uint32_t *d_rate, int sop, int eph, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    if (!d_stream || !d_offs || !d_lens || !d_numbps || !d_kept || !d_rate || !d_out || !d_tile_offs) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    int r = rate_check(P, "j2k_plan_encode_tile_parts_kept_passes");
    if (r != J2K_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    r = cl_prepare(P);
    if (r != J2K_OK) return r;
    return encode_tile_parts_impl(P, d_stream, d_offs, d_lens, d_numbps, sop, eph, d_out, cap, d_tile_offs, d_kept, d_rate, 1);
}

// j2k_plan_decode_tile_parts_floors at pass granularity: d_pfloors[j] = the coding passes block j's header leaves undecoded, 3 floor - s with
// s = (passes + 2) % 3 (0 for an uncut block); d_numbps as that call.  j2k_plan_decode_blocks_pfloors decodes them.
extern "C" int j2k_plan_decode_tile_parts_pfloors(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, uint64_t *d_offs,
                                                  uint32_t *d_lens, uint8_t *d_numbps, uint8_t *d_pfloors) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!d_pfloors) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    const int r = rate_check(P, "j2k_plan_decode_tile_parts_pfloors");
    if (r != J2K_OK) return r;
    return decode_tile_parts_impl(P, d_cs, len, d_tile_offs, sop, eph, d_offs, d_lens, d_numbps, nullptr, d_pfloors);
}

// Block j stops f = max(3 skip_planes, d_pfloors[j]) coding passes short of its last: whole planes down to ceil(f / 3), then the first
// 3 ceil(f / 3) - f passes of the next plane; every sample takes the midpoint of what ITS last pass left (tests/pass_cases.py: coarse_pass).
extern "C" int j2k_plan_decode_blocks_pfloors(j2k_plan *P, const uint8_t *d_stream, const uint64_t *d_offs, const uint32_t *d_lens, const uint8_t *d_numbps,
                                              int skip_planes, const uint8_t *d_pfloors, int32_t *d_decoded) {
    graph_note_plan(P);
    if (!P || !d_stream || !d_offs || !d_lens || !d_numbps || !d_pfloors || !d_decoded) return J2K_ERR_INVALID_ARG;
    int r = check_skip_planes(P->ctx, P->spec.coder, skip_planes, "j2k_plan_decode_blocks_pfloors");
    if (r == J2K_OK) r = rate_check(P, "j2k_plan_decode_blocks_pfloors");
    if (r != J2K_OK) return r;
    return plan_decode_blocks_jobs(P, P->d_djobs, (int)P->blocks.size(), d_stream, d_offs, d_lens, d_numbps, d_decoded, nullptr, skip_planes, nullptr, d_pfloors);
}

// ---- frame calls ----------------------------------------------------------------------------------------------------------------------------
// one budget (target == NULL) or one distortion target -> the request of the one frame encoder; every refusal before the first launch
static int passes_request(j2k_plan *P, const char *who, int64_t max_body_bytes, const double *target, double *d_achieved, EncodeRequest &q) {
    const int r = encode_request(P, who, target ? nullptr : &max_body_bytes, target, 1, false, false, nullptr, 1, d_achieved, q);
    if (r != J2K_OK) return r;
    q.passes = true;
    return J2K_OK;
}

extern "C" int j2k_plan_encode_frame_pixels_passes(j2k_plan *P, int format, const void *d_pix, size_t stride, int sop, int eph, int64_t max_body_bytes,
                                                   const double *target, uint8_t *d_out, size_t cap, uint64_t *d_tile_offs, double *d_achieved) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    if (!d_out || !d_tile_offs) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    EncodeRequest q;
    const int r = passes_request(P, "j2k_plan_encode_frame_pixels_passes", max_body_bytes, target, d_achieved, q);
    if (r != J2K_OK) return r;
    return plan_encode_frame_cl(P, q, [&](int32_t *d_coeff) { return j2k_plan_forward_pixels(P, format, d_pix, stride, d_coeff); }, sop, eph, d_out, cap, d_tile_offs,
                                nullptr);
}

extern "C" int j2k_encode_pixels_host_passes(j2k_plan *P, int format, const void *pix, size_t stride, int sop, int eph, int64_t max_body_bytes, const double *target,
                                             uint8_t *out, size_t cap, size_t *out_len, uint64_t *tile_offs, uint32_t *lens, uint8_t *numbps, double *achieved) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    EncodeRequest q;
    int r = host_call_check(P, pix, out_len);
    if (r == J2K_OK) r = passes_request(P, "j2k_encode_pixels_host_passes", max_body_bytes, target, nullptr, q);
    if (r != J2K_OK) return r;
    return encode_pixels_host(P, format, pix, stride, q, true, j2k_plan_frame_bound(P), sop, eph, out, cap, out_len, tile_offs, nullptr, lens, numbps, achieved);
}

// j2k_plan_decode_frame_pixels_rate at pass granularity; area (or null): only that rectangle, as j2k_plan_decode_frame_pixels_area returns it
extern "C" int j2k_plan_decode_frame_pixels_passes(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, int reduce,
                                                   int skip_planes, const j2k_rect *area, void *d_pix, size_t stride) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    const PlanSpec &S = P->spec;
    AreaOut o{};
    int r = check_skip_planes(ctx, S.coder, skip_planes, "j2k_plan_decode_frame_pixels_passes");
    if (r == J2K_OK) r = rate_check(P, "j2k_plan_decode_frame_pixels_passes");
    if (r == J2K_OK && area) r = area_check(P, area, reduce, o, "j2k_plan_decode_frame_pixels_passes");
    if (r != J2K_OK) return r;
    if (!d_cs || !d_pix) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    if (area) {                                                      // the packed window's own conditions (j2k_plan_decode_frame_pixels_area)
        if (S.precision < 1 || S.precision > 16 || (S.C != 1 && S.C != 3 && S.C != 4)) return fail(ctx, J2K_ERR_UNSUPPORTED, "unsupported number of components / precision");
        const size_t bpp = (size_t)(S.C == 1 ? 1 : 4) * (S.precision > 8 ? 2 : 1);
        if (stride < (size_t)o.w * bpp) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_plan_decode_frame_pixels_passes: stride smaller than a row of the rectangle");
        if (S.C != 1 && S.precision <= 8 && (((uintptr_t)d_pix | stride) & 3)) return fail(ctx, J2K_ERR_INVALID_ARG, "RGBA rows must be 4-byte aligned");
    }
    DecodeRequest q;
    q.truncated = true; q.passes = true; q.reduce = reduce; q.skip_planes = skip_planes; q.area = area;
    return plan_decode_frame(P, d_cs, len, d_tile_offs, sop, eph, q, area ? &o : nullptr, d_pix, stride);
}

extern "C" int j2k_decode_pixels_host_passes(j2k_plan *P, const uint8_t *cs, size_t len, int sop, int eph, int reduce, int skip_planes, const j2k_rect *area,
                                             void *pix, size_t stride) {
    graph_note_plan(P);
    int r = host_call_check(P, cs, pix);
    if (r != J2K_OK) return r;
    AreaOut o{};
    r = check_skip_planes(P->ctx, P->spec.coder, skip_planes, "j2k_decode_pixels_host_passes");
    if (r == J2K_OK) r = rate_check(P, "j2k_decode_pixels_host_passes");
    if (r == J2K_OK && area) r = area_check(P, area, reduce, o, "j2k_decode_pixels_host_passes");
    int32_t wr = 0, hr = 0;
    if (r == J2K_OK && !area && reduce != 0) r = j2k_plan_reduced_size(P, reduce, &wr, &hr);
    if (r != J2K_OK) return r;
    const size_t rows = area ? (size_t)o.h : reduced_rows(P->spec.H, reduce);
    // (with a rectangle the status is read before the copy back, as in j2k_decode_pixels_host_area: a refused stream leaves pix alone)
    return decode_host(P, cs, len, rows * stride, pix, area != nullptr, [&](const uint8_t *d_cs, void *d_pix) {
        return j2k_plan_decode_frame_pixels_passes(P, d_cs, len, nullptr, sop, eph, reduce, skip_planes, area, d_pix, stride);
    });
}
