// j2k_area.cpp -- region decode behind the C ABI (include/j2kgfx.h: j2k_plan_area_shape, j2k_plan_area_blocks, j2k_plan_decode_frame_pixels_area,
// j2k_decode_pixels_host_area): the pixels of a rectangle, decoding only the code-blocks it needs.  The need set is computed on the device from the
// rectangle (area.hip; definition: tests/area_cases.py, rule: DESIGN.md 7); everything else is the frame decoder's own stages (plan_decode_frame,
// j2k_frame.cpp, with DecodeRequest.area): the packet parse of the call without `area`, the MQ block decoders on tables in which the other blocks
// are empty, the whole-frame inverse into a staging frame of the plan, and a pack of the window (pixels.hip).  Here: the refusals and the tables.
#include "j2k_host.h"

using namespace j2k;

// every refusal of an area call that its plan, `reduce` and rectangle decide (host only)
int area_check(const j2k_plan *P, const j2k_rect *area, int reduce, AreaOut &out, const char *who) {
    j2k_ctx *ctx = P->ctx;
    const PlanSpec &S = P->spec;
    const std::string w(who);
    if (!S.mallat) return fail(ctx, J2K_ERR_UNSUPPORTED, (w + ": region decode needs a Mallat plan (the prefix layout has no spatial locality below level 0)").c_str());
    if (S.coder != J2K_CODER_MQ) return fail(ctx, J2K_ERR_UNSUPPORTED, (w + ": region decode needs the MQ coder (the HT frame decoder keeps state in its planes)").c_str());
    if (S.frame_h > 0 && S.frame_h < S.H) return fail(ctx, J2K_ERR_UNSUPPORTED, (w + ": region decode of a batch plan (frame_rows)").c_str());
    if (P->tile_count != P->tiles_x * P->tiles_y) return fail(ctx, J2K_ERR_UNSUPPORTED, (w + ": region decode of a shard plan (tile_first / tile_count)").c_str());
    if (reduce < 0 || reduce > S.levels || reduce > 30) return fail(ctx, J2K_ERR_INVALID_ARG, "reduce outside 0 ... decomposition levels");
    const int tw = S.tile_w > 0 ? S.tile_w : S.W, th = S.tile_h > 0 ? S.tile_h : S.H, mask = (1 << reduce) - 1;
    if ((tw < S.W && (tw & mask)) || (th < S.H && (th & mask))) return fail(ctx, J2K_ERR_INVALID_ARG, "reduce: the tile size is not a multiple of 2^reduce");
    if (!area) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": no rectangle").c_str());
    if (area->x0 < 0 || area->y0 < 0 || area->x0 >= area->x1 || area->y0 >= area->y1 || area->x1 > S.W || area->y1 > S.H)
        return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": the rectangle is inverted, empty or outside the frame").c_str());
    auto shr = [&](int v) { return (int)(((int64_t)v + mask) >> reduce); };
    out.x0 = shr(area->x0); out.y0 = shr(area->y0);
    out.w = shr(area->x1) - out.x0; out.h = shr(area->y1) - out.y0;
    if (out.w <= 0 || out.h <= 0) return fail(ctx, J2K_ERR_INVALID_ARG, (w + ": the rectangle is empty after reduce").c_str());
    return J2K_OK;
}

extern "C" int j2k_plan_area_shape(const j2k_plan *P, const j2k_rect *area, int reduce, int *out_w, int *out_h) {
    if (!P || !out_w || !out_h) return J2K_ERR_INVALID_ARG;
    AreaOut o{};
    const int r = area_check(P, area, reduce, o, "j2k_plan_area_shape");
    if (r != J2K_OK) return r;
    *out_w = o.w; *out_h = o.h;
    return J2K_OK;
}

// the plan data of area_blocks_kernel, uploaded at the first area call (or the first region-of-interest encode: j2k_rate.cpp)
int area_tables(j2k_plan *P, bool frame) {
    j2k_ctx *ctx = P->ctx;
    const PlanSpec &S = P->spec;
    if (P->d_area_planes && (!frame || P->d_area_frame)) return J2K_OK;
    if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "capture: the tables of a region decode are made at its first call -- run the call once before j2k_ctx_capture_begin");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (frame && !P->d_area_frame) HIPCHK(ctx, hipMalloc((void **)&P->d_area_frame, (size_t)S.W * S.H * S.C * 4 + 64));
    if (P->d_area_planes) return J2K_OK;
    std::vector<AreaPlane> planes(P->plane_desc.size() / 7);
    for (size_t p = 0; p < planes.size(); p++) {
        const int64_t *d = &P->plane_desc[p * 7];                      // tile, comp, x0, y0, w, h, coefficient offset
        planes[p] = AreaPlane{(int32_t)d[2], (int32_t)d[3], (int32_t)d[4], (int32_t)d[5], S.levels, {0, 0, 0}};
    }
    int r = upload(ctx, &P->d_area_blocks, P->blocks);
    if (r == J2K_OK) r = upload(ctx, &P->d_area_planes, planes);      // (last: its presence says the tables are complete)
    return r;
}

int area_launch(j2k_plan *P, const j2k_rect *area, int reduce, uint8_t *d_need, uint32_t *d_lens, uint8_t *d_numbps, uint8_t *d_floors) {
    j2k_ctx *ctx = P->ctx;
    HIPCHK(ctx, launch_area_blocks(ctx->stream, P->d_area_blocks, (int)P->blocks.size(), P->d_area_planes, area->x0, area->y0, area->x1, area->y1, reduce,
                                   P->spec.wavelet == W97 ? 2 : 1, d_need, d_lens, d_numbps, d_floors));
    return J2K_OK;
}

extern "C" int j2k_plan_area_blocks(j2k_plan *P, const j2k_rect *area, int reduce, uint8_t *d_need) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    AreaOut o{};
    int r = area_check(P, area, reduce, o, "j2k_plan_area_blocks");
    if (r != J2K_OK) return r;
    if (!d_need) return fail(P->ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    r = area_tables(P, false);
    if (r != J2K_OK) return r;
    return area_launch(P, area, reduce, d_need, nullptr, nullptr, nullptr);
}

extern "C" int j2k_plan_decode_frame_pixels_area(j2k_plan *P, const uint8_t *d_cs, size_t len, const uint64_t *d_tile_offs, int sop, int eph, int layers, int truncated,
                                                 int reduce, int skip_planes, const j2k_rect *area, void *d_pix, size_t stride) {
    graph_note_plan(P);
    if (!P) return J2K_ERR_INVALID_ARG;
    j2k_ctx *ctx = P->ctx;
    const PlanSpec &S = P->spec;
    AreaOut o{};
    int r = area_check(P, area, reduce, o, "j2k_plan_decode_frame_pixels_area");
    if (r == J2K_OK) r = check_skip_planes(ctx, S.coder, skip_planes, "j2k_plan_decode_frame_pixels_area");
    if (r != J2K_OK) return r;
    if (layers < 0 || layers > J2K_MAX_LAYERS) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_plan_decode_frame_pixels_area: the layer count is 1 ... 32 (0: not a layered stream)");
    if (layers > 0 && (r = rate_check(P, "j2k_plan_decode_frame_pixels_area")) != J2K_OK) return r;
    if (truncated && (r = raw_magref_refuse(P, "j2k_plan_decode_frame_pixels_area (truncated)")) != J2K_OK) return r;
    if (!d_cs || !d_pix) return fail(ctx, J2K_ERR_INVALID_ARG, "null device pointer");
    // decoder.createImage's formats, as j2k_pack_pixels checks them
    if (S.precision < 1 || S.precision > 16 || (S.C != 1 && S.C != 3 && S.C != 4)) return fail(ctx, J2K_ERR_UNSUPPORTED, "unsupported number of components / precision");
    const size_t bpp = (size_t)(S.C == 1 ? 1 : 4) * (S.precision > 8 ? 2 : 1);
    if (stride < (size_t)o.w * bpp) return fail(ctx, J2K_ERR_INVALID_ARG, "j2k_plan_decode_frame_pixels_area: stride smaller than a row of the rectangle");
    if (S.C != 1 && S.precision <= 8 && (((uintptr_t)d_pix | stride) & 3)) return fail(ctx, J2K_ERR_INVALID_ARG, "RGBA rows must be 4-byte aligned");
    DecodeRequest q;
    q.layers = layers; q.truncated = truncated != 0; q.reduce = reduce; q.skip_planes = skip_planes; q.area = area;
    return plan_decode_frame(P, d_cs, len, d_tile_offs, sop, eph, q, &o, d_pix, stride);
}

extern "C" int j2k_decode_pixels_host_area(j2k_plan *P, const uint8_t *cs, size_t len, int sop, int eph, int layers, int truncated, int reduce, int skip_planes,
                                           const j2k_rect *area, void *pix, size_t stride) {
    graph_note_plan(P);
    const int c = host_call_check(P, cs, pix);
    if (c != J2K_OK) return c;
    AreaOut o{};
    const int r = area_check(P, area, reduce, o, "j2k_decode_pixels_host_area");
    if (r != J2K_OK) return r;
    // (the status is read before the copy back -- it synchronises; a refused stream wrote nothing: pix stays as it is)
    return decode_host(P, cs, len, (size_t)o.h * stride, pix, true, [&](const uint8_t *d_cs, void *d_pix) {
        return j2k_plan_decode_frame_pixels_area(P, d_cs, len, nullptr, sop, eph, layers, truncated, reduce, skip_planes, area, d_pix, stride);
    });
}
