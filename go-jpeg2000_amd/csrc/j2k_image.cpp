// j2k_image.cpp -- the default branch of encoder.extractImageData (encoder.go:178-195) for *image.YCbCr, *image.CMYK and
// *image.Paletted (C ABI of libj2kgfx.so, include/j2kgfx.h): the image's colours are a packed RGBA8 frame's, so every call is the
// J2K_PIX_RGBA8 call on them -- staged through an RGBA8 frame (image.hip), or, for YCbCr 4:4:4 / 4:2:2 / 4:2:0, read by the 5-3
// level-0 workgroup kernel itself (dwt53_l0pix_fwd_body.inc).  The closed-loop frame call is in j2k_frame.cpp, the host one-call
// form in j2k_hostcalls.cpp.
#include "j2k_host.h"

using namespace j2k;

static bool go_ratio_ok(int r) { return r >= J2K_YCBCR_444 && r <= J2K_YCBCR_410; }

// Bytes of each plane the rectangle reaches (the largest offset + 1; 0 for an empty image): Go indexes its slices up to there.
// J2K_ERR_INVALID_ARG for what is not an image of these types at all.
int image_device_bytes(const j2k_image *img, uint64_t need[3]) {
    need[0] = need[1] = need[2] = 0;
    if (!img || img->width < 0 || img->height < 0) return J2K_ERR_INVALID_ARG;
    const int64_t w = img->width, h = img->height;
    if ((int64_t)img->min_x + w > INT32_MAX || (int64_t)img->min_y + h > INT32_MAX) return J2K_ERR_INVALID_ARG;
    const int nplanes = img->kind == J2K_IMG_YCBCR ? 3 : 1;
    int64_t row[3] = {0, 0, 0}, rows[3] = {h, h, h};
    switch (img->kind) {
    case J2K_IMG_YCBCR: {
        if (!go_ratio_ok(img->ratio)) return J2K_ERR_INVALID_ARG;
        const int hd = ycc_hdiv(img->ratio), vd = ycc_vdiv(img->ratio);
        const int mx = img->min_x, my = img->min_y, xl = (int)(mx + w - 1), yl = (int)(my + h - 1);
        row[0] = w;
        row[1] = row[2] = w ? (int64_t)(xl / hd - mx / hd) + 1 : 0;        // Go's truncating `/`, as COffset
        rows[1] = rows[2] = h ? (int64_t)(yl / vd - my / vd) + 1 : 0;
        break;
    }
    case J2K_IMG_CMYK: row[0] = 4 * w; break;
    case J2K_IMG_PALETTED:
        if (img->npal < 0 || img->npal > 256 || (img->npal && !img->palette)) return J2K_ERR_INVALID_ARG;
        row[0] = w;
        break;
    default: return J2K_ERR_INVALID_ARG;
    }
    for (int k = 0; k < nplanes; k++) {
        if (img->stride[k] < row[k]) return J2K_ERR_INVALID_ARG;
        if (w && h) need[k] = (uint64_t)((rows[k] - 1) * img->stride[k] + row[k]);
        if (need[k] && img->len[k] >= need[k] && !img->plane[k]) return J2K_ERR_INVALID_ARG;
    }
    return J2K_OK;
}

extern "C" int j2k_image_validate(const j2k_image *img, int width, int height) {
    uint64_t need[3];
    const int r = image_device_bytes(img, need);
    if (r != J2K_OK) return r;
    if ((width >= 0 && img->width != width) || (height >= 0 && img->height != height)) return J2K_ERR_INVALID_ARG;
    for (int k = 0; k < 3; k++)
        if (need[k] > img->len[k]) return J2K_ERR_GO_PANIC;           // index out of range
    if (img->kind == J2K_IMG_PALETTED && img->npal == 0 && img->width && img->height) return J2K_ERR_GO_PANIC;   // At returns nil
    return J2K_OK;
}

static int image_check(j2k_ctx *ctx, const j2k_image *img, int width, int height) {
    const int r = j2k_image_validate(img, width, height);
    if (r == J2K_ERR_GO_PANIC)
        return fail(ctx, r, "image: a plane shorter than the rectangle reaches, or an empty palette (Go panics in At)");
    if (r != J2K_OK) return fail(ctx, r, "image: unknown kind / ratio, a stride shorter than a row, or dims other than the plan's");
    return J2K_OK;
}

// d_img -> packed RGBA8 at d_pix; a palette index >= npal goes to *status_word when given, else the call synchronises and returns
// J2K_ERR_GO_PANIC (flag_word: a device int the call may use for that)
static int convert_rgba8(j2k_ctx *ctx, const j2k_image *d_img, uint32_t *d_pix, size_t stride_px, int *status_word, int *flag_word) {
    const bool pal = d_img->kind == J2K_IMG_PALETTED;
    int *flag = status_word ? status_word : flag_word;
    if (pal && !status_word) HIPCHK(ctx, hipMemsetAsync(flag_word, 0, sizeof(int), ctx->stream));
    HIPCHK(ctx, launch_image_to_rgba8(ctx->stream, *d_img, d_pix, stride_px, flag));
    if (pal && !status_word) {
        if (ctx->capturing) return fail(ctx, J2K_ERR_INVALID_ARG, "a paletted image synchronises (its index check): not while the context captures a graph");
        int f = 0;
        HIPCHK(ctx, hipMemcpyAsync(&f, flag_word, sizeof f, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (f) return fail(ctx, J2K_ERR_GO_PANIC, "image: a palette index >= len(Palette) (Go: index out of range)");
    }
    return J2K_OK;
}

extern "C" int j2k_image_to_rgba8(j2k_ctx *ctx, const j2k_image *img, void *d_pix, size_t stride) {
    if (!ctx || !img || !d_pix) return J2K_ERR_INVALID_ARG;
    int r = image_check(ctx, img, -1, -1);
    if (r != J2K_OK) return r;
    if (stride < (size_t)img->width * 4 || (((uintptr_t)d_pix | stride) & 3)) return fail(ctx, J2K_ERR_INVALID_ARG, "bad RGBA8 stride / alignment");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((r = stage_reserve(ctx, 0, 64)) != J2K_OK) return r;
    return convert_rgba8(ctx, img, (uint32_t *)d_pix, stride / 4, nullptr, (int *)ctx->stage[0]);
}

// the host planes at 256-byte aligned offsets of a device buffer, the palette behind them; returns the bytes it takes
size_t image_layout(const j2k_image *img, const uint64_t need[3], size_t off[4]) {
    size_t at = 0;
    for (int k = 0; k < 3; k++) { off[k] = at; at += (need[k] + 255) & ~uint64_t(255); }
    off[3] = at;
    return at + (img->kind == J2K_IMG_PALETTED ? 3 * (size_t)img->npal : 0);
}
int image_upload(j2k_ctx *ctx, const j2k_image *img, const uint64_t need[3], uint8_t *dev, const size_t off[4], j2k_image *d_img) {
    *d_img = *img;
    for (int k = 0; k < 3; k++) {
        d_img->plane[k] = need[k] ? dev + off[k] : nullptr;
        if (need[k]) HIPCHK(ctx, hipMemcpyAsync(dev + off[k], img->plane[k], need[k], hipMemcpyHostToDevice, ctx->stream));
    }
    d_img->palette = img->kind == J2K_IMG_PALETTED && img->npal ? dev + off[3] : nullptr;
    if (d_img->palette) HIPCHK(ctx, hipMemcpyAsync(dev + off[3], img->palette, 3 * (size_t)img->npal, hipMemcpyHostToDevice, ctx->stream));
    return J2K_OK;
}

extern "C" int j2k_extract_image_planar(j2k_ctx *ctx, const j2k_image *img, int target_precision, int32_t *const *planes) {
    if (!ctx || !img || !planes || target_precision < 0 || target_precision > 16) return J2K_ERR_INVALID_ARG;
    int r = image_check(ctx, img, -1, -1);
    if (r != J2K_OK) return r;
    const int w = img->width, h = img->height;
    const size_t n = (size_t)w * h;
    if (!n) return J2K_OK;
    uint64_t need[3];
    image_device_bytes(img, need);
    size_t off[4];
    const size_t img_bytes = (image_layout(img, need, off) + 255) & ~size_t(255), rgba_at = img_bytes, flag_at = rgba_at + ((n * 4 + 255) & ~size_t(255));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    r = stage_reserve(ctx, 0, flag_at + 64);                    // the planes cross PCIe at their native sizes
    if (r == J2K_OK) r = stage_reserve(ctx, 1, n * 4 * 3 + 64);
    if (r != J2K_OK) return r;
    uint8_t *dev = (uint8_t *)ctx->stage[0];
    j2k_image d_img;
    if ((r = image_upload(ctx, img, need, dev, off, &d_img)) != J2K_OK) return r;
    if ((r = convert_rgba8(ctx, &d_img, (uint32_t *)(dev + rgba_at), (size_t)w, nullptr, (int *)(dev + flag_at))) != J2K_OK) return r;
    r = j2k_unpack_pixels(ctx, J2K_PIX_RGBA8, dev + rgba_at, (size_t)w * 4, w, h, target_precision, (int32_t *)ctx->stage[1]);
    if (r != J2K_OK) return r;
    for (int c = 0; c < 3; c++)
        HIPCHK(ctx, hipMemcpyAsync(planes[c], (int32_t *)ctx->stage[1] + (size_t)c * n, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return J2K_OK;
}

// The fused source: a YCbCr 4:4:4 / 4:2:2 / 4:2:0 image at an even, non-negative Rect.Min (Go's offsets are then shifts of the frame
// position) on a plan whose RGBA8 frames take the level-0 workgroup kernel alone, with the planes aligned for its loads: the Y plane
// 16 bytes (it stands in for the frame pointer), 8 Y bytes per lane (ystride % 8), 8 or 4 chroma bytes per lane, one chroma stride.
static bool image_fusable(const j2k_plan *P, const j2k_image *img, YccSrc *src) {
    if (img->kind != J2K_IMG_YCBCR || img->ratio > J2K_YCBCR_420 || (img->min_x & 1) || (img->min_y & 1) || img->min_x < 0 || img->min_y < 0) return false;
    if (img->width != P->spec.W || img->height != P->spec.H || !plan_rgba8_wg_fusable(P)) return false;
    const uintptr_t ca = img->ratio == J2K_YCBCR_444 ? 7 : 3;
    if (((uintptr_t)img->plane[0] & 15) || (img->stride[0] & 7) || img->stride[1] != img->stride[2]) return false;
    if (((uintptr_t)img->plane[1] | (uintptr_t)img->plane[2] | (uintptr_t)img->stride[1]) & ca) return false;
    if (src) *src = YccSrc{img->plane[0], img->plane[1], img->plane[2], img->stride[0], img->stride[1], img->ratio, 0};
    return true;
}

extern "C" int j2k_plan_image_fused(const j2k_plan *P, const j2k_image *d_img) {
    if (!P || !d_img) return J2K_ERR_INVALID_ARG;
    if (j2k_image_validate(d_img, P->spec.W, P->spec.H) == J2K_ERR_INVALID_ARG) return J2K_ERR_INVALID_ARG;
    return image_fusable(P, d_img, nullptr) ? 1 : 0;
}

int plan_forward_image_impl(j2k_plan *P, const j2k_image *d_img, int32_t *d_coeff, int *status_word) {
    j2k_ctx *ctx = P->ctx;
    const PlanSpec &S = P->spec;
    if (S.C != 3) return fail(ctx, J2K_ERR_INVALID_ARG, "an image.YCbCr / CMYK / Paletted is 3 components (encoder.go:178-195): the plan has another count");
    int r = image_check(ctx, d_img, S.W, S.H);
    if (r != J2K_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PixIO io;
    if (image_fusable(P, d_img, &io.ycc)) {
        io.stride = S.W;                  // (the pixel stride of the RGBA8 frame it replaces: the launch path wants one)
        io.triple = 8;
        return plan_forward_impl(P, d_img->plane[0], d_coeff, io);
    }
    const size_t fb = ((size_t)S.W * S.H * 4 + 255) & ~size_t(255);
    if ((r = stage_reserve(ctx, 1, fb + 64)) != J2K_OK) return r;        // the RGBA8 frame (forward_pixels stages in slot 0)
    uint8_t *rgba = (uint8_t *)ctx->stage[1];
    if ((r = convert_rgba8(ctx, d_img, (uint32_t *)rgba, (size_t)S.W, status_word, (int *)(rgba + fb))) != J2K_OK) return r;
    return j2k_plan_forward_pixels(P, J2K_PIX_RGBA8, rgba, (size_t)S.W * 4, d_coeff);
}

extern "C" int j2k_plan_forward_image(j2k_plan *P, const j2k_image *d_img, int32_t *d_coeff) {
    graph_note_plan(P);
    if (!P || !d_img || !d_coeff) return J2K_ERR_INVALID_ARG;
    return plan_forward_image_impl(P, d_img, d_coeff, nullptr);
}
