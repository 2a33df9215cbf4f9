// image.hip -- the default branch of encoder.extractImageData (encoder.go:178-195) for *image.YCbCr, *image.CMYK and
// *image.Paletted: every pixel's r>>8, g>>8, b>>8 of At(x, y).RGBA() into a packed RGBA8 frame (alpha 255), which the
// J2K_PIX_RGBA8 calls then take as they are -- the default branch makes 3 components at precision 8, like image.RGBA.
// Colours: image_color.h.  Offsets as image.YCbCr.YOffset / COffset and image.CMYK / Paletted.PixOffset, with Go's
// truncating `/` (C++'s): Rect.Min may be odd or negative.  The host has checked every offset against the planes' lengths.
#include "j2k_internal.h"

namespace j2k {

__global__ __launch_bounds__(256) void image_to_rgba8_kernel(const j2k_image img, uint32_t *__restrict__ pix, size_t stride_px,
                                                             int *__restrict__ flag) {
    const int w = img.width, h = img.height;
    const size_t n = (size_t)w * h;
    const int hd = ycc_hdiv(img.ratio), vd = ycc_vdiv(img.ratio);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int dy = (int)(i / (size_t)w), dx = (int)(i - (size_t)dy * w);
        uint32_t v;
        if (img.kind == J2K_IMG_YCBCR) {
            const int x = img.min_x + dx, y = img.min_y + dy;
            const int64_t yi = (int64_t)dy * img.stride[0] + dx;
            const int64_t cx = x / hd - img.min_x / hd, cy = y / vd - img.min_y / vd;
            v = ycbcr_rgba8(img.plane[0][yi], img.plane[1][cy * img.stride[1] + cx], img.plane[2][cy * img.stride[2] + cx]);
        } else if (img.kind == J2K_IMG_CMYK) {
            const uint8_t *p = img.plane[0] + (int64_t)dy * img.stride[0] + 4 * (int64_t)dx;
            v = cmyk_rgba8(p[0], p[1], p[2], p[3]);
        } else {
            const int k = img.plane[0][(int64_t)dy * img.stride[0] + dx];
            if (k >= img.npal) {          // Go: index out of range
                *flag = J2K_ERR_GO_PANIC;
                v = 0xFF000000u;
            } else {
                const uint8_t *e = img.palette + 3 * k;
                v = (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | 0xFF000000u;
            }
        }
        pix[(size_t)dy * stride_px + dx] = v;
    }
}

hipError_t launch_image_to_rgba8(hipStream_t s, const j2k_image &img, uint32_t *pix, size_t stride_px, int *flag) {
    const size_t n = (size_t)img.width * img.height;
    if (!n) return hipSuccess;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 65536);
    hipLaunchKernelGGL(image_to_rgba8_kernel, dim3(blocks), dim3(256), 0, s, img, pix, stride_px, flag);
    return hipGetLastError();
}

}  // namespace j2k
