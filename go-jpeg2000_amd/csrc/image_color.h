// image_color.h -- the colours of the default branch of encoder.extractImageData (encoder.go:178-195) for the image types Go's
// decoders return: r>>8, g>>8, b>>8 of img.At(x, y).RGBA() (image/color, Go >= 1.8), restated in int32 / uint32 arithmetic
// (every product fits).  Shared by image.hip (the staged conversion) and the fused 5-3 level-0 kernel (dwt53_l0pix_fwd_body.inc).
#pragma once
#include <stdint.h>

namespace j2k {

// color.YCbCr.RGBA() takes each of r, g, b to v >> 8 clamped to [0, 0xFFFF] (0 below, 0xFFFF above 0xFFFFFF); the default branch
// takes >> 8 once more: clamp(v, 0, 0xFFFFFF) >> 16.  Note Y * 0x10100, not YCbCrToRGB's 0x10101.
__host__ __device__ __forceinline__ int ycc_clamp16(int v) { return (v < 0 ? 0 : (v > 0xFFFFFF ? 0xFFFFFF : v)) >> 16; }
__host__ __device__ __forceinline__ uint32_t ycbcr_rgba8(int Y, int Cb, int Cr) {
    const int yy = Y * 0x10100, cb = Cb - 128, cr = Cr - 128;
    const int r = ycc_clamp16(yy + 91881 * cr), g = ycc_clamp16(yy - 22554 * cb - 46802 * cr), b = ycc_clamp16(yy + 116130 * cb);
    return (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16 | 0xFF000000u;
}
// color.CMYK.RGBA(): w = 0xFFFF - K * 0x101, r = (0xFFFF - C * 0x101) * w / 0xFFFF in uint32, then >> 8
__host__ __device__ __forceinline__ uint32_t cmyk_rgba8(uint32_t C, uint32_t M, uint32_t Yc, uint32_t K) {
    const uint32_t w = 0xFFFFu - K * 0x101u;
    const uint32_t r = (0xFFFFu - C * 0x101u) * w / 0xFFFFu, g = (0xFFFFu - M * 0x101u) * w / 0xFFFFu, b = (0xFFFFu - Yc * 0x101u) * w / 0xFFFFu;
    return (r >> 8) | (g >> 8) << 8 | (b >> 8) << 16 | 0xFF000000u;
}
// image.YCbCr chroma subsampling of a ratio (J2K_YCBCR_*): horizontal / vertical divisor
__host__ __device__ __forceinline__ int ycc_hdiv(int ratio) { return (ratio == 4 || ratio == 5) ? 4 : ((ratio == 1 || ratio == 2) ? 2 : 1); }
__host__ __device__ __forceinline__ int ycc_vdiv(int ratio) { return (ratio == 2 || ratio == 3 || ratio == 5) ? 2 : 1; }

}  // namespace j2k
