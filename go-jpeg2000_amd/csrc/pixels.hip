// pixels.hip -- pixel unpack / pack at native width: the host loops on either side of the
// tile-component path.
//
// Replaces (reference, mrjoshuak/go-jpeg2000):
//   encoder.extractImageData   encoder.go:79-213   image.Gray / Gray16 / RGBA / RGBA64 / NRGBA / NRGBA64 -> planar
//                                                  int32 components (+ the Options.Precision rescale, :196-210)
//   decoder.createImage        decoder.go:417-588  planar int32 -> image.Gray / Gray16 / RGBA / RGBA64 (clamp, rescale)
//
// The byte layouts are Go's image package: Pix is row-major with `stride` bytes per row; 16-bit samples are
// big-endian; RGBA = R,G,B,A bytes.  Arithmetic is Go int32: the rescale multiplies wrap (65535 * 65535 overflows)
// and `/` truncates toward zero, exactly as written in the reference.
#include "j2k_internal.h"

namespace j2k {

__device__ __forceinline__ int be16(const uint8_t *p) { return (int)p[0] << 8 | (int)p[1]; }
__device__ __forceinline__ int go_muldiv(int v, int a, int b) { return (int)((uint32_t)v * (uint32_t)a) / b; }   // int32 wrap, trunc

__global__ __launch_bounds__(256) void unpack_pixels_kernel(const uint8_t *__restrict__ pix, size_t stride, int format, int w, int h,
                                                            int src_max, int dst_max, int32_t *__restrict__ planes) {
    const size_t n = (size_t)w * h;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / (size_t)w), x = (int)(i - (size_t)y * w);
        const uint8_t *row = pix + (size_t)y * stride;
        int v[4] = {0, 0, 0, 0};
        int nc = 1;
        switch (format) {
        case J2K_PIX_GRAY8: v[0] = row[x]; break;
        case J2K_PIX_GRAY16: v[0] = be16(row + 2 * (size_t)x); break;
        case J2K_PIX_RGBA8: {        // alpha ignored (encoder.go:107)
            const uint32_t p = *reinterpret_cast<const uint32_t *>(row + 4 * (size_t)x);   // Pix rows of image.RGBA are 4-byte aligned when stride % 4 == 0
            v[0] = p & 0xFF; v[1] = (p >> 8) & 0xFF; v[2] = (p >> 16) & 0xFF; nc = 3;
            break;
        }
        case J2K_PIX_NRGBA8: {
            const uint32_t p = *reinterpret_cast<const uint32_t *>(row + 4 * (size_t)x);
            v[0] = p & 0xFF; v[1] = (p >> 8) & 0xFF; v[2] = (p >> 16) & 0xFF; v[3] = p >> 24; nc = 4;
            break;
        }
        case J2K_PIX_RGBA64: {
            const uint8_t *q = row + 8 * (size_t)x;
            v[0] = be16(q); v[1] = be16(q + 2); v[2] = be16(q + 4); nc = 3;
            break;
        }
        default: {                   // J2K_PIX_NRGBA64
            const uint8_t *q = row + 8 * (size_t)x;
            v[0] = be16(q); v[1] = be16(q + 2); v[2] = be16(q + 4); v[3] = be16(q + 6); nc = 4;
            break;
        }
        }
        for (int c = 0; c < nc; c++) {
            int t = v[c];
            if (dst_max != src_max) t = go_muldiv(t, dst_max, src_max);       // encoder.go:196-210
            planes[(size_t)c * n + i] = t;
        }
    }
}

// decoder.createImage: ncomp 1 -> Gray (precision <= 8) or Gray16; 3 / 4 -> RGBA (precision <= 8) or RGBA64.  The rectangle (x0, y0, rw, rh) of
// w x h planes: the whole frame, or the rows of tiles that a shard's inverse transform wrote
__global__ __launch_bounds__(256) void pack_pixels_kernel(const int32_t *__restrict__ planes, int ncomp, int precision, int w, int h, int x0, int y0, int rw,
                                                          int rh, uint8_t *__restrict__ pix, size_t stride, const int *__restrict__ guard) {
    if (guard && *guard) return;             // (the frame decoder: a stream that was refused leaves the caller's frame alone)
    const size_t n = (size_t)w * h, m = (size_t)rw * rh;
    const int max_val = (int)((1u << precision) - 1);
    const bool wide = precision > 8;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < m; j += (size_t)gridDim.x * 256) {
        const int yy = (int)(j / (size_t)rw), y = y0 + yy, x = x0 + (int)(j - (size_t)yy * rw);
        const size_t i = (size_t)y * w + x;
        uint8_t *row = pix + (size_t)y * stride;
        int v[4];
        for (int c = 0; c < ncomp; c++) {
            int t = planes[(size_t)c * n + i];
            t = t < 0 ? 0 : (t > max_val ? max_val : t);
            if (wide) t = go_muldiv(t, 65535, max_val);
            else if (precision != 8) t = go_muldiv(t, 255, max_val);
            v[c] = t;
        }
        if (ncomp == 1) {
            if (wide) { row[2 * (size_t)x] = (uint8_t)((uint32_t)v[0] >> 8); row[2 * (size_t)x + 1] = (uint8_t)v[0]; }   // uint16(v), big-endian
            else row[x] = (uint8_t)v[0];
        } else {
            const int a = ncomp == 4 ? v[3] : (wide ? 65535 : 255);
            if (wide) {
                uint8_t *q = row + 8 * (size_t)x;
                const int o[4] = {v[0], v[1], v[2], a};
                for (int c = 0; c < 4; c++) { q[2 * c] = (uint8_t)((uint32_t)o[c] >> 8); q[2 * c + 1] = (uint8_t)o[c]; }
            } else {
                *reinterpret_cast<uint32_t *>(row + 4 * (size_t)x) =
                    ((uint32_t)v[0] & 0xFF) | ((uint32_t)v[1] & 0xFF) << 8 | ((uint32_t)v[2] & 0xFF) << 16 | ((uint32_t)a & 0xFF) << 24;
            }
        }
    }
}

// pack_pixels_kernel for a region decode: the rectangle (x0, y0, rw, rh) of the w x h planes into a pix that holds that rectangle ALONE, at
// origin (0, 0) -- rh rows of rw pixels.  A kernel of its own, so that pack_pixels_kernel stays the code it was.
__global__ __launch_bounds__(256) void pack_pixels_window_kernel(const int32_t *__restrict__ planes, int ncomp, int precision, int w, int h, int x0, int y0, int rw,
                                                                 int rh, uint8_t *__restrict__ pix, size_t stride, const int *__restrict__ guard) {
    if (guard && *guard) return;             // (a stream that was refused leaves the caller's buffer alone)
    const size_t n = (size_t)w * h, m = (size_t)rw * rh;
    const int max_val = (int)((1u << precision) - 1);
    const bool wide = precision > 8;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < m; j += (size_t)gridDim.x * 256) {
        const int y = (int)(j / (size_t)rw), x = (int)(j - (size_t)y * rw);          // in the rectangle = in pix
        const size_t i = (size_t)(y0 + y) * w + x0 + x;
        uint8_t *row = pix + (size_t)y * stride;
        int v[4];
        for (int c = 0; c < ncomp; c++) {
            int t = planes[(size_t)c * n + i];
            t = t < 0 ? 0 : (t > max_val ? max_val : t);
            if (wide) t = go_muldiv(t, 65535, max_val);
            else if (precision != 8) t = go_muldiv(t, 255, max_val);
            v[c] = t;
        }
        if (ncomp == 1) {
            if (wide) { row[2 * (size_t)x] = (uint8_t)((uint32_t)v[0] >> 8); row[2 * (size_t)x + 1] = (uint8_t)v[0]; }
            else row[x] = (uint8_t)v[0];
        } else {
            const int a = ncomp == 4 ? v[3] : (wide ? 65535 : 255);
            if (wide) {
                uint8_t *q = row + 8 * (size_t)x;
                const int o[4] = {v[0], v[1], v[2], a};
                for (int c = 0; c < 4; c++) { q[2 * c] = (uint8_t)((uint32_t)o[c] >> 8); q[2 * c + 1] = (uint8_t)o[c]; }
            } else {
                *reinterpret_cast<uint32_t *>(row + 4 * (size_t)x) =
                    ((uint32_t)v[0] & 0xFF) | ((uint32_t)v[1] & 0xFF) << 8 | ((uint32_t)v[2] & 0xFF) << 16 | ((uint32_t)a & 0xFF) << 24;
            }
        }
    }
}

// ---- sum of squared sample differences of two frames in the same Pix layout, per channel as stored (alpha included) -------------------------
// One streaming pass: a row is cut into pieces of 16 bytes, 64 consecutive pieces are one item, and the wavefronts of the grid stride over the
// items (row, chunk).  A piece never splits a pixel's channels apart from their place: 16 is a multiple of every pixel size, so byte i of a piece
// (8-bit samples) or sample i (16-bit, big-endian) belongs to channel i % channels.  Rows whose two pointers are 16-byte aligned take one
// 16-byte load per frame and piece; any other row, and the ragged piece at a row's end, is read byte by byte (bytes past the row count as
// equal).  Every wavefront leaves 4 partial sums; sse_reduce_kernel adds them.  Integer sums, exact in uint64: no order to define, no atomics.
#define SSE_MAX_WAVES 1024
union SsePiece { uint4 v; uint8_t b[16]; };
__global__ __launch_bounds__(256) void sse_partial_kernel(const uint8_t *__restrict__ a, size_t stride_a, const uint8_t *__restrict__ b, size_t stride_b,
                                                          size_t rowbytes, int h, int wide, int nch, uint64_t *__restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (size_t)gridDim.x * 4;
    const size_t chunks = (rowbytes + 1023) / 1024, items = chunks * (size_t)h;
    uint64_t acc[4] = {0, 0, 0, 0};
    for (size_t it = wave; it < items; it += nwaves) {
        const size_t y = it / chunks, off = (it - y * chunks) * 1024 + (size_t)lane * 16;
        if (off >= rowbytes) continue;
        const uint8_t *pa = a + y * stride_a + off, *pb = b + y * stride_b + off;
        const int nbytes = (int)(rowbytes - off < 16 ? rowbytes - off : 16);
        SsePiece A, B;
        if (nbytes == 16 && ((((uintptr_t)pa) | ((uintptr_t)pb)) & 15) == 0) {
            A.v = *reinterpret_cast<const uint4 *>(pa);
            B.v = *reinterpret_cast<const uint4 *>(pb);
        } else {
            A.v = make_uint4(0, 0, 0, 0); B.v = A.v;
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (i < nbytes) { A.b[i] = pa[i]; B.b[i] = pb[i]; }
        }
        if (wide) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int d = be16(A.b + 2 * i) - be16(B.b + 2 * i);
                acc[i & 3] += (uint64_t)((uint32_t)(d < 0 ? -d : d) * (uint32_t)(d < 0 ? -d : d));       // 65535^2 < 2^32
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int d = (int)A.b[i] - (int)B.b[i];
                acc[i & 3] += (uint64_t)(uint32_t)(d * d);
            }
        }
    }
    if (nch == 1) { acc[0] += acc[1] + acc[2] + acc[3]; acc[1] = acc[2] = acc[3] = 0; }     // one channel: the four phases are the same one
#pragma unroll
    for (int c = 0; c < 4; c++) {
        uint64_t s = acc[c];
        for (int o = 32; o > 0; o >>= 1) s += (uint64_t)__shfl_xor((unsigned long long)s, o);
        if (lane == 0) partial[wave * 4 + c] = s;
    }
}
// one workgroup of 4 wavefronts: wavefront c adds channel c's partial sums
__global__ __launch_bounds__(256) void sse_reduce_kernel(const uint64_t *__restrict__ partial, int nwaves, int nch, uint64_t *__restrict__ sums) {
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
    uint64_t s = 0;
    for (int i = lane; i < nwaves; i += 64) s += partial[(size_t)i * 4 + c];
    for (int o = 32; o > 0; o >>= 1) s += (uint64_t)__shfl_xor((unsigned long long)s, o);
    if (lane == 0 && c < nch) sums[c] = s;
}

size_t pixels_sse_workspace() { return (size_t)SSE_MAX_WAVES * 4 * sizeof(uint64_t); }
// channels: 1 or 4 as stored; partial: pixels_sse_workspace() bytes; sums: `channels` words, always written
hipError_t launch_pixels_sse(hipStream_t s, const uint8_t *a, size_t stride_a, const uint8_t *b, size_t stride_b, size_t rowbytes, int h, bool wide, int channels,
                             uint64_t *partial, uint64_t *sums) {
    if (channels != 1 && channels != 4) return hipErrorInvalidValue;
    const size_t items = ((rowbytes + 1023) / 1024) * (size_t)(h > 0 ? h : 0);
    const int blocks = (int)std::max<size_t>(1, std::min<size_t>((items + 3) / 4, SSE_MAX_WAVES / 4));
    hipLaunchKernelGGL(sse_partial_kernel, dim3(blocks), dim3(256), 0, s, a, stride_a, b, stride_b, rowbytes, h > 0 ? h : 0, wide ? 1 : 0, channels, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sse_reduce_kernel, dim3(1), dim3(256), 0, s, partial, blocks * 4, channels, sums);
    return hipGetLastError();
}

hipError_t launch_unpack_pixels(hipStream_t s, const uint8_t *pix, size_t stride, int format, int w, int h, int src_max, int dst_max,
                                int32_t *planes) {
    const size_t n = (size_t)w * h;
    if (!n) return hipSuccess;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 65536);
    hipLaunchKernelGGL(unpack_pixels_kernel, dim3(blocks), dim3(256), 0, s, pix, stride, format, w, h, src_max, dst_max, planes);
    return hipGetLastError();
}

hipError_t launch_pack_pixels_rect(hipStream_t s, const int32_t *planes, int ncomp, int precision, int w, int h, int x0, int y0, int rw, int rh, uint8_t *pix,
                                   size_t stride, const int *guard) {
    if (x0 < 0 || y0 < 0 || rw < 0 || rh < 0 || x0 + rw > w || y0 + rh > h) return hipErrorInvalidValue;
    const size_t m = (size_t)rw * rh;
    if (!m) return hipSuccess;
    const int blocks = (int)std::min<size_t>((m + 255) / 256, 65536);
    hipLaunchKernelGGL(pack_pixels_kernel, dim3(blocks), dim3(256), 0, s, planes, ncomp, precision, w, h, x0, y0, rw, rh, pix, stride, guard);
    return hipGetLastError();
}
hipError_t launch_pack_pixels_window(hipStream_t s, const int32_t *planes, int ncomp, int precision, int w, int h, int x0, int y0, int rw, int rh, uint8_t *pix,
                                     size_t stride, const int *guard) {
    if (x0 < 0 || y0 < 0 || rw < 0 || rh < 0 || x0 + rw > w || y0 + rh > h) return hipErrorInvalidValue;
    const size_t m = (size_t)rw * rh;
    if (!m) return hipSuccess;
    const int blocks = (int)std::min<size_t>((m + 255) / 256, 65536);
    hipLaunchKernelGGL(pack_pixels_window_kernel, dim3(blocks), dim3(256), 0, s, planes, ncomp, precision, w, h, x0, y0, rw, rh, pix, stride, guard);
    return hipGetLastError();
}
hipError_t launch_pack_pixels(hipStream_t s, const int32_t *planes, int ncomp, int precision, int w, int h, uint8_t *pix, size_t stride) {
    return launch_pack_pixels_rect(s, planes, ncomp, precision, w, h, 0, 0, w, h, pix, stride);
}

}  // namespace j2k
