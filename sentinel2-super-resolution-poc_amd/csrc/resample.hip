// Resampled tile levels: a separable filter given as tap tables, two passes, integer arithmetic only.
// The kernels know no filter: Lanczos, cubic and bilinear differ in the tables the host builds (s2sr/tiles.py
// plan_resample_axis).  Per axis and output sample j: first[j] (source index of tap 0), count[j] (taps, 0 = the sample misses
// the source) and coef[t][j] (22 fractional bits, [K][n_out]: neighbouring samples read neighbouring words).  The arithmetic
// is Pillow's Image.resize for RGBA:
//   resample_h : source pixel -> premultiplied (c' = ((m >> 8) + m) >> 8, m = c * a + 128) -> per channel
//                clip((2^21 + sum coef * px) >> 22) -> intermediate [rows][nx*256] RGBA u8, only the source rows the vertical tables
//                read.  The source is a row-major raster or a tile-major level (template flag).
//   resample_v : the same sum down the intermediate's columns -> un-premultiplied (alpha 0 / 255: copy, else
//                min(255, 255 * c' / a)) -> out[ty][tx][py][px], the layout of tiles_base_kernel.
// Every index comes from tables the entry (engine_tiles.hip, resample_tables.h) has range-checked against the buffers, and
// 255 * sum|coef| + 2^21 < 2^31 per sample: int32 accumulators cannot wrap.
#include "s2sr_internal.h"

namespace s2sr {

namespace {

__device__ __forceinline__ int clip8(int acc) { return min(max((acc + (1 << 21)) >> 22, 0), 255); }

template <bool LEVEL>
__global__ void __launch_bounds__(256) resample_h_kernel(const uint8_t* __restrict__ src, int sb, const int32_t* __restrict__ first,
                                                         const int32_t* __restrict__ count, const int32_t* __restrict__ coef, int MW,
                                                         int r0, int nrows, uint8_t* __restrict__ inter) {
    const size_t total = (size_t)MW * nrows;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int gx = (int)(i % MW), r = r0 + (int)(i / MW);
        const int c0 = first[gx], n = count[gx];
        // LEVEL: row r of the child mosaic lives in tile row r >> 8, and a tap's column picks the tile inside it
        const uchar4* row = LEVEL ? (const uchar4*)src + ((size_t)(r >> 8) * sb * 256 + (r & 255)) * 256 : (const uchar4*)src + (size_t)r * sb;
        int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        for (int t = 0; t < n; ++t) {
            const int c = c0 + t;
            const uchar4 p = LEVEL ? row[(size_t)(c >> 8) * 65536 + (c & 255)] : row[c];
            const int k = coef[(size_t)t * MW + gx];
            const int a = p.w;
            const int m0 = p.x * a + 128, m1 = p.y * a + 128, m2 = p.z * a + 128;
            s0 += k * (((m0 >> 8) + m0) >> 8);
            s1 += k * (((m1 >> 8) + m1) >> 8);
            s2 += k * (((m2 >> 8) + m2) >> 8);
            s3 += k * a;
        }
        ((uchar4*)inter)[i] = make_uchar4((uint8_t)clip8(s0), (uint8_t)clip8(s1), (uint8_t)clip8(s2), (uint8_t)clip8(s3));
    }
}

__global__ void __launch_bounds__(256) resample_v_kernel(const uint8_t* __restrict__ inter, int r0, const int32_t* __restrict__ first,
                                                         const int32_t* __restrict__ count, const int32_t* __restrict__ coef, int nx,
                                                         int ny, uint8_t* __restrict__ out) {
    const int MW = nx * 256, MH = ny * 256;
    const size_t total = (size_t)MW * MH;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int gx = (int)(i % MW), gy = (int)(i / MW);
        const int n = count[gy];
        const uchar4* col = (const uchar4*)inter + (n ? (size_t)(first[gy] - r0) * MW + gx : 0);      // (a row with taps starts at or below r0)
        int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        for (int t = 0; t < n; ++t) {
            const uchar4 p = col[(size_t)t * MW];
            const int k = coef[(size_t)t * MH + gy];
            s0 += k * p.x; s1 += k * p.y; s2 += k * p.z; s3 += k * p.w;
        }
        int c0 = clip8(s0), c1 = clip8(s1), c2 = clip8(s2);
        const int a = clip8(s3);
        if (a != 0 && a != 255) { c0 = min(255, 255 * c0 / a); c1 = min(255, 255 * c1 / a); c2 = min(255, 255 * c2 / a); }
        ((uchar4*)out)[(((size_t)(gy >> 8) * nx + (gx >> 8)) * 256 + (gy & 255)) * 256 + (gx & 255)] =
            make_uchar4((uint8_t)c0, (uint8_t)c1, (uint8_t)c2, (uint8_t)a);
    }
}

inline int grid_for(size_t total) { return stride_grid(total, 16384, GF_RESAMPLE); }   // under the diagnostic grid cap (s2sr_internal.h)

}  // namespace

hipError_t launch_resample_h(const uint8_t* d_src, bool level, int sb, const int32_t* d_first, const int32_t* d_count,
                             const int32_t* d_coef, int nx, int r0, int nrows, uint8_t* d_inter, hipStream_t st) {
    if (nrows <= 0) return hipSuccess;          // no output row reads the source: the vertical pass writes a transparent level
    const int MW = nx * 256;
    const dim3 grid(grid_for((size_t)MW * nrows));
    if (level)
        hipLaunchKernelGGL(resample_h_kernel<true>, grid, dim3(256), 0, st, d_src, sb, d_first, d_count, d_coef, MW, r0, nrows, d_inter);
    else
        hipLaunchKernelGGL(resample_h_kernel<false>, grid, dim3(256), 0, st, d_src, sb, d_first, d_count, d_coef, MW, r0, nrows, d_inter);
    return hipGetLastError();
}

hipError_t launch_resample_v(const uint8_t* d_inter, int r0, const int32_t* d_first, const int32_t* d_count, const int32_t* d_coef,
                             int nx, int ny, uint8_t* d_out, hipStream_t st) {
    hipLaunchKernelGGL(resample_v_kernel, dim3(grid_for((size_t)nx * ny * 65536)), dim3(256), 0, st, d_inter, r0, d_first, d_count,
                       d_coef, nx, ny, d_out);
    return hipGetLastError();
}

}  // namespace s2sr
