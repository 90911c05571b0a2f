// Nodata-aware enhance: the two kernels around the net that keep pixels which were never measured out of its
// way.  The FILL runs in front of the net and gives every invalid pixel the samples of its nearest valid neighbour, so that the
// net sees extrapolated ground instead of a full-contrast step; the MASK runs behind everything else and writes the nodata
// value back over the output pixels of every invalid input pixel.
//
// Definition (integers throughout):
//   image     [H, W, 3] interleaved, uint8 or uint16.  valid: uint8 [H, W], nonzero = valid.  radius R: 1..64.
//   fill      a valid pixel is unchanged.  An invalid pixel p = (y, x) takes all three samples of the valid pixel q = (qy, qx)
//             that minimises the key (d2, qy, qx) lexicographically, d2 = (qy - y)^2 + (qx - x)^2, over all valid q with
//             d2 <= R^2.  No such q: p keeps its samples.  The image edge is not replicated: there are no candidates outside.
//   separable per column c, d1(y, c) = the signed offset in [-R, R] to the vertically nearest valid pixel of column c (a tie goes
//             to the pixel above; NONE if there is none).  The answer for p is the minimum over c in [x - R, x + R] and [0, W)
//             of ((c - x)^2 + d1(y, c)^2, y + d1(y, c), c), subject to the first term being <= R^2: inside a column only the
//             vertically nearest pixel can win (any other has a larger d2), and the tie to the pixel above is the key's qy.
//   mask      output pixel (Y, X) at scale s is invalid iff input pixel (Y / s, X / s) is invalid; an invalid output pixel gets
//             out_nodata in all three samples, a valid one is not touched (it may happen to equal out_nodata: the mask is the
//             truth, the value only the file convention).
//
// Fill kernel.  In place on the uploaded image: only valid pixels are read as sources and only invalid ones are written, so no
// workgroup reads what another writes.  A workgroup of 256 threads owns a tile of 16 rows x 256 columns, thread t column t.  It
// reads the tile's own valid bytes first and goes on to the next tile if none is invalid; then it stages the valid bytes of the
// tile plus an R halo in LDS ((16 + 2R) x (256 + 2R) bytes, 0 outside the image; R = 64: 54 KB) and goes on if none is valid;
// then d1 of its 16 rows over the 256 + 2R staged columns (int8, 6 KB); then every invalid pixel takes the minimum over at most
// 2R + 1 packed keys  d2 << 16 | (dy + R) << 8 | (dx + R)  -- for fixed (y, x) ordered exactly as (d2, qy, qx) -- and copies its
// source's three samples.  A mostly valid or mostly empty raster costs about one read of the mask.
//
// Mask kernel.  One thread per input pixel of the band of output rows [yb, ye): an invalid one stores out_nodata into its s x s
// output pixels, per output row three words of s samples each (x4: 3 x 4 B for uint8, 3 x 8 B for uint16; x2: 3 x 2 B, 3 x 4 B).
// It reads nothing of the image and writes only where the pixel is invalid.
//
// Both kernels run grid-stride loops with 64-bit offsets, and take every index from sizes the launchers have checked.
#include "s2sr_internal.h"

namespace s2sr {

namespace {

constexpr int kFillRows = 16, kFillCols = 256, kFillThreads = 256, kMaxRadius = 64;
constexpr int kNone = -128;                         // d1: no valid pixel within R in this column

static_assert(kFillCols == kFillThreads, "thread t owns column t of the tile");

template <class T>
__global__ void __launch_bounds__(kFillThreads) nodata_fill_kernel(T* __restrict__ img, const uint8_t* __restrict__ valid, int H, int W, int R,
                                                                   int tiles_x, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fill_lds[];
    const int SW = kFillCols + 2 * R, SH = kFillRows + 2 * R;
    uint8_t* vs = fill_lds;                                          // [SH][SW]: valid, row y0 - R + sr, column x0 - R + sc
    int8_t* d1 = (int8_t*)(fill_lds + ((SH * SW + 15) & ~15));       // [kFillRows][SW]
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {           // (t is uniform over the workgroup: so is every barrier below)
        const int y0 = (t / tiles_x) * kFillRows, x0 = (t % tiles_x) * kFillCols;
        const int x = x0 + tid;
        // the tile's own pixels: nothing invalid, nothing to do.  (The barrier also ends the tile before's reads of vs and d1.)
        int invalid = 0;
        if (x < W)
            for (int r = 0; r < kFillRows && y0 + r < H; ++r) invalid |= valid[(size_t)(y0 + r) * W + x] == 0;
        if (!__syncthreads_or(invalid)) continue;
        int any = 0;
        for (int i = tid; i < SH * SW; i += kFillThreads) {
            const int sr = i / SW, sc = i - sr * SW;
            const int y = y0 - R + sr, c = x0 - R + sc;
            uint8_t v = 0;
            if (y >= 0 && y < H && c >= 0 && c < W) v = valid[(size_t)y * W + c] != 0;
            vs[i] = v;
            any |= v;
        }
        if (!__syncthreads_or(any)) continue;                        // no source within reach of any pixel of the tile
        for (int i = tid; i < kFillRows * SW; i += kFillThreads) {
            const int r = i / SW, sc = i - r * SW;
            int d = kNone;
            for (int k = 0; k <= R; ++k) {                           // staged rows R + r - k >= 0 and R + r + k < SH
                if (vs[(R + r - k) * SW + sc]) { d = -k; break; }    // the pixel above first: the tie
                if (vs[(R + r + k) * SW + sc]) { d = k; break; }
            }
            d1[i] = (int8_t)d;
        }
        __syncthreads();
        if (x >= W) continue;                                        // (no barrier follows in this iteration)
        const int dx_lo = x < R ? -x : -R, dx_hi = W - 1 - x < R ? W - 1 - x : R;
        for (int r = 0; r < kFillRows && y0 + r < H; ++r) {
            if (vs[(R + r) * SW + R + tid]) continue;
            const int8_t* row = d1 + r * SW + R + tid;               // row[dx], dx in [-R, R]: staged columns tid .. tid + 2R < SW
            uint32_t best = 0xffffffffu;
            for (int dx = dx_lo; dx <= dx_hi; ++dx) {
                const int d = row[dx];
                const uint32_t cost = (uint32_t)(dx * dx + d * d);
                if (d != kNone && cost <= (uint32_t)(R * R)) {
                    const uint32_t key = cost << 16 | (uint32_t)(d + R) << 8 | (uint32_t)(dx + R);
                    best = key < best ? key : best;
                }
            }
            if (best == 0xffffffffu) continue;
            const int y = y0 + r, qy = y + (int)((best >> 8) & 255u) - R, qx = x + (int)(best & 255u) - R;   // a staged valid pixel: inside the image
            const T* src = img + ((size_t)qy * W + qx) * 3;
            T* dst = img + ((size_t)y * W + x) * 3;
            const T a = src[0], b = src[1], c = src[2];
            dst[0] = a; dst[1] = b; dst[2] = c;
        }
    }
}

// Wd: one word of `scale` samples; an output row holds 3 W of them, an output pixel row of one input pixel three
template <class Wd>
__global__ void __launch_bounds__(256) nodata_mask_kernel(const uint8_t* __restrict__ valid, int W, int scale, int iy0, int iy1, int yb, int ye,
                                                          Wd fill, Wd* __restrict__ out) {
    const size_t n = (size_t)(iy1 - iy0) * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int iy = iy0 + (int)(i / W), ix = (int)(i % W);
        if (valid[(size_t)iy * W + ix]) continue;
        const int o0 = iy * scale > yb ? iy * scale : yb, o1 = iy * scale + scale < ye ? iy * scale + scale : ye;
        for (int oy = o0; oy < o1; ++oy) {
            Wd* p = out + ((size_t)oy * W + ix) * 3;
            p[0] = fill; p[1] = fill; p[2] = fill;
        }
    }
}

template <class T>
hipError_t fill_impl(T* d_img, const uint8_t* d_valid, int H, int W, int radius, hipStream_t st) {
    if (!d_img || !d_valid || H <= 0 || W <= 0 || radius < 1 || radius > kMaxRadius) return hipErrorInvalidValue;
    const long long tiles_x = ((long long)W + kFillCols - 1) / kFillCols, ntiles = tiles_x * (((long long)H + kFillRows - 1) / kFillRows);
    if (ntiles > 0x7fffffffLL) return hipErrorInvalidValue;
    const int SW = kFillCols + 2 * radius, SH = kFillRows + 2 * radius;
    const int lds = ((SH * SW + 15) & ~15) + kFillRows * SW;         // R = 64: 61440 bytes, inside the 64 KB a kernel gets without opting in
    const unsigned grid = (unsigned)capped_grid((int)(ntiles < 16384 ? ntiles : 16384), ntiles, GF_NODATA);
    hipLaunchKernelGGL(nodata_fill_kernel<T>, dim3(grid), dim3(kFillThreads), lds, st, d_img, d_valid, H, W, radius, (int)tiles_x, (int)ntiles);
    return hipGetLastError();
}

template <class Wd>
hipError_t mask_launch(const uint8_t* d_valid, int W, int scale, int yb, int ye, Wd fill, void* d_out, hipStream_t st) {
    if ((uintptr_t)d_out % sizeof(Wd)) return hipErrorInvalidValue;
    const int iy0 = yb / scale, iy1 = (ye + scale - 1) / scale;
    const size_t n = (size_t)(iy1 - iy0) * W;
    hipLaunchKernelGGL(nodata_mask_kernel<Wd>, dim3((unsigned)stride_grid(n, 8192, GF_NODATA)), dim3(256), 0, st, d_valid, W, scale, iy0, iy1, yb, ye, fill, (Wd*)d_out);
    return hipGetLastError();
}

bool mask_args_ok(const void* d_valid, const void* d_out, int H, int W, int scale, int yb, int ye, int out_nodata, int max_value) {
    return d_valid && d_out && H > 0 && W > 0 && (scale == 2 || scale == 4) && yb >= 0 && yb < ye && (long long)ye <= (long long)H * scale &&
           out_nodata >= 0 && out_nodata <= max_value;
}

}  // namespace

// Fills the invalid pixels of d_img [H, W, 3] in place (d_valid: uint8 [H, W] on the device); radius 1..64.
hipError_t launch_nodata_fill(uint8_t* d_img, const uint8_t* d_valid, int H, int W, int radius, hipStream_t st) {
    return fill_impl(d_img, d_valid, H, W, radius, st);
}
hipError_t launch_nodata_fill(uint16_t* d_img, const uint8_t* d_valid, int H, int W, int radius, hipStream_t st) {
    return fill_impl(d_img, d_valid, H, W, radius, st);
}

// out_nodata into the output pixels of every invalid input pixel, rows [yb, ye) of d_out [scale H, scale W, 3] (the whole image's
// base; aligned to scale samples); d_valid: uint8 [H, W]; scale 2 or 4.
hipError_t launch_nodata_mask(const uint8_t* d_valid, int H, int W, int scale, int yb, int ye, int out_nodata, uint8_t* d_out, hipStream_t st) {
    if (!mask_args_ok(d_valid, d_out, H, W, scale, yb, ye, out_nodata, 255)) return hipErrorInvalidValue;
    const uint32_t v = (uint32_t)out_nodata * 0x01010101u;
    return scale == 4 ? mask_launch<uint32_t>(d_valid, W, 4, yb, ye, v, d_out, st) : mask_launch<uint16_t>(d_valid, W, 2, yb, ye, (uint16_t)v, d_out, st);
}
hipError_t launch_nodata_mask(const uint8_t* d_valid, int H, int W, int scale, int yb, int ye, int out_nodata, uint16_t* d_out, hipStream_t st) {
    if (!mask_args_ok(d_valid, d_out, H, W, scale, yb, ye, out_nodata, 65535)) return hipErrorInvalidValue;
    const uint32_t v = (uint32_t)out_nodata * 0x00010001u;
    return scale == 4 ? mask_launch<uint2>(d_valid, W, 4, yb, ye, make_uint2(v, v), d_out, st) : mask_launch<uint32_t>(d_valid, W, 2, yb, ye, v, d_out, st);
}

}  // namespace s2sr
