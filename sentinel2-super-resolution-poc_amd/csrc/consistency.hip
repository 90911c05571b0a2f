// Radiometric consistency: one back-projection step against the box-average sensor model, so that the mean of the
// S x S output samples over an input pixel is that input pixel again.  Integers throughout; the numpy restatement is
// tests/consistency_model.py.
//
// Definition, per channel.  S = 2 or 4, n = S S.  q: the quantised image [S H, S W, 3].  v = clamp(img, lo, hi): the input the net
// saw (8 bits: lo, hi = 0, 255).  sum[y, x] = the sum of q over block [S y, S y + S) x [S x, S x + S);  e = n v - sum.
//   exact   k = floor(e / n), r = e - n k in 0..n-1; block sample (i, j) gets d = k + (rank[i][j] < r), rank the 4 x 4 Bayer order
//           (S = 2: [[0,2],[3,1]]);  q' = clip(q + d, lo, hi).  Where no sample of a block clips, sum' = n v.
//   smooth  the residual interpolated bilinearly between input-pixel centres, edges replicated: output row Y = S y + i has
//           t = 2 i + 1 - S, neighbour row clamp(y + sign(t), 0, H - 1), weights w1 = |t| for the neighbour and w0 = 2 S - w1 for
//           y; columns alike;  num = sum of wy wx e over the four pairs, den = 4 S S n, d = floor((num + den / 2) / den),
//           q' = clip(q + d, lo, hi).  |e| <= 16 * 65535 and wy wx sums to 4 S S <= 64: int32 holds every intermediate.
//   mode 1  the exact step.   mode 2  the smooth step, the block sums again on its result, the exact step on what remains.
//   inexact[c] = the blocks of channel c whose final sum differs from n v (a sample clipped).
//
// One kernel template, three forms.  A workgroup of 256 threads owns a tile of 64 x 64 output pixels (16 x 16 input pixels at
// S = 4, 32 x 32 at S = 2): it stages the tile's samples in LDS (dword loads where every row starts on a dword, sample loads
// otherwise: an output row is 3 S W esz bytes, only 2-byte aligned for S = 2 / uint8 / odd W), then a thread takes one (block,
// channel) at a time, its S x S samples in registers -- sums, steps, clips and the recount need no other thread -- writes them back
// to LDS, and the tile leaves as it came.  In place.
//   FORM_RESIDUAL  e of every block of the band into a residual plane int32 [H, W, 3]; the image is only read.
//   FORM_EXACT     mode 1.
//   FORM_SMOOTH    mode 2; the residuals of the tile's blocks and of one ring around them come from the residual plane ((TI + 2)^2 x 3
//                  int32 in LDS, indices clamped to the image: the edge replication).
// Mode 2 is two launches because the pass runs in place: a workgroup that took its neighbours' residuals from the image would
// race their owners' stores, and a residual taken from a corrected block is 0.  The plane costs 12 bytes per input pixel
// written and read again, next to S S 3 esz bytes of image per input pixel read twice and written once.
// inexact: counted per workgroup in LDS, then one vector atomic per channel into a device uint64[3].
// Grid-stride loops over the tiles, 64-bit offsets, every index from sizes the launcher has checked.
#include "s2sr_internal.h"

namespace s2sr {

namespace {

constexpr int kTile = 64, kPitch = kTile * 3, kThreads = 256;     // output pixels per tile side; samples per staged row
enum { FORM_RESIDUAL = 0, FORM_EXACT = 1, FORM_SMOOTH = 2 };

typedef uint32_t __attribute__((may_alias)) word_t;

template <int S> struct Rank;
template <> struct Rank<4> { static __device__ __forceinline__ int at(int i, int j) {
    constexpr int r[4][4] = {{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}};
    return r[i][j];
} };
template <> struct Rank<2> { static __device__ __forceinline__ int at(int i, int j) {
    constexpr int r[2][2] = {{0, 2}, {3, 1}};
    return r[i][j];
} };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// img: [S H, S W, 3], read and (but for FORM_RESIDUAL) written in block rows [by0, by1).  lr: [H, W, 3], the input.  swap: image
// channel c is input channel 2 - c.  e: the residual plane.  cnt: uint64[3].  wide: every image row starts on a dword.
template <class T, int S, int FORM>
__global__ void __launch_bounds__(kThreads) consistency_kernel(T* __restrict__ img, const T* __restrict__ lr, int32_t* __restrict__ e,
                                                               unsigned long long* __restrict__ cnt, int H, int W, int by0, int by1, int lo,
                                                               int hi, int swap, int wide, int tiles_x, int ntiles) {
    constexpr int TI = kTile / S, n = S * S, EW = TI + 2;
    constexpr int log_n = S == 4 ? 4 : 2, log_den = 2 + 2 * log_n;               // den = 4 S S n = 4 n n
    constexpr int kRowWords = kPitch * (int)sizeof(T) / 4;
    __shared__ __attribute__((aligned(16))) T qs[kTile * kPitch];
    __shared__ int32_t es[FORM == FORM_SMOOTH ? EW * EW * 3 : 1];
    __shared__ unsigned int bad[3];
    const int tid = threadIdx.x;
    const size_t row_s = (size_t)W * S * 3;                                      // samples of one image row
    if (tid < 3) bad[tid] = 0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {                       // (t is uniform over the workgroup: so is every barrier)
        const int y0 = by0 + (t / tiles_x) * TI, x0 = (t % tiles_x) * TI;        // the tile's first block
        const int nby = by1 - y0 < TI ? by1 - y0 : TI, nbx = W - x0 < TI ? W - x0 : TI;
        const int rows = nby * S, row_n = nbx * S * 3;                           // staged rows, samples in each
        T* g = img + (size_t)y0 * S * row_s + (size_t)x0 * S * 3;
        __syncthreads();                                                         // the tile before has left qs and es
        if (wide) {                                                              // row_n * sizeof(T) is a multiple of 4 here (launcher)
            const int wpr = row_n * (int)sizeof(T) / 4;
            for (int i = tid; i < rows * wpr; i += kThreads) {
                const int r = i / wpr, w = i - r * wpr;
                ((word_t*)qs)[r * kRowWords + w] = ((const word_t*)(g + (size_t)r * row_s))[w];
            }
        } else {
            for (int i = tid; i < rows * row_n; i += kThreads) {
                const int r = i / row_n, w = i - r * row_n;
                qs[r * kPitch + w] = g[(size_t)r * row_s + w];
            }
        }
        if (FORM == FORM_SMOOTH) {
            const int ew = nbx + 2;
            for (int i = tid; i < (nby + 2) * ew * 3; i += kThreads) {
                const int c = i % 3, lx = (i / 3) % ew, ly = i / (3 * ew);
                const int yy = clampi(y0 - 1 + ly, 0, H - 1), xx = clampi(x0 - 1 + lx, 0, W - 1);
                es[(ly * EW + lx) * 3 + c] = e[((size_t)yy * W + xx) * 3 + c];
            }
        }
        __syncthreads();
        for (int it = tid; it < nby * nbx * 3; it += kThreads) {
            const int c = it % 3, bx = (it / 3) % nbx, by = it / (3 * nbx);
            const size_t px = (size_t)(y0 + by) * W + (x0 + bx);
            const int v = clampi((int)lr[px * 3 + (swap ? 2 - c : c)], lo, hi);
            T* q0 = qs + (by * S) * kPitch + (bx * S) * 3 + c;
            int q[S][S], sum = 0;
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int j = 0; j < S; ++j) { q[i][j] = q0[i * kPitch + j * 3]; sum += q[i][j]; }
            if (FORM == FORM_RESIDUAL) {
                e[px * 3 + c] = n * v - sum;
                continue;
            }
            if (FORM == FORM_SMOOTH) {
                const int32_t* ec = es + ((by + 1) * EW + (bx + 1)) * 3 + c;     // ec[(dy * EW + dx) * 3], dy, dx in -1..1
                sum = 0;
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    const int ty = 2 * i + 1 - S, sy = ty < 0 ? -1 : 1, wy1 = ty < 0 ? -ty : ty, wy0 = 2 * S - wy1;
#pragma unroll
                    for (int j = 0; j < S; ++j) {
                        const int tx = 2 * j + 1 - S, sx = tx < 0 ? -1 : 1, wx1 = tx < 0 ? -tx : tx, wx0 = 2 * S - wx1;
                        const int num = wy0 * (wx0 * ec[0] + wx1 * ec[sx * 3]) + wy1 * (wx0 * ec[sy * EW * 3] + wx1 * ec[(sy * EW + sx) * 3]);
                        const int d = (num + (1 << (log_den - 1))) >> log_den;   // floor: an arithmetic shift
                        q[i][j] = clampi(q[i][j] + d, lo, hi);
                        sum += q[i][j];
                    }
                }
            }
            const int er = n * v - sum, k = er >> log_n, r = er & (n - 1);     // floor(e / n) and the remainder in 0..n-1
            sum = 0;
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    const int o = clampi(q[i][j] + k + (Rank<S>::at(i, j) < r ? 1 : 0), lo, hi);
                    q0[i * kPitch + j * 3] = (T)o;
                    sum += o;
                }
            if (sum != n * v) atomicAdd(&bad[c], 1u);
        }
        if (FORM == FORM_RESIDUAL) continue;
        __syncthreads();
        if (wide) {
            const int wpr = row_n * (int)sizeof(T) / 4;
            for (int i = tid; i < rows * wpr; i += kThreads) {
                const int r = i / wpr, w = i - r * wpr;
                ((word_t*)(g + (size_t)r * row_s))[w] = ((const word_t*)qs)[r * kRowWords + w];
            }
        } else {
            for (int i = tid; i < rows * row_n; i += kThreads) {
                const int r = i / row_n, w = i - r * row_n;
                g[(size_t)r * row_s + w] = qs[r * kPitch + w];
            }
        }
    }
    if (FORM == FORM_RESIDUAL) return;
    __syncthreads();
    if (tid < 3 && bad[tid]) atomicAdd(cnt + tid, (unsigned long long)bad[tid]);
}

template <class T, int S>
hipError_t launch_form(int form, T* d_img, const T* d_lr, int32_t* d_e, unsigned long long* d_cnt, int H, int W, int by0, int by1, int lo,
                       int hi, int swap, hipStream_t st) {
    constexpr int TI = kTile / S;
    const long long tiles_x = ((long long)W + TI - 1) / TI, ntiles = tiles_x * (((long long)(by1 - by0) + TI - 1) / TI);
    if (ntiles > 0x7fffffffLL) return hipErrorInvalidValue;
    // dword rows: the image's base and the bytes of a row are multiples of 4 (a tile's first column, 64 k pixels, always is; a
    // ragged tile's row then holds S (W - x0) 3 esz bytes, a multiple of 4 with the row)
    const int wide = (uintptr_t)d_img % 4 == 0 && ((size_t)W * S * 3 * sizeof(T)) % 4 == 0;
    const unsigned grid = (unsigned)capped_grid((int)(ntiles < 16384 ? ntiles : 16384), ntiles, GF_CONSISTENCY);
    const dim3 g(grid), b(kThreads);
    if (form == FORM_RESIDUAL)
        hipLaunchKernelGGL((consistency_kernel<T, S, FORM_RESIDUAL>), g, b, 0, st, d_img, d_lr, d_e, d_cnt, H, W, by0, by1, lo, hi, swap, wide, (int)tiles_x, (int)ntiles);
    else if (form == FORM_EXACT)
        hipLaunchKernelGGL((consistency_kernel<T, S, FORM_EXACT>), g, b, 0, st, d_img, d_lr, d_e, d_cnt, H, W, by0, by1, lo, hi, swap, wide, (int)tiles_x, (int)ntiles);
    else
        hipLaunchKernelGGL((consistency_kernel<T, S, FORM_SMOOTH>), g, b, 0, st, d_img, d_lr, d_e, d_cnt, H, W, by0, by1, lo, hi, swap, wide, (int)tiles_x, (int)ntiles);
    return hipGetLastError();
}

template <class T>
hipError_t launch_impl(int form, T* d_img, const T* d_lr, int32_t* d_e, unsigned long long* d_cnt, int H, int W, int S, int by0, int by1,
                       int lo, int hi, int swap, int max_value, hipStream_t st) {
    if (!d_img || !d_lr || !d_cnt || H <= 0 || W <= 0 || (S != 2 && S != 4) || by0 < 0 || by0 >= by1 || by1 > H || lo < 0 || lo > hi ||
        hi > max_value || form < FORM_RESIDUAL || form > FORM_SMOOTH || (form != FORM_EXACT && !d_e) || (uintptr_t)d_img % sizeof(T))
        return hipErrorInvalidValue;
    if ((long long)W * S * 3 > 0x7fffffffLL / 2) return hipErrorInvalidValue;                  // (a row's samples stay far inside int)
    return S == 4 ? launch_form<T, 4>(form, d_img, d_lr, d_e, d_cnt, H, W, by0, by1, lo, hi, swap, st)
                  : launch_form<T, 2>(form, d_img, d_lr, d_e, d_cnt, H, W, by0, by1, lo, hi, swap, st);
}

}  // namespace

hipError_t launch_consistency(int form, uint8_t* d_img, const uint8_t* d_lr, int32_t* d_e, unsigned long long* d_cnt, int H, int W, int S,
                              int by0, int by1, int swap, hipStream_t st) {
    return launch_impl(form, d_img, d_lr, d_e, d_cnt, H, W, S, by0, by1, 0, 255, swap, 255, st);
}
hipError_t launch_consistency(int form, uint16_t* d_img, const uint16_t* d_lr, int32_t* d_e, unsigned long long* d_cnt, int H, int W, int S,
                              int by0, int by1, int lo, int hi, hipStream_t st) {
    return launch_impl(form, d_img, d_lr, d_e, d_cnt, H, W, S, by0, by1, lo, hi, 0, 65535, st);
}

}  // namespace s2sr
