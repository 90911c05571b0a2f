// Carrying an extra band to the SR grid: guided upsampling of a uint16 band [H, W] against the uint16 image
// [S H, S W, 3] a 16-bit door produced, then the consistency pass's exact step, so that every block mean is the measured band value
// again.  Integers throughout; the numpy restatement is tests/bands_model.py.
//
// Definition.  S = 2 or 4, n = S S.  q: the guide.  w0..w2 the guide weights, Wt their sum.  p = clamp(b, lo, hi).
//   guide    I[Y, X] = floor((w0 q0 + w1 q1 + w2 q2) / Wt);  G[y, x] = floor(blocksum(I) / n).
//   coeffs   per valid pixel, over the valid pixels of the window [y - r, y + r] x [x - r, x + r] cut at the border: N, SG, Sp, SGG, SGp;
//            cov = N SGp - SG Sp, var = N SGG - SG SG;  A = clamp(floor((cov << 16) / (var + N N eps)), -(4 << 16), 4 << 16) (Q16, gain
//            limit 4);  C = floor(((Sp << 16) - A SG) / N).  Invalid pixels: A = C = 0.
//   apply    A and C interpolated bilinearly between input-pixel centres with the consistency pass's weights (output row Y = S y + i:
//            t = 2 i + 1 - S, neighbour row clamp(y + sign(t), 0, H - 1), weights |t| and 2 S - |t|; columns alike), an invalid
//            neighbour replaced by the pixel itself;  Abar, Cbar the undivided sums, den = 4 S S;
//            g0 = floor((Abar I + Cbar + (den << 15)) / (den << 16)), g = clamp(g0, lo, hi).
//   exact    e = n p - blocksum(g), k = floor(e / n), rr = e - n k; sample (i, j) gets k + (rank[i][j] < rr), rank the Bayer order of
//            consistency.hip;  g' = clamp(g + d, lo, hi).  Invalid blocks are written `fill`.
//   inexact  the valid blocks whose final sum differs from n p.
// Widths.  G, p <= 65535 and N <= 81 (r = 4): SG, Sp < 2^23 (int32), SGG, SGp < 2^39, N SGp < 2^45, cov <= N N 65535^2 / 4 < 2^43,
// cov << 16 < 2^59; var + N N eps < 2^45 + 2^13 eps.  |A| <= 2^18, A SG < 2^41, C < 2^36 in magnitude.  Abar <= 64 2^18 = 2^24 (int32),
// Abar I < 2^40, Cbar < 2^42: int64 holds every intermediate, and den << 16 is a power of two: the apply step divides by a shift.
// floor(x / Wt) for x < 2^26 is (x m) >> sh with m = floor(2^sh / Wt) + 1, sh = 26 + ceil(log2 Wt) (Granlund & Montgomery 1994): the
// launcher computes m, sh; no division per sample anywhere.  The two 64-bit floor divisions of `coeffs` are per INPUT pixel.
//
// Two kernels, workgroups of 256 threads on tiles of 16 x 16 input pixels, grid-stride over the tiles of rows [y0, y1).
//   band_coeffs  stages G (formed from the guide: S rows of 3 S samples per pixel, as dwords -- a guide row is 6 S W bytes, a block's
//                run 6 S bytes: both multiples of 4 for even S), p and the mask of the tile and a halo of r in LDS, out-of-image pixels
//                as invalid; a thread takes one pixel: the five sums, the two divisions; A into an int32 plane, C into an int64 plane.
//   band_apply   stages the 18 x 18 ring of A, C and the mask with clamped indices; a thread takes one block, its n samples in
//                registers: I from the guide (dwords), g0, the clip, the sum, the remainder spread, the recount; stores the block's
//                rows of the uint16 plane [S H, S W] as dwords (a row is 2 S W bytes, a block's run 2 S).  inexact is counted per
//                workgroup in LDS, then one vector atomic into a device uint64.
// 64-bit offsets; every index comes from sizes the launcher has checked.
#include "s2sr_internal.h"

namespace s2sr {

namespace {

constexpr int kTI = 16, kThreads = 256, kMaxR = 4, kHaloW = kTI + 2 * kMaxR, kRing = kTI + 2;

typedef uint32_t __attribute__((may_alias)) word_t;

struct GuideDiv { uint32_t w0, w1, w2, m, sh; };     // I = ((w0 q0 + w1 q1 + w2 q2) * m) >> sh

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
__device__ __forceinline__ long long floor_div(long long a, long long b) {     // b > 0
    long long q = a / b;
    return q * b > a ? q - 1 : q;
}

// the S guide values of row `row` of block column bx: 3 S samples = 3 S / 2 dwords
template <int S>
__device__ __forceinline__ void guide_row(const uint16_t* __restrict__ q, size_t row_s, size_t row, int bx, const GuideDiv& gd, int (&I)[S]) {
    constexpr int NW = 3 * S / 2;
    const word_t* src = (const word_t*)(q + row * row_s + (size_t)bx * (3 * S));
    uint32_t v[2 * NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const uint32_t d = src[k];
        v[2 * k] = d & 0xffffu;
        v[2 * k + 1] = d >> 16;
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const uint32_t x = gd.w0 * v[3 * j] + gd.w1 * v[3 * j + 1] + gd.w2 * v[3 * j + 2];
        I[j] = (int)(((unsigned long long)x * gd.m) >> gd.sh);
    }
}

// q: the guide [S H, S W, 3].  band: [H, W].  valid: [H, W] or null.  A: int32 [H, W], C: int64 [H, W]; written for pixel rows [y0, y1).
template <int S>
__global__ void __launch_bounds__(kThreads) band_coeffs_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ band,
                                                               const uint8_t* __restrict__ valid, int32_t* __restrict__ A,
                                                               long long* __restrict__ C, int H, int W, int y0, int y1, int lo, int hi,
                                                               GuideDiv gd, int r, long long eps, int tiles_x, int ntiles) {
    constexpr int log_n = S == 4 ? 4 : 2;
    __shared__ int Gs[kHaloW * kHaloW], ps[kHaloW * kHaloW];
    __shared__ uint8_t ms[kHaloW * kHaloW];
    const int tid = threadIdx.x;
    const size_t row_s = (size_t)W * S * 3;
    const int hw = kTI + 2 * r;                                                  // the staged side
    const int yend = y1 + r < H ? y1 + r : H;                                    // no window of rows [y0, y1) reaches further down
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {                       // (t is uniform over the workgroup: so is every barrier)
        const int ty0 = y0 + (t / tiles_x) * kTI, tx0 = (t % tiles_x) * kTI;
        __syncthreads();                                                         // the tile before has left the LDS
        for (int i = tid; i < hw * hw; i += kThreads) {
            const int ly = i / hw, lx = i - ly * hw;
            const int y = ty0 - r + ly, x = tx0 - r + lx;
            int g = 0, p = 0, m = 0;
            if (y >= 0 && y < yend && x >= 0 && x < W) {
                const size_t px = (size_t)y * W + x;
                m = valid ? valid[px] != 0 : 1;
                if (m) {                                                         // (an invalid pixel's samples are never looked at)
                    p = clampi((int)band[px], lo, hi);
                    unsigned int sum = 0;
#pragma unroll
                    for (int k = 0; k < S; ++k) {
                        int I[S];
                        guide_row<S>(q, row_s, (size_t)y * S + k, x, gd, I);
#pragma unroll
                        for (int j = 0; j < S; ++j) sum += (unsigned int)I[j];
                    }
                    g = (int)(sum >> log_n);
                }
            }
            Gs[ly * kHaloW + lx] = g;
            ps[ly * kHaloW + lx] = p;
            ms[ly * kHaloW + lx] = (uint8_t)m;
        }
        __syncthreads();
        const int by = tid / kTI, bx = tid % kTI;
        const int y = ty0 + by, x = tx0 + bx;
        if (y >= y1 || x >= W) continue;
        const size_t px = (size_t)y * W + x;
        int a = 0;
        long long c = 0;
        if (ms[(by + r) * kHaloW + bx + r]) {
            int N = 0, SG = 0, Sp = 0;
            unsigned long long SGG = 0, SGp = 0;
            for (int dy = 0; dy <= 2 * r; ++dy)
                for (int dx = 0; dx <= 2 * r; ++dx) {
                    const int o = (by + dy) * kHaloW + bx + dx;
                    if (!ms[o]) continue;
                    const unsigned int g = (unsigned int)Gs[o], p = (unsigned int)ps[o];
                    N += 1; SG += (int)g; Sp += (int)p;
                    SGG += (unsigned long long)g * g;
                    SGp += (unsigned long long)g * p;
                }
            const long long cov = (long long)N * (long long)SGp - (long long)SG * Sp;
            const long long var = (long long)N * (long long)SGG - (long long)SG * SG;
            long long aa = floor_div(cov * 65536, var + (long long)N * N * eps);
            constexpr long long kGain = 4ll << 16;
            aa = aa < -kGain ? -kGain : aa > kGain ? kGain : aa;
            a = (int)aa;
            c = floor_div(((long long)Sp << 16) - aa * SG, N);
        }
        A[px] = a;
        C[px] = c;
    }
}

// out: the uint16 plane [S H, S W], written for block rows [by0, by1).  A, C: read for block rows by0 - 1 .. by1 (clamped to the image).
template <int S>
__global__ void __launch_bounds__(kThreads) band_apply_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ band,
                                                              const uint8_t* __restrict__ valid, const int32_t* __restrict__ A,
                                                              const long long* __restrict__ C, uint16_t* __restrict__ out,
                                                              unsigned long long* __restrict__ cnt, int H, int W, int by0, int by1, int lo,
                                                              int hi, GuideDiv gd, int fill, int tiles_x, int ntiles) {
    constexpr int n = S * S, log_n = S == 4 ? 4 : 2, log_den = 2 + log_n + 16;   // den << 16 = 4 S S 2^16
    __shared__ long long Cs[kRing * kRing];
    __shared__ int As[kRing * kRing];
    __shared__ uint8_t ms[kRing * kRing];
    __shared__ unsigned int bad;
    const int tid = threadIdx.x;
    const size_t row_s = (size_t)W * S * 3, orow = (size_t)W * S;
    const int ymax = by1 < H - 1 ? by1 : H - 1;                                  // the last coefficient row blocks [by0, by1) read
    if (tid == 0) bad = 0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int ty0 = by0 + (t / tiles_x) * kTI, tx0 = (t % tiles_x) * kTI;
        __syncthreads();
        for (int i = tid; i < kRing * kRing; i += kThreads) {
            const int ly = i / kRing, lx = i - ly * kRing;
            const int yy = clampi(ty0 - 1 + ly, 0, ymax), xx = clampi(tx0 - 1 + lx, 0, W - 1);
            const size_t px = (size_t)yy * W + xx;
            As[i] = A[px];
            Cs[i] = C[px];
            ms[i] = valid ? (uint8_t)(valid[px] != 0) : (uint8_t)1;
        }
        __syncthreads();
        const int by = tid / kTI, bx = tid % kTI;
        const int y = ty0 + by, x = tx0 + bx;
        if (y >= by1 || x >= W) continue;
        const int o = (by + 1) * kRing + bx + 1;
        word_t* dst = (word_t*)(out + (size_t)y * S * orow + (size_t)x * S);
        if (!ms[o]) {
            const word_t f = (word_t)fill | ((word_t)fill << 16);
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int k = 0; k < S / 2; ++k) dst[i * (orow / 2) + k] = f;
            continue;
        }
        const int p = clampi((int)band[(size_t)y * W + x], lo, hi);
        // the 3 x 3 neighbourhood, invalid neighbours replaced by the pixel itself
        int a[3][3];
        long long c[3][3];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int oo = ms[o + dy * kRing + dx] ? o + dy * kRing + dx : o;
                a[dy + 1][dx + 1] = As[oo];
                c[dy + 1][dx + 1] = Cs[oo];
            }
        int g[S][S], sum = 0;
#pragma unroll
        for (int i = 0; i < S; ++i) {
            const int ty = 2 * i + 1 - S, sy = ty < 0 ? 0 : 2, wy1 = ty < 0 ? -ty : ty, wy0 = 2 * S - wy1;
            int I[S];
            guide_row<S>(q, row_s, (size_t)y * S + i, x, gd, I);
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const int tx = 2 * j + 1 - S, sx = tx < 0 ? 0 : 2, wx1 = tx < 0 ? -tx : tx, wx0 = 2 * S - wx1;
                const int ab = wy0 * (wx0 * a[1][1] + wx1 * a[1][sx]) + wy1 * (wx0 * a[sy][1] + wx1 * a[sy][sx]);
                const long long cb = wy0 * (wx0 * c[1][1] + wx1 * c[1][sx]) + wy1 * (wx0 * c[sy][1] + wx1 * c[sy][sx]);
                const long long lin = (long long)ab * I[j] + cb + (1ll << (log_den - 1));
                const long long g0 = lin >> log_den;                              // floor: an arithmetic shift
                g[i][j] = g0 < lo ? lo : g0 > hi ? hi : (int)g0;
                sum += g[i][j];
            }
        }
        const int er = n * p - sum, k = er >> log_n, rr = er & (n - 1);           // floor(e / n) and the remainder in 0..n-1
        sum = 0;
#pragma unroll
        for (int i = 0; i < S; ++i) {
#pragma unroll
            for (int j = 0; j < S; ++j) {
                g[i][j] = clampi(g[i][j] + k + (Rank<S>::at(i, j) < rr ? 1 : 0), lo, hi);
                sum += g[i][j];
            }
#pragma unroll
            for (int kk = 0; kk < S / 2; ++kk) dst[i * (orow / 2) + kk] = (word_t)g[i][2 * kk] | ((word_t)g[i][2 * kk + 1] << 16);
        }
        if (sum != n * p) atomicAdd(&bad, 1u);
    }
    __syncthreads();
    if (tid == 0 && bad) atomicAdd(cnt, (unsigned long long)bad);
}

bool guide_div(const int w[3], GuideDiv& gd) {
    int wt = 0;
    for (int c = 0; c < 3; ++c) {
        if (w[c] < 0 || w[c] > 255) return false;
        wt += w[c];
    }
    if (wt < 1) return false;
    int l = 0;
    while ((1 << l) < wt) ++l;
    gd.w0 = (uint32_t)w[0]; gd.w1 = (uint32_t)w[1]; gd.w2 = (uint32_t)w[2];
    gd.sh = 26 + l;                                                              // x <= 765 * 65535 < 2^26
    gd.m = (uint32_t)(((1ull << gd.sh) / (unsigned)wt) + 1);                     // < 2^27 + 1
    return true;
}

bool common_ok(const uint16_t* d_q, const uint16_t* d_band, const void* d_A, const void* d_C, int H, int W, int S, int y0, int y1, int lo, int hi) {
    return d_q && d_band && d_A && d_C && H > 0 && W > 0 && (S == 2 || S == 4) && y0 >= 0 && y0 < y1 && y1 <= H && lo >= 0 && lo < hi &&
           hi <= 65535 && (uintptr_t)d_q % 4 == 0 && (uintptr_t)d_A % 4 == 0 && (uintptr_t)d_C % 8 == 0 &&
           (long long)W * S * 3 <= 0x3fffffffLL && (long long)H * S <= 0x3fffffffLL;
}

bool tile_grid(int W, int rows, int& tiles_x, int& ntiles, unsigned& grid) {
    const long long tx = ((long long)W + kTI - 1) / kTI, nt = tx * (((long long)rows + kTI - 1) / kTI);
    if (nt > 0x7fffffffLL) return false;
    tiles_x = (int)tx; ntiles = (int)nt;
    grid = (unsigned)capped_grid((int)(nt < 16384 ? nt : 16384), nt, GF_BANDS);
    return true;
}

}  // namespace

hipError_t launch_band_coeffs(const uint16_t* d_q, const uint16_t* d_band, const uint8_t* d_valid, int32_t* d_A, long long* d_C, int H, int W,
                              int S, int y0, int y1, int lo, int hi, const int w[3], int r, long long eps, hipStream_t st) {
    GuideDiv gd;
    int tiles_x, ntiles;
    unsigned grid;
    if (!common_ok(d_q, d_band, d_A, d_C, H, W, S, y0, y1, lo, hi) || r < 1 || r > kMaxR || eps < 1 || eps > (1ll << 40) || !guide_div(w, gd) ||
        !tile_grid(W, y1 - y0, tiles_x, ntiles, grid))
        return hipErrorInvalidValue;
    if (S == 4)
        hipLaunchKernelGGL(band_coeffs_kernel<4>, dim3(grid), dim3(kThreads), 0, st, d_q, d_band, d_valid, d_A, d_C, H, W, y0, y1, lo, hi, gd, r, eps, tiles_x, ntiles);
    else
        hipLaunchKernelGGL(band_coeffs_kernel<2>, dim3(grid), dim3(kThreads), 0, st, d_q, d_band, d_valid, d_A, d_C, H, W, y0, y1, lo, hi, gd, r, eps, tiles_x, ntiles);
    return hipGetLastError();
}

hipError_t launch_band_apply(const uint16_t* d_q, const uint16_t* d_band, const uint8_t* d_valid, const int32_t* d_A, const long long* d_C,
                             uint16_t* d_out, unsigned long long* d_cnt, int H, int W, int S, int by0, int by1, int lo, int hi, const int w[3],
                             int fill, hipStream_t st) {
    GuideDiv gd;
    int tiles_x, ntiles;
    unsigned grid;
    if (!common_ok(d_q, d_band, d_A, d_C, H, W, S, by0, by1, lo, hi) || !d_out || !d_cnt || (uintptr_t)d_out % 4 || (uintptr_t)d_cnt % 8 ||
        fill < 0 || fill > 65535 || !guide_div(w, gd) || !tile_grid(W, by1 - by0, tiles_x, ntiles, grid))
        return hipErrorInvalidValue;
    if (S == 4)
        hipLaunchKernelGGL(band_apply_kernel<4>, dim3(grid), dim3(kThreads), 0, st, d_q, d_band, d_valid, d_A, d_C, d_out, d_cnt, H, W, by0, by1, lo, hi, gd, fill, tiles_x, ntiles);
    else
        hipLaunchKernelGGL(band_apply_kernel<2>, dim3(grid), dim3(kThreads), 0, st, d_q, d_band, d_valid, d_A, d_C, d_out, d_cnt, H, W, by0, by1, lo, hi, gd, fill, tiles_x, ntiles);
    return hipGetLastError();
}

}  // namespace s2sr
