// Display rendering of 16-bit images: the two passes over the image that turn a uint16 [H, W, 3] raster into the
// 8-bit image the PNG writer, the warp, the pyramid and the post-process take.  The policy between the passes -- percentile limits
// from the histogram, the stretch LUT -- is 3 x 65536 numbers and lives in Python (s2sr/display.py).
//
// Definition (integers where it matters):
//   image     uint16 [H, W, 3], interleaved.  nodata: 0..65535, or -1 for none.  A sample equal to nodata is left out of the
//             statistics of its channel; it is still mapped like any other sample.
//   hist      hist[c][v] = number of counted samples of channel c with value v, exact (uint64).
//   limits    percentiles in whole basis points bp, 0 <= bp_lo < bp_hi <= 10000.  For a histogram g with n = sum(g) counted
//             samples: k = ((n - 1) * bp) // 10000, limit = the k-th smallest counted sample (0-based) = the smallest v with
//             cumsum(g)[v] >= k + 1.  linked: g = hist[0] + hist[1] + hist[2], one (lo, hi) for all channels; else g = hist[c].
//             n == 0 -> (0, 1).  hi == lo -> (lo - 1, hi) if hi > 0 else (0, 1).
//   lut       lut[c][x] = 0 for x <= lo, 255 for x >= hi; between them (510 * (x - lo) + (hi - lo)) // (2 * (hi - lo)) for
//             gamma == 1 (round half up, in integers), floor(255 * ((x - lo) / (hi - lo)) ** (1 / gamma) + 0.5) in float64 otherwise.
//   out       out[y, x, c] = lut[c][img[y, x, c]].
//
// Both kernels work on a band of whole rows, i.e. on the flat samples [s0, s1) of the image, in groups of 24 samples = 8 pixels =
// three 16-byte loads per lane.  Groups are counted from the image's first sample, so register k of a group holds channel k % 3
// whatever row the band starts at (rows need not start aligned); the image base must be 16-byte aligned and readable up to the next
// multiple of 16 bytes behind its last sample.  A 16-byte vector that lies wholly outside the band is not loaded; samples of a
// loaded vector outside the band are ignored.
//
// Histogram.  3 x 65536 uint32 counters are 768 KB: they do not fit the 160 KB of LDS.  Privatisation: one VALUE RANGE per
// workgroup in LDS.  The values are cut into 8 ranges of 8192; a workgroup owns one (chunk of the band, range) pair, keeps
// 3 x 8192 uint32 counters (96 KB) in LDS, reads its chunk and counts the samples of its range with LDS atomics, then adds its
// non-zero counters to the uint64 global histogram.  The band is read 8 times (from L2 / Infinity Cache after the first), which
// is cheap next to the contention it removes: a global atomic per sample would put every sample of a real raster on a few hundred
// addresses.  Where all active lanes of a wave hold the same value (constant areas: the worst case) one lane adds the wave's count.
// The range of a workgroup rotates with its chunk, so that the 8 workgroups of one range do not all land on one XCD.
// Limits: a band holds at most 2^30 samples (the LDS counters are 32 bits wide; the host side cuts larger bands); global counters
// are 64 bits, so counts are exact for any image.
#include "s2sr_internal.h"

namespace s2sr {

namespace {

constexpr int kRangeBits = 13;                      // 8192 values per range
constexpr int kRangeBins = 1 << kRangeBits;
constexpr int kRanges = 65536 / kRangeBins;         // 8
constexpr int kHistThreads = 1024;
constexpr int kHistLdsBytes = 3 * kRangeBins * 4;   // 96 KB
constexpr int kGroup = 24;                          // samples per lane and step: 8 pixels, three 16-byte vectors

// the 8 samples of a 16-byte vector
__device__ __forceinline__ void unpack8(const uint4& q, uint32_t* v) {
    v[0] = q.x & 0xffffu; v[1] = q.x >> 16; v[2] = q.y & 0xffffu; v[3] = q.y >> 16;
    v[4] = q.z & 0xffffu; v[5] = q.z >> 16; v[6] = q.w & 0xffffu; v[7] = q.w >> 16;
}

__global__ void __launch_bounds__(kHistThreads, 1) display_hist_kernel(const uint16_t* __restrict__ img, size_t s0, size_t s1, int nodata,
                                                                       int chunks, unsigned long long* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bins[];   // [3][kRangeBins]
    const int chunk = blockIdx.x / kRanges;
    const uint32_t range = (uint32_t)(blockIdx.x + chunk) % kRanges;
    for (int i = threadIdx.x; i < 3 * kRangeBins; i += kHistThreads) bins[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const size_t g0 = s0 / kGroup, g1 = (s1 + kGroup - 1) / kGroup;
    for (size_t g = g0 + (size_t)chunk * kHistThreads + threadIdx.x; g < g1; g += (size_t)chunks * kHistThreads) {
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const size_t vb = g * kGroup + 8 * v;
            if (vb + 8 <= s0 || vb >= s1) continue;
            const uint4 q = *(const uint4*)(img + vb);
            uint32_t s[8];
            unpack8(q, s);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = (8 * v + j) % 3;
                const size_t flat = vb + j;
                const uint32_t val = s[j];
                if (flat >= s0 && flat < s1 && (val >> kRangeBits) == range && (int)val != nodata) {
                    const uint32_t bin = (uint32_t)c * kRangeBins + (val & (kRangeBins - 1));
                    const uint32_t first = __builtin_amdgcn_readfirstlane(bin);
                    const unsigned long long active = __ballot(1), same = __ballot(bin == first);
                    if (same == active) {   // one value in the whole wave: one add of the wave's count
                        if (lane == __ffsll((long long)active) - 1) atomicAdd(&bins[bin], (uint32_t)__popcll(active));
                    } else {
                        atomicAdd(&bins[bin], 1u);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * kRangeBins; i += kHistThreads) {
        const uint32_t n = bins[i];
        if (n) atomicAdd(&hist[(size_t)(i >> kRangeBits) * 65536 + range * kRangeBins + (i & (kRangeBins - 1))], (unsigned long long)n);
    }
}

// one lane: a group of 24 samples through the LUTs -> 24 contiguous bytes (three 8-byte stores inside the band, bytes at its edges)
__global__ void __launch_bounds__(256) display_apply_kernel(const uint16_t* __restrict__ img, size_t s0, size_t s1,
                                                            const uint8_t* __restrict__ lut, uint8_t* __restrict__ out) {
    const size_t g0 = s0 / kGroup, g1 = (s1 + kGroup - 1) / kGroup;
    for (size_t g = g0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < g1; g += (size_t)gridDim.x * blockDim.x) {
        const size_t base = g * kGroup;
        const bool whole = base >= s0 && base + kGroup <= s1;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const size_t vb = base + 8 * v;
            if (vb + 8 <= s0 || vb >= s1) continue;
            const uint4 q = *(const uint4*)(img + vb);
            uint32_t s[8], o[8];
            unpack8(q, s);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = lut[(size_t)((8 * v + j) % 3) * 65536 + s[j]];
            if (whole) {
                uint2 w;
                w.x = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
                w.y = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
                *(uint2*)(out + vb) = w;      // base is a multiple of 24: 8-byte aligned
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (vb + j >= s0 && vb + j < s1) out[vb + j] = (uint8_t)o[j];
            }
        }
    }
}

}  // namespace

// Counts the samples [s0, s1) of d_img (s1 - s0 <= 2^30) into d_hist [3][65536] (added to what is there).
hipError_t launch_display_hist(const uint16_t* d_img, size_t s0, size_t s1, int nodata, unsigned long long* d_hist, hipStream_t st) {
    if (s1 <= s0) return hipSuccess;
    if (s1 - s0 > ((size_t)1 << 30) || ((uintptr_t)d_img & 15)) return hipErrorInvalidValue;
    static KernelLaunchState state;
    int ncu = 256;
    hipError_t e = state.prepare((const void*)display_hist_kernel, kHistLdsBytes, &ncu);
    if (e != hipSuccess) return e;
    const size_t groups = (s1 + kGroup - 1) / kGroup - s0 / kGroup;
    size_t chunks = (groups + kHistThreads - 1) / kHistThreads;
    const size_t cap = (size_t)(2 * ncu / kRanges > 1 ? 2 * ncu / kRanges : 1);   // two rounds of one workgroup per CU
    const size_t needed = chunks;
    if (chunks > cap) chunks = cap;
    // the kernel strides over its `chunks` argument, one workgroup per (chunk, range): the grid stays a multiple of kRanges
    chunks = (size_t)capped_grid((int)(chunks * kRanges), (long long)(needed * kRanges), GF_DISPLAY, kRanges) / kRanges;
    hipLaunchKernelGGL(display_hist_kernel, dim3((unsigned)(chunks * kRanges)), dim3(kHistThreads), kHistLdsBytes, st, d_img, s0, s1, nodata,
                       (int)chunks, d_hist);
    return hipGetLastError();
}

// d_out[i] = d_lut[i % 3][d_img[i]] for the samples [s0, s1); d_out is addressed from the image's first sample, like d_img.
hipError_t launch_display_apply(const uint16_t* d_img, size_t s0, size_t s1, const uint8_t* d_lut, uint8_t* d_out, hipStream_t st) {
    if (s1 <= s0) return hipSuccess;
    if (((uintptr_t)d_img & 15) || ((uintptr_t)d_out & 7)) return hipErrorInvalidValue;
    const size_t groups = (s1 + kGroup - 1) / kGroup - s0 / kGroup;
    hipLaunchKernelGGL(display_apply_kernel, dim3((unsigned)stride_grid(groups, 8192, GF_DISPLAY)), dim3(256), 0, st, d_img, s0, s1, d_lut, d_out);
    return hipGetLastError();
}

}  // namespace s2sr
