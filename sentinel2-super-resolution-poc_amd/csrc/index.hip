// Normalised-difference indices on the SR grid: one streaming pass over two uint16 planes that gives the int16 index
// raster, its RGBA rendering, its exact histogram and exact per-zone sums, each optional; and the rendering alone for an index
// raster that already exists.  The policy around it -- which bands, the colour ramp, statistics from the histogram -- is Python
// (s2sr/index.py).
//
// Definition (integers; tests/index_model.py restates it in numpy):
//   a' = max(a - offset, 0), b' = max(b - offset, 0), n = a' - b', d = a' + b' + L
//   v  = sign(n) floor((2 |n| K + d) / (2 d))   for d > 0: round half away from zero, |v| <= K <= 16383
//   v  = -32768 (nodata)                        for d == 0, and for a pixel whose mask cell valid[y / vs][x / vs] is 0
//   2 |n| K + d <= 2 * 65535 * 16383 + 196605 < 2^32 and 2 d < 2^19: unsigned 32-bit arithmetic.
//   undefined   the unmasked pixels with d == 0
//   hist        hist[v + K] = the defined pixels of value v (uint64 [2 K + 1], added to)
//   rgba        lut[(uint16)(v + 32768)], lut = uint8 [65536][4]; nodata: 0, 0, 0, 0 whatever the LUT holds
//   zonal       int64 [Z + 1][3]: count, sum v, sum v^2 of the defined pixels of label zones[y / zs][x / zs]; row 0: label 0 and
//               labels above Z (added to)
//
// Both kernels work on the flat pixels [p0, p1) of the image (a band of whole rows) in groups of 8 pixels counted from the image's
// first pixel: one 16-byte load per lane from a 1-channel plane, three from an interleaved 3-channel one (the channel is picked in
// registers), one 16-byte store of the index and two of the RGBA.  Every base is 16-byte aligned and readable up to the next
// multiple of 16 bytes behind its last sample; a vector wholly outside the band is not loaded, samples outside it are ignored, and
// a group at the band's edge stores sample by sample.  A pixel's mask and zone cells come from its row and column, found by one
// division per group and stepped from there.
//
// Histogram.  2 K + 1 counters of 32 bits are at most 131 KB: one workgroup's copy fits the 160 KB of LDS, so the planes are read
// once (display.hip needs value ranges and eight reads).  1024 threads, one workgroup per CU, LDS atomics; where every active lane
// of a wave holds one value (a field of constant index: the common case) one lane adds the wave's count.  At its end a workgroup
// adds its non-zero counters to the uint64 global histogram.  A band holds fewer than 2^31 pixels, so no LDS counter overflows.
//
// Zonal sums.  A lane sums its 8 pixels while the label stays (a change inside the group goes to memory at once: one lane per
// border crossing).  The wave then takes one turn per label its lanes hold -- one inside a field, two where it straddles a border
// -- reducing that label's sums across the lanes.  The first label of a turn goes to the wave's pending sums, kept in registers
// until the label changes or the kernel ends; a further label leaves as one lane's three 64-bit atomics.  At the kernel's end the
// 16 waves' pending sums meet in LDS and neighbours with one label leave as one add: the pixels without a zone and the inside of a
// field cost three atomics per workgroup and launch.  (Per-lane adds at the borders, the first version, cost 9 ms on a 16384^2
// image with 64-pixel zone cells: profiles/index_bench_line.json has the figure of this one.)  Integer adds: no order changes them.
#include "s2sr_internal.h"

namespace s2sr {

namespace {

constexpr int kThreads = 1024;
constexpr int kPx = 8;                                          // pixels per lane and step
constexpr int kMaxBins = 2 * 16383 + 1;
constexpr int kMaxLds = (kMaxBins * 4 + 15) & ~15;              // 131,072 B

struct IndexArgs {
    const uint16_t* a;
    const uint16_t* b;
    int32_t ac, ca, bc, cb;
    uint32_t W, p0, p1;
    int32_t offset;
    uint32_t L, K;
    const uint8_t* valid;
    uint32_t vs, vw;
    const uint16_t* zones;
    uint32_t zs, zw, Z;
    const uint32_t* lut;
    int16_t* out;
    uint32_t* rgba;
    unsigned long long* hist;
    unsigned long long* zonal;
    unsigned long long* undefined;
};

__device__ __forceinline__ void unpack8(const uint4& q, uint32_t* v) {
    v[0] = q.x & 0xffffu; v[1] = q.x >> 16; v[2] = q.y & 0xffffu; v[3] = q.y >> 16;
    v[4] = q.z & 0xffffu; v[5] = q.z >> 16; v[6] = q.w & 0xffffu; v[7] = q.w >> 16;
}

// the 8 samples of channel ch of pixels [8 g, 8 g + 8) of a plane with c (1 or 3) channels per pixel
__device__ __forceinline__ void load_plane(const uint16_t* __restrict__ p, int c, int ch, uint32_t g, uint32_t p0, uint32_t p1, uint32_t* s) {
    if (c == 1) {
        unpack8(*(const uint4*)(p + (size_t)g * kPx), s);
        return;
    }
    uint32_t t[24];
    const size_t s0 = (size_t)p0 * 3, s1 = (size_t)p1 * 3;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const size_t vb = (size_t)g * 24 + 8 * v;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (vb + 8 > s0 && vb < s1) q = *(const uint4*)(p + vb);
        unpack8(q, t + 8 * v);
    }
#pragma unroll
    for (int j = 0; j < kPx; ++j) s[j] = ch == 0 ? t[3 * j] : ch == 1 ? t[3 * j + 1] : t[3 * j + 2];
}

// row / column cell of a pixel in a grid of `scale` pixels per cell, stepped pixel by pixel along the flat order
struct Cell {
    uint32_t xq, xr, yq, yr;
    __device__ __forceinline__ void at(uint32_t y, uint32_t x, uint32_t scale) {
        xq = x / scale; xr = x - xq * scale;
        yq = y / scale; yr = y - yq * scale;
    }
    __device__ __forceinline__ void step(bool wrap, uint32_t scale) {
        if (wrap) {
            xq = 0; xr = 0;
            if (++yr == scale) { yr = 0; ++yq; }
        } else if (++xr == scale) {
            xr = 0; ++xq;
        }
    }
};

__device__ __forceinline__ void zonal_add(unsigned long long* zonal, uint32_t label, long long cnt, long long s, long long s2) {
    unsigned long long* z = zonal + (size_t)label * 3;
    atomicAdd(z, (unsigned long long)cnt);
    atomicAdd(z + 1, (unsigned long long)s);
    atomicAdd(z + 2, (unsigned long long)s2);
}

template <bool HIST, bool ZONAL>
__global__ void __launch_bounds__(kThreads, 1) index_nd_kernel(const IndexArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bins[];   // [2 K + 1] (HIST)
    __shared__ uint32_t undef_wg;
    const uint32_t nbins = 2 * p.K + 1;
    if (HIST)
        for (uint32_t i = threadIdx.x; i < nbins; i += kThreads) bins[i] = 0;
    if (threadIdx.x == 0) undef_wg = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t g0 = p.p0 / kPx, g1 = (p.p1 + kPx - 1) / kPx;
    const bool cells = p.valid || ZONAL;
    uint32_t undef = 0;
    uint32_t wlabel = 0;                          // the wave's pending sums (the same in every lane)
    long long wcnt = 0, ws = 0, ws2 = 0;
    // base is the same in every lane of the workgroup: the wave-wide steps below run with all lanes
    for (uint32_t base = g0 + blockIdx.x * kThreads; base < g1; base += gridDim.x * kThreads) {
        const uint32_t g = base + threadIdx.x;
        uint32_t cur = 0, lc = 0, ls2 = 0;        // the lane's sums of this group (ZONAL)
        int32_t ls = 0;
        if (g < g1) {
            uint32_t sa[kPx], sb[kPx];
            load_plane(p.a, p.ac, p.ca, g, p.p0, p.p1, sa);
            load_plane(p.b, p.bc, p.cb, g, p.p0, p.p1, sb);
            const uint32_t pix = g * kPx;
            uint32_t x = 0;
            Cell cv{0, 0, 0, 0}, cz{0, 0, 0, 0};
            if (cells) {
                const uint32_t y = pix / p.W;
                x = pix - y * p.W;
                if (p.valid) cv.at(y, x, p.vs);
                if (ZONAL) cz.at(y, x, p.zs);
            }
            int32_t val[kPx];
            uint32_t col[kPx];
#pragma unroll
            for (int j = 0; j < kPx; ++j) {
                const bool in = pix + j >= p.p0 && pix + j < p.p1;
                bool nod = true;
                int32_t v = -32768;
                if (in) {
                    const bool masked = p.valid && p.valid[(size_t)cv.yq * p.vw + cv.xq] == 0;
                    const int32_t a1 = max((int32_t)sa[j] - p.offset, 0), b1 = max((int32_t)sb[j] - p.offset, 0);
                    const int32_t n = a1 - b1;
                    const uint32_t d = (uint32_t)(a1 + b1) + p.L;
                    if (!masked && d == 0) ++undef;
                    if (!masked && d != 0) {
                        const uint32_t q = (2u * (uint32_t)abs(n) * p.K + d) / (2u * d);
                        v = n < 0 ? -(int32_t)q : (int32_t)q;
                        nod = false;
                    }
                }
                val[j] = v;
                col[j] = 0;
                if (!nod) {
                    if (p.rgba) col[j] = p.lut[(uint32_t)(v + 32768)];
                    if (HIST) {
                        const uint32_t bin = (uint32_t)(v + (int32_t)p.K);
                        const uint32_t first = __builtin_amdgcn_readfirstlane(bin);
                        const unsigned long long active = __ballot(1), same = __ballot(bin == first);
                        if (same == active) {   // one value in the whole wave: one add of the wave's count
                            if (lane == __ffsll((long long)active) - 1) atomicAdd(&bins[bin], (uint32_t)__popcll(active));
                        } else {
                            atomicAdd(&bins[bin], 1u);
                        }
                    }
                    if (ZONAL) {
                        uint32_t label = p.zones[(size_t)cz.yq * p.zw + cz.xq];
                        if (label > p.Z) label = 0;
                        if (lc && label != cur) {             // a zone border inside the group
                            zonal_add(p.zonal, cur, lc, ls, ls2);
                            lc = 0; ls = 0; ls2 = 0;
                        }
                        cur = label;
                        ++lc; ls += v; ls2 += (uint32_t)(v * v);
                    }
                }
                if (cells) {
                    const bool wrap = ++x == p.W;
                    if (wrap) x = 0;
                    if (p.valid) cv.step(wrap, p.vs);
                    if (ZONAL) cz.step(wrap, p.zs);
                }
            }
            const bool whole = pix >= p.p0 && pix + kPx <= p.p1;
            if (p.out) {
                if (whole) {
                    uint4 w;
                    w.x = (uint32_t)(val[0] & 0xffff) | ((uint32_t)val[1] << 16);
                    w.y = (uint32_t)(val[2] & 0xffff) | ((uint32_t)val[3] << 16);
                    w.z = (uint32_t)(val[4] & 0xffff) | ((uint32_t)val[5] << 16);
                    w.w = (uint32_t)(val[6] & 0xffff) | ((uint32_t)val[7] << 16);
                    *(uint4*)(p.out + (size_t)pix) = w;
                } else {
#pragma unroll
                    for (int j = 0; j < kPx; ++j)
                        if (pix + j >= p.p0 && pix + j < p.p1) p.out[(size_t)pix + j] = (int16_t)val[j];
                }
            }
            if (p.rgba) {
                if (whole) {
                    *(uint4*)(p.rgba + (size_t)pix) = make_uint4(col[0], col[1], col[2], col[3]);
                    *(uint4*)(p.rgba + (size_t)pix + 4) = make_uint4(col[4], col[5], col[6], col[7]);
                } else {
#pragma unroll
                    for (int j = 0; j < kPx; ++j)
                        if (pix + j >= p.p0 && pix + j < p.p1) p.rgba[(size_t)pix + j] = col[j];
                }
            }
        }
        if (ZONAL) {   // all lanes of the wave are here
            const bool has = lc > 0;
            unsigned long long todo = __ballot(has);
            bool first = true;
            while (todo) {   // one turn per label the wave holds: one inside a field, two where it straddles a border
                const uint32_t l0 = (uint32_t)__shfl((int)cur, __ffsll((long long)todo) - 1);
                const bool mine = has && cur == l0;
                int32_t rc = mine ? (int32_t)lc : 0, rs = mine ? ls : 0;
                long long r2 = mine ? (long long)ls2 : 0;
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) {
                    rc += __shfl_xor(rc, m);
                    rs += __shfl_xor(rs, m);
                    r2 += __shfl_xor(r2, m);
                }
                if (l0 == wlabel || first) {     // the wave's pending sums follow the first label of the turn
                    if (l0 != wlabel) {
                        if (lane == 0 && wcnt) zonal_add(p.zonal, wlabel, wcnt, ws, ws2);
                        wlabel = l0; wcnt = 0; ws = 0; ws2 = 0;
                    }
                    wcnt += rc; ws += rs; ws2 += r2;
                } else if (lane == 0) {
                    zonal_add(p.zonal, l0, rc, rs, r2);
                }
                first = false;
                todo &= ~__ballot(mine);
            }
        }
    }
    if (ZONAL) {   // the waves' pending sums meet in LDS: neighbours that hold one label leave as one add
        __shared__ uint32_t zl[kThreads / 64];
        __shared__ long long zc[kThreads / 64], zs[kThreads / 64], zq[kThreads / 64];
        if (lane == 0) {
            const int w = threadIdx.x >> 6;
            zl[w] = wlabel; zc[w] = wcnt; zs[w] = ws; zq[w] = ws2;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t l = zl[0];
            long long c = zc[0], s = zs[0], q = zq[0];
            for (int w = 1; w < kThreads / 64; ++w) {
                if (zl[w] != l) {
                    if (c) zonal_add(p.zonal, l, c, s, q);
                    l = zl[w]; c = 0; s = 0; q = 0;
                }
                c += zc[w]; s += zs[w]; q += zq[w];
            }
            if (c) zonal_add(p.zonal, l, c, s, q);
        }
    }
    if (undef) atomicAdd(&undef_wg, undef);
    __syncthreads();
    if (threadIdx.x == 0 && undef_wg && p.undefined) atomicAdd(p.undefined, (unsigned long long)undef_wg);
    if (HIST)
        for (uint32_t i = threadIdx.x; i < nbins; i += kThreads) {
            const uint32_t n = bins[i];
            if (n) atomicAdd(&p.hist[i], (unsigned long long)n);
        }
}

// one lane: 8 index samples through the LUT -> 32 contiguous bytes
__global__ void __launch_bounds__(256) index_render_kernel(const int16_t* __restrict__ idx, uint32_t p0, uint32_t p1, const uint32_t* __restrict__ lut,
                                                           uint32_t* __restrict__ rgba) {
    const uint32_t g0 = p0 / kPx, g1 = (p1 + kPx - 1) / kPx;
    for (uint32_t g = g0 + blockIdx.x * blockDim.x + threadIdx.x; g < g1; g += gridDim.x * blockDim.x) {
        const uint32_t pix = g * kPx;
        uint32_t s[kPx], col[kPx];
        unpack8(*(const uint4*)(idx + (size_t)pix), s);
#pragma unroll
        for (int j = 0; j < kPx; ++j) col[j] = s[j] == 0x8000u ? 0u : lut[s[j] ^ 0x8000u];      // (uint16)(v + 32768)
        if (pix >= p0 && pix + kPx <= p1) {
            *(uint4*)(rgba + (size_t)pix) = make_uint4(col[0], col[1], col[2], col[3]);
            *(uint4*)(rgba + (size_t)pix + 4) = make_uint4(col[4], col[5], col[6], col[7]);
        } else {
#pragma unroll
            for (int j = 0; j < kPx; ++j)
                if (pix + j >= p0 && pix + j < p1) rgba[(size_t)pix + j] = col[j];
        }
    }
}

template <bool HIST, bool ZONAL>
hipError_t launch_form(const IndexArgs& a, hipStream_t st) {
    static KernelLaunchState state;
    int ncu = 256;
    hipError_t e = state.prepare((const void*)index_nd_kernel<HIST, ZONAL>, kMaxLds, &ncu);
    if (e != hipSuccess) return e;
    const uint32_t groups = (a.p1 + kPx - 1) / kPx - a.p0 / kPx;
    const long long blocks = ((long long)groups + kThreads - 1) / kThreads;
    // with the histogram in LDS one workgroup fills a CU; without it two of them do
    const long long most = HIST ? ncu : 2 * ncu;
    const int grid = capped_grid((int)(blocks < most ? blocks : most), blocks, GF_DISPLAY);
    const size_t lds = HIST ? ((size_t)(2 * a.K + 1) * 4 + 15) & ~(size_t)15 : 0;
    hipLaunchKernelGGL((index_nd_kernel<HIST, ZONAL>), dim3((unsigned)grid), dim3(kThreads), lds, st, a);
    return hipGetLastError();
}

bool plane_ok(const void* p, int c, int ch) { return p && ((uintptr_t)p & 15) == 0 && (c == 1 || c == 3) && ch >= 0 && ch < c; }

}  // namespace

hipError_t launch_index_nd(const uint16_t* d_a, int ac, int ca, const uint16_t* d_b, int bc, int cb, int H, int W, int y0, int y1, int offset,
                           int L, int K, const uint8_t* d_valid, int vs, const uint16_t* d_zones, int zs, int Z, const uint8_t* d_lut,
                           int16_t* d_out, unsigned long long* d_hist, unsigned long long* d_zonal, uint8_t* d_rgba,
                           unsigned long long* d_undefined, hipStream_t st) {
    if (!plane_ok(d_a, ac, ca) || !plane_ok(d_b, bc, cb) || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || y0 < 0 || y0 >= y1 || y1 > H ||
        offset < 0 || offset > 65535 || L < 0 || L > 65535 || K < 1 || K > 16383 || (d_valid && vs < 1) || (d_zones && (zs < 1 || Z < 1 || Z > 65535)) ||
        (d_zonal != nullptr) != (d_zones != nullptr) || (d_rgba && !d_lut) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_rgba & 15) ||
        ((uintptr_t)d_lut & 3) || ((uintptr_t)d_hist & 7) || ((uintptr_t)d_zonal & 7) || ((uintptr_t)d_undefined & 7))
        return hipErrorInvalidValue;
    IndexArgs a{};
    a.a = d_a; a.b = d_b; a.ac = ac; a.ca = ca; a.bc = bc; a.cb = cb;
    a.W = (uint32_t)W; a.p0 = (uint32_t)y0 * (uint32_t)W; a.p1 = (uint32_t)y1 * (uint32_t)W;
    a.offset = offset; a.L = (uint32_t)L; a.K = (uint32_t)K;
    a.valid = d_valid; a.vs = d_valid ? (uint32_t)vs : 1; a.vw = (a.W + a.vs - 1) / a.vs;
    a.zones = d_zones; a.zs = d_zones ? (uint32_t)zs : 1; a.zw = (a.W + a.zs - 1) / a.zs; a.Z = (uint32_t)Z;
    a.lut = (const uint32_t*)d_lut; a.out = d_out; a.rgba = (uint32_t*)d_rgba; a.hist = d_hist; a.zonal = d_zonal; a.undefined = d_undefined;
    if (d_hist) return d_zones ? launch_form<true, true>(a, st) : launch_form<true, false>(a, st);
    return d_zones ? launch_form<false, true>(a, st) : launch_form<false, false>(a, st);
}

hipError_t launch_index_render(const int16_t* d_idx, int H, int W, int y0, int y1, const uint8_t* d_lut, uint8_t* d_rgba, hipStream_t st) {
    if (!d_idx || !d_lut || !d_rgba || ((uintptr_t)d_idx & 15) || ((uintptr_t)d_rgba & 15) || ((uintptr_t)d_lut & 3) || H <= 0 || W <= 0 ||
        (long long)H * W > 0x7fffffffLL || y0 < 0 || y0 >= y1 || y1 > H)
        return hipErrorInvalidValue;
    const uint32_t p0 = (uint32_t)y0 * (uint32_t)W, p1 = (uint32_t)y1 * (uint32_t)W;
    const size_t groups = (p1 + kPx - 1) / kPx - p0 / kPx;
    hipLaunchKernelGGL(index_render_kernel, dim3((unsigned)stride_grid(groups, 8192, GF_DISPLAY)), dim3(256), 0, st, d_idx, p0, p1,
                       (const uint32_t*)d_lut, (uint32_t*)d_rgba);
    return hipGetLastError();
}

}  // namespace s2sr
