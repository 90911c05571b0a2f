// Management zones: integer k-means inside every field.  D int16 index rasters and a uint16 label raster -> a uint8
// zone raster, per (field, zone) sums, the final centres, a status per field and the number of iterations.  The host side is
// engine_mzones.hip; the policy -- index units, class names, hectares, GeoJSON -- is Python (s2sr/mzones.py).
//
// Definition (integers; tests/mzones_model.py restates it in numpy; include/s2sr.h has it in full):
//   member      label l in 1..Z and none of the D values is -32768; everything else is zone 0 and counted nowhere
//   statistics  n_l, lo_d, hi_d over the members; n_l == 0: absent (status 0); n_l < k min_per_zone: skipped (1); else zoned (2)
//   start       c[j][d] = lo_d + ((2 j + 1)(hi_d - lo_d)) / (2 k)
//   iteration   a member goes to the smallest j of the smallest sum_d (v_d - c[j][d])^2; per (field, j) n and s_d in int64; a
//               cluster with n > 0 moves to sign(s_d) ((2 |s_d| + n) / (2 n)), an empty one stays
//   zones       once more to the final centres; zone id = 1 + rank of (c[j][0], j)
//   smoothing   the 3 x 3 mode among the neighbours of the same label and zone > 0, ties to the own id, then the smallest
//   table       per (field, zone): pixels, then per feature sum v_d, sum v_d^2, from the final raster
//
// Why the bytes depend on nothing but the inputs: every sum is an integer add, every statistic an integer min or max, and a centre
// is a function of the finished sums, so neither the order of the atomics, nor the row bands, nor the number of workgroups shows.
// One term of a distance is at most 65534^2 < 2^32, the sum of four below 2^34: uint32 for D = 1, uint64 beyond.  A lane's sums over
// its 8 pixels, a wave's over its 512 and the wave's pending sums (let go before 65000 pixels are in them: 65000 * 32767 < 2^31) fit
// int32; squares travel in 64 bits.
//
// The pixel passes with sums (statistics, assign-and-accumulate, table) share one walk.  The band is cut into tiles of 64 pixels by
// 32 rows; a workgroup of 256 threads takes a tile a turn, a lane one group of 8 pixels (16-byte loads of labels and features where
// W is a multiple of 8), so a wave holds 8 rows of 64 pixels.  The tiles are numbered column by column and a workgroup takes a
// contiguous run of them: it walks DOWN a strip of 64 pixels, and fields are spatially coherent, so the label of one turn is most
// often the label of the next.  A lane sums while the label stays and fetches a field's k D centres once per run of equal labels (a
// change inside the group goes to memory at once: one lane per border crossing).  The wave then takes one turn per label its lanes
// hold, reducing that label's sums across the lanes; the first label of a turn joins the wave's pending sums, which stay in
// registers until the label changes, a further label leaves as one lane's 64-bit atomics.  The inside of a field costs a handful of
// atomics per wave and launch, not per pixel (index.hip measured the difference for its zonal sums: 9 ms against 0.4 ms).
// No workgroup waits for another; order comes from the stream.
#include "s2sr_internal.h"

namespace s2sr {

namespace {

constexpr int kTileW = 64, kTileH = 32, kPx = 8;
constexpr int kMostBlocks = 2048;                                // 256 CUs x 8 workgroups of 256
constexpr int kNoData = -32768;
constexpr uint32_t kPendingMost = 65000 - kTileW * kTileH / 4;    // pixels in a wave's pending sums before its turn's 512 join them

struct Walk {
    uint32_t W, y0, y1, tiles_y, ntiles;
    int vec;
};

// the lane's group of tile t: its row, its first column and how many of its 8 pixels exist (0: none)
__device__ __forceinline__ uint32_t lane_group(const Walk& g, uint32_t t, uint32_t* y, uint32_t* xs) {
    const uint32_t tx = t / g.tiles_y, ty = t - tx * g.tiles_y;
    *y = g.y0 + ty * kTileH + (threadIdx.x >> 3);
    *xs = tx * kTileW + (threadIdx.x & 7) * kPx;
    if (*y >= g.y1 || *xs >= g.W) return 0;
    return g.W - *xs < (uint32_t)kPx ? g.W - *xs : (uint32_t)kPx;
}
// the workgroup's run of tiles
__device__ __forceinline__ void block_run(const Walk& g, uint32_t* t0, uint32_t* t1) {
    const uint32_t per = (g.ntiles + gridDim.x - 1) / gridDim.x;
    const unsigned long long a = (unsigned long long)blockIdx.x * per, b = a + per;
    *t0 = a < g.ntiles ? (uint32_t)a : g.ntiles;
    *t1 = b < g.ntiles ? (uint32_t)b : g.ntiles;
}

__device__ __forceinline__ void load8_u16(const uint16_t* __restrict__ p, size_t base, uint32_t n, int vec, uint32_t* v) {
    if (vec) {
        const uint4 q = *(const uint4*)(p + base);
        v[0] = q.x & 0xffffu; v[1] = q.x >> 16; v[2] = q.y & 0xffffu; v[3] = q.y >> 16;
        v[4] = q.z & 0xffffu; v[5] = q.z >> 16; v[6] = q.w & 0xffffu; v[7] = q.w >> 16;
    } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j) v[j] = (uint32_t)j < n ? p[base + j] : 0u;
    }
}
__device__ __forceinline__ void load8_i16(const int16_t* __restrict__ p, size_t base, uint32_t n, int vec, int* v) {
    uint32_t u[kPx];
    load8_u16((const uint16_t*)p, base, n, vec, u);
#pragma unroll
    for (int j = 0; j < kPx; ++j) v[j] = (int)(int16_t)u[j];
}
__device__ __forceinline__ void load8_u8(const uint8_t* __restrict__ p, size_t base, uint32_t n, int vec, uint32_t* v) {
    if (vec) {
        const uint2 q = *(const uint2*)(p + base);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = (q.x >> (8 * j)) & 255u;
            v[4 + j] = (q.y >> (8 * j)) & 255u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j) v[j] = (uint32_t)j < n ? p[base + j] : 0u;
    }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
    return v;
}

// ---- field statistics ------------------------------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void stats_out(uint32_t* cnt, int* lo, int* hi, uint32_t l, uint32_t c, const int* a, const int* b) {
    atomicAdd(cnt + l, c);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        atomicMin(lo + (size_t)l * D + d, a[d]);
        atomicMax(hi + (size_t)l * D + d, b[d]);
    }
}

template <int D>
__global__ void __launch_bounds__(256) mz_stats_kernel(const int16_t* __restrict__ feat, size_t plane, const uint16_t* __restrict__ labels, const Walk g,
                                                       uint32_t Z, uint32_t* __restrict__ cnt, int* __restrict__ lo, int* __restrict__ hi) {
    const int lane = threadIdx.x & 63;
    uint32_t wlabel = 0, wc = 0;                                 // the wave's pending statistics (the same in every lane)
    int wlo[D], whi[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { wlo[d] = 0x7fffffff; whi[d] = -0x7fffffff - 1; }
    uint32_t t0, t1;
    block_run(g, &t0, &t1);
    for (uint32_t t = t0; t < t1; ++t) {                         // t is the same in every lane of the workgroup
        uint32_t y, xs, cur = 0, lc = 0;
        int llo[D], lhi[D];
#pragma unroll
        for (int d = 0; d < D; ++d) { llo[d] = 0x7fffffff; lhi[d] = -0x7fffffff - 1; }
        const uint32_t n = lane_group(g, t, &y, &xs);
        if (n) {
            const size_t base = (size_t)y * g.W + xs;
            uint32_t lab[kPx];
            int v[D][kPx];
            load8_u16(labels, base, n, g.vec, lab);
#pragma unroll
            for (int d = 0; d < D; ++d) load8_i16(feat + (size_t)d * plane, base, n, g.vec, v[d]);
#pragma unroll
            for (int j = 0; j < kPx; ++j) {
                const uint32_t l = lab[j] > Z ? 0u : lab[j];
                bool member = (uint32_t)j < n && l != 0;
#pragma unroll
                for (int d = 0; d < D; ++d) member = member && v[d][j] != kNoData;
                if (!member) continue;
                if (l != cur) {
                    if (lc) stats_out<D>(cnt, lo, hi, cur, lc, llo, lhi);
                    cur = l; lc = 0;
#pragma unroll
                    for (int d = 0; d < D; ++d) { llo[d] = 0x7fffffff; lhi[d] = -0x7fffffff - 1; }
                }
                ++lc;
#pragma unroll
                for (int d = 0; d < D; ++d) { llo[d] = min(llo[d], v[d][j]); lhi[d] = max(lhi[d], v[d][j]); }
            }
        }
        unsigned long long todo = __ballot(lc > 0);
        bool first = true;
        while (todo) {                                           // one turn per label the wave holds
            const uint32_t l0 = (uint32_t)__shfl((int)cur, __ffsll((long long)todo) - 1);
            const bool mine = lc > 0 && cur == l0;
            const uint32_t rc = (uint32_t)wave_sum(mine ? (int)lc : 0);
            int rlo[D], rhi[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                rlo[d] = wave_min(mine ? llo[d] : 0x7fffffff);
                rhi[d] = wave_max(mine ? lhi[d] : -0x7fffffff - 1);
            }
            if (l0 == wlabel || first) {
                if (l0 != wlabel) {
                    if (lane == 0 && wc) stats_out<D>(cnt, lo, hi, wlabel, wc, wlo, whi);
                    wlabel = l0; wc = 0;
#pragma unroll
                    for (int d = 0; d < D; ++d) { wlo[d] = 0x7fffffff; whi[d] = -0x7fffffff - 1; }
                }
                wc += rc;
#pragma unroll
                for (int d = 0; d < D; ++d) { wlo[d] = min(wlo[d], rlo[d]); whi[d] = max(whi[d], rhi[d]); }
            } else if (lane == 0) {
                stats_out<D>(cnt, lo, hi, l0, rc, rlo, rhi);
            }
            first = false;
            todo &= ~__ballot(mine);
        }
    }
    if (lane == 0 && wc) stats_out<D>(cnt, lo, hi, wlabel, wc, wlo, whi);
}

// ---- the tables: one thread per field, or per (field, cluster) ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) mz_clear_kernel(uint32_t* __restrict__ cnt, int* __restrict__ lo, int* __restrict__ hi, size_t fields, int D) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < fields; i += (size_t)gridDim.x * 256) {
        cnt[i] = 0;
        for (int d = 0; d < D; ++d) { lo[i * D + d] = 0x7fffffff; hi[i * D + d] = -0x7fffffff - 1; }
    }
}

// status and the start centres; row 0 is no field
__global__ void __launch_bounds__(256) mz_start_kernel(const uint32_t* __restrict__ cnt, const int* __restrict__ lo, const int* __restrict__ hi, size_t fields,
                                                       int k, int D, long long least, uint8_t* __restrict__ status, int* __restrict__ centres) {
    const size_t items = fields * (size_t)k;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const size_t l = i / (size_t)k;
        const int j = (int)(i - l * (size_t)k);
        const uint32_t n = l ? cnt[l] : 0u;
        const int st = n == 0 ? 0 : (long long)n < least ? 1 : 2;
        if (j == 0) status[l] = (uint8_t)st;
        for (int d = 0; d < D; ++d) {
            int c = 0;
            if (st == 2) {
                const int a = lo[l * D + d], b = hi[l * D + d];
                c = a + ((2 * j + 1) * (b - a)) / (2 * k);         // (2 j + 1)(b - a) <= 15 * 65534
            }
            centres[i * D + d] = c;
        }
    }
}

// the sums of one iteration become the centres; the sums are left at zero for the next.  *changed: any centre moved
__global__ void __launch_bounds__(256) mz_update_kernel(unsigned long long* __restrict__ acc, size_t fields, int k, int D, const uint8_t* __restrict__ status,
                                                        int* __restrict__ centres, uint32_t* __restrict__ changed) {
    const size_t items = fields * (size_t)k;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        if (status[i / (size_t)k] != 2) continue;
        unsigned long long* row = acc + i * (size_t)(1 + D);
        const long long n = (long long)row[0];
        if (n == 0) continue;                                    // an empty cluster keeps its centre (and its sums are zero)
        row[0] = 0;
        bool moved = false;
        for (int d = 0; d < D; ++d) {
            const long long s = (long long)row[1 + d];
            row[1 + d] = 0;
            const long long a = s < 0 ? -s : s, q = (2 * a + n) / (2 * n);
            const int c = (int)(s < 0 ? -q : q);
            moved = moved || c != centres[i * D + d];
            centres[i * D + d] = c;
        }
        if (moved) atomicOr(changed, 1u);
    }
}

// zone id = 1 + rank of (c[j][0], j); the centres in rank order
__global__ void __launch_bounds__(256) mz_rank_kernel(const int* __restrict__ centres, size_t fields, int k, int D, const uint8_t* __restrict__ status,
                                                      uint8_t* __restrict__ zone_of, int* __restrict__ ranked) {
    const size_t items = fields * (size_t)k;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const size_t l = i / (size_t)k;
        const int j = (int)(i - l * (size_t)k);
        if (status[l] != 2) {
            zone_of[i] = 0;
            for (int d = 0; d < D; ++d) ranked[i * D + d] = 0;
            continue;
        }
        const int mine = centres[i * D];
        int rank = 0;
        for (int o = 0; o < k; ++o) {
            const int c = centres[(l * k + o) * D];
            rank += c < mine || (c == mine && o < j);
        }
        zone_of[i] = (uint8_t)(1 + rank);
        for (int d = 0; d < D; ++d) ranked[(l * k + rank) * D + d] = centres[i * D + d];
    }
}

// ---- assign ---------------------------------------------------------------------------------------------------------------------------
template <int D, int KM>
__device__ __forceinline__ void fetch_centres(const int* __restrict__ centres, uint32_t l, int k, int* c) {
#pragma unroll
    for (int j = 0; j < KM; ++j)
#pragma unroll
        for (int d = 0; d < D; ++d) c[j * D + d] = j < k ? centres[((size_t)l * k + j) * D + d] : 0;
}
// the smallest j of the smallest distance
template <int D, int KM>
__device__ __forceinline__ int nearest(const int* c, int k, const int* v) {
    int best = 0;
    if (D == 1) {
        const int e = v[0] - c[0];
        uint32_t bd = (uint32_t)e * (uint32_t)e;                 // |e| <= 65534: the square is below 2^32
#pragma unroll
        for (int j = 1; j < KM; ++j) {
            const int f = v[0] - c[j];
            const uint32_t dj = (uint32_t)f * (uint32_t)f;
            if (j < k && dj < bd) { bd = dj; best = j; }
        }
    } else {
        unsigned long long bd = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int e = v[d] - c[d];
            bd += (uint32_t)e * (uint32_t)e;
        }
#pragma unroll
        for (int j = 1; j < KM; ++j) {
            unsigned long long dj = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int f = v[d] - c[j * D + d];
                dj += (uint32_t)f * (uint32_t)f;
            }
            if (j < k && dj < bd) { bd = dj; best = j; }
        }
    }
    return best;
}

struct SumArgs {
    const int16_t* feat;
    size_t plane;
    const uint16_t* labels;
    const uint8_t* zone;                                         // TABLE: the cluster is the raster's id - 1
    Walk g;
    uint32_t Z;
    int k;
    const int* centres;
    const uint8_t* status;
    unsigned long long* acc;                                     // [Z + 1][k][1 + D]: n, s_d; TABLE: [Z + 1][k][1 + 2 D]: n, then s_d, q_d per feature
};

template <int D, int KM, bool TABLE>
__device__ __forceinline__ void sums_out(unsigned long long* acc, uint32_t l, int k, const int* n, const int* s, const long long* q) {
#pragma unroll
    for (int j = 0; j < KM; ++j) {
        if (j >= k || n[j] == 0) continue;
        unsigned long long* row = acc + ((size_t)l * k + j) * (TABLE ? 1 + 2 * D : 1 + D);
        atomicAdd(row, (unsigned long long)n[j]);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if constexpr (TABLE) {
                atomicAdd(row + 1 + 2 * d, (unsigned long long)(long long)s[j * D + d]);
                atomicAdd(row + 2 + 2 * d, (unsigned long long)q[j * D + d]);
            } else {
                atomicAdd(row + 1 + d, (unsigned long long)(long long)s[j * D + d]);
            }
        }
    }
}

// Assign and accumulate (TABLE false: the hot kernel, once per iteration), and the table pass (TABLE true).
template <int D, int KM, bool TABLE>
__global__ void __launch_bounds__(256) mz_sums_kernel(const SumArgs p) {
    constexpr int Q = TABLE ? KM * D : 1;
    const int lane = threadIdx.x & 63;
    const int k = p.k;
    uint32_t wlabel = 0, wtot = 0;                               // the wave's pending sums (the same in every lane)
    int wn[KM], ws[KM * D];
    long long wq[Q];
#pragma unroll
    for (int j = 0; j < KM; ++j) wn[j] = 0;
#pragma unroll
    for (int i = 0; i < KM * D; ++i) ws[i] = 0;
#pragma unroll
    for (int i = 0; i < Q; ++i) wq[i] = 0;
    uint32_t t0, t1;
    block_run(p.g, &t0, &t1);
    for (uint32_t t = t0; t < t1; ++t) {                         // t is the same in every lane of the workgroup
        uint32_t y, xs, cur = 0, lc = 0;
        int ln[KM], ls[KM * D];
        long long lq[Q];
#pragma unroll
        for (int j = 0; j < KM; ++j) ln[j] = 0;
#pragma unroll
        for (int i = 0; i < KM * D; ++i) ls[i] = 0;
#pragma unroll
        for (int i = 0; i < Q; ++i) lq[i] = 0;
        const uint32_t n = lane_group(p.g, t, &y, &xs);
        if (n) {
            const size_t base = (size_t)y * p.g.W + xs;
            uint32_t lab[kPx], zid[kPx];
            int v[D][kPx];
            int c[KM * D];
            bool zoned = false;
            load8_u16(p.labels, base, n, p.g.vec, lab);
            if constexpr (TABLE) load8_u8(p.zone, base, n, p.g.vec, zid);
#pragma unroll
            for (int d = 0; d < D; ++d) load8_i16(p.feat + (size_t)d * p.plane, base, n, p.g.vec, v[d]);
#pragma unroll
            for (int j = 0; j < kPx; ++j) {
                const uint32_t l = lab[j] > p.Z ? 0u : lab[j];
                bool member = (uint32_t)j < n && l != 0;
                int px[D];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    px[d] = v[d][j];
                    member = member && px[d] != kNoData;
                }
                if constexpr (TABLE) member = member && zid[j] >= 1 && zid[j] <= (uint32_t)k;
                if (!member) continue;
                if (l != cur) {
                    if (lc) sums_out<D, KM, TABLE>(p.acc, cur, k, ln, ls, lq);
                    cur = l; lc = 0;
#pragma unroll
                    for (int jj = 0; jj < KM; ++jj) ln[jj] = 0;
#pragma unroll
                    for (int i = 0; i < KM * D; ++i) ls[i] = 0;
#pragma unroll
                    for (int i = 0; i < Q; ++i) lq[i] = 0;
                    if (!TABLE) {                                // a field's centres: once per run of equal labels
                        zoned = p.status[l] == 2;
                        if (zoned) fetch_centres<D, KM>(p.centres, l, k, c);
                    }
                }
                if (!TABLE && !zoned) continue;
                const int best = TABLE ? (int)zid[j] - 1 : nearest<D, KM>(c, k, px);
                ++lc;
#pragma unroll
                for (int jj = 0; jj < KM; ++jj) {
                    const bool m = jj == best;
                    ln[jj] += m;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        ls[jj * D + d] += m ? px[d] : 0;
                        if constexpr (TABLE) lq[jj * D + d] += m ? (long long)(px[d] * px[d]) : 0;
                    }
                }
            }
        }
        unsigned long long todo = __ballot(lc > 0);
        bool first = true;
        while (todo) {                                           // one turn per label the wave holds
            const uint32_t l0 = (uint32_t)__shfl((int)cur, __ffsll((long long)todo) - 1);
            const bool mine = lc > 0 && cur == l0;
            int rn[KM], rs[KM * D];
            long long rq[Q];
#pragma unroll
            for (int j = 0; j < KM; ++j) {
                rn[j] = 0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    rs[j * D + d] = 0;
                    if constexpr (TABLE) rq[j * D + d] = 0;
                }
                if (j >= k) continue;
                rn[j] = wave_sum(mine ? ln[j] : 0);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    rs[j * D + d] = wave_sum(mine ? ls[j * D + d] : 0);
                    if constexpr (TABLE) rq[j * D + d] = wave_sum(mine ? lq[j * D + d] : 0ll);
                }
            }
            if constexpr (!TABLE) rq[0] = 0;
            if (l0 == wlabel || first) {
                if (l0 != wlabel || wtot > kPendingMost) {
                    if (lane == 0 && wtot) sums_out<D, KM, TABLE>(p.acc, wlabel, k, wn, ws, wq);
                    wlabel = l0; wtot = 0;
#pragma unroll
                    for (int j = 0; j < KM; ++j) wn[j] = 0;
#pragma unroll
                    for (int i = 0; i < KM * D; ++i) ws[i] = 0;
#pragma unroll
                    for (int i = 0; i < Q; ++i) wq[i] = 0;
                }
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    wn[j] += rn[j];
                    wtot += (uint32_t)rn[j];
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        ws[j * D + d] += rs[j * D + d];
                        if constexpr (TABLE) wq[j * D + d] += rq[j * D + d];
                    }
                }
            } else if (lane == 0) {
                sums_out<D, KM, TABLE>(p.acc, l0, k, rn, rs, rq);
            }
            first = false;
            todo &= ~__ballot(mine);
        }
    }
    if (lane == 0 && wtot) sums_out<D, KM, TABLE>(p.acc, wlabel, k, wn, ws, wq);
}

// the final assignment: the zone raster through the rank map; one lane a group of 8 pixels of rows [y0, y1)
template <int D>
__global__ void __launch_bounds__(256) mz_assign_kernel(const int16_t* __restrict__ feat, size_t plane, const uint16_t* __restrict__ labels, uint32_t W,
                                                        uint32_t y0, uint32_t y1, uint32_t G, int vec, uint32_t Z, int k, const int* __restrict__ centres,
                                                        const uint8_t* __restrict__ status, const uint8_t* __restrict__ zone_of, uint8_t* __restrict__ zone) {
    const size_t items = (size_t)(y1 - y0) * G;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const uint32_t y = y0 + (uint32_t)(i / G), xs = (uint32_t)(i % G) * kPx;
        const uint32_t n = W - xs < (uint32_t)kPx ? W - xs : (uint32_t)kPx;
        const size_t base = (size_t)y * W + xs;
        uint32_t lab[kPx], out[kPx];
        int v[D][kPx];
        int c[8 * D];
        load8_u16(labels, base, n, vec, lab);
#pragma unroll
        for (int d = 0; d < D; ++d) load8_i16(feat + (size_t)d * plane, base, n, vec, v[d]);
        uint32_t cur = 0;
        bool zoned = false;
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
            out[j] = 0;
            const uint32_t l = lab[j] > Z ? 0u : lab[j];
            bool member = (uint32_t)j < n && l != 0;
            int px[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                px[d] = v[d][j];
                member = member && px[d] != kNoData;
            }
            if (!member) continue;
            if (l != cur) {
                cur = l;
                zoned = status[l] == 2;
                if (zoned) fetch_centres<D, 8>(centres, l, k, c);
            }
            if (zoned) out[j] = zone_of[(size_t)l * k + nearest<D, 8>(c, k, px)];
        }
        if (vec) {
            *(uint2*)(zone + base) = make_uint2(out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24, out[4] | out[5] << 8 | out[6] << 16 | out[7] << 24);
        } else {
            for (uint32_t j = 0; j < n; ++j) zone[base + j] = (uint8_t)out[j];
        }
    }
}

// one Jacobi pass of the 3 x 3 mode filter over rows [y0, y1): src is the whole previous raster.  One lane a group of 8 pixels: per
// row of the neighbourhood one 8-byte load of the zones, one 16-byte load of the labels and the two samples beside them; a group
// without a zone loads nothing more than its own 8 bytes.
__global__ void __launch_bounds__(256) mz_mode_kernel(const uint8_t* __restrict__ src, const uint16_t* __restrict__ labels, uint32_t H, uint32_t W, uint32_t y0,
                                                      uint32_t y1, uint32_t G, int vec, int k, uint8_t* __restrict__ dst) {
    const size_t items = (size_t)(y1 - y0) * G;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const uint32_t y = y0 + (uint32_t)(i / G), xs = (uint32_t)(i % G) * kPx;
        const uint32_t n = W - xs < (uint32_t)kPx ? W - xs : (uint32_t)kPx;
        const size_t base = (size_t)y * W + xs;
        uint32_t own[kPx], out[kPx];
        load8_u8(src, base, n, vec, own);
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
            any |= own[j];
            out[j] = 0;
        }
        if (any) {
            uint32_t lab[kPx];
            unsigned long long votes[kPx];                       // 8 bits per id: at most 9 votes each
            load8_u16(labels, base, n, vec, lab);
#pragma unroll
            for (int j = 0; j < kPx; ++j) votes[j] = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                if ((dy < 0 && y == 0) || (dy > 0 && y + 1 >= H)) continue;
                const size_t rb = (size_t)(y + dy) * W + xs;
                uint32_t z[kPx + 2], l[kPx + 2];                 // the columns xs - 1 .. xs + 8; a zone of 0 casts no vote
                load8_u8(src, rb, n, vec, z + 1);
                load8_u16(labels, rb, n, vec, l + 1);
                z[0] = xs > 0 ? src[rb - 1] : 0u;
                l[0] = xs > 0 ? labels[rb - 1] : 0u;
                z[kPx + 1] = xs + kPx < W ? src[rb + kPx] : 0u;
                l[kPx + 1] = xs + kPx < W ? labels[rb + kPx] : 0u;
#pragma unroll
                for (int j = 0; j < kPx; ++j)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const uint32_t zz = z[j + dx];
                        if (zz != 0 && zz <= 8u && l[j + dx] == lab[j]) votes[j] += 1ull << (8 * (zz - 1));
                    }
            }
#pragma unroll
            for (int j = 0; j < kPx; ++j) {
                if (own[j] == 0 || own[j] > 8u) continue;
                uint32_t best = 0, most = 0;
                for (int c = 1; c <= k; ++c) {
                    const uint32_t v = (uint32_t)(votes[j] >> (8 * (c - 1))) & 255u;
                    if (v > most) { most = v; best = (uint32_t)c; }
                }
                const uint32_t mine = (uint32_t)(votes[j] >> (8 * (own[j] - 1))) & 255u;
                out[j] = mine == most ? own[j] : best;           // the own id if it is among the tied, otherwise the smallest of them
            }
        }
        if (vec) {
            *(uint2*)(dst + base) = make_uint2(out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24, out[4] | out[5] << 8 | out[6] << 16 | out[7] << 24);
        } else {
            for (uint32_t j = 0; j < n; ++j) dst[base + j] = (uint8_t)out[j];
        }
    }
}

inline bool bad_call(const void* a, const void* b, int D, int H, int W, int y0, int y1, int Z, int k) {
    return !a || !b || D < 1 || D > 4 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || y0 < 0 || y0 >= y1 || y1 > H || Z < 1 || Z > 65535 || k < 2 ||
           k > 8;
}
inline Walk walk_of(int W, int y0, int y1, int vec) {
    Walk g;
    g.W = (uint32_t)W; g.y0 = (uint32_t)y0; g.y1 = (uint32_t)y1;
    g.tiles_y = ((uint32_t)(y1 - y0) + kTileH - 1) / kTileH;
    g.ntiles = g.tiles_y * (((uint32_t)W + kTileW - 1) / kTileW);
    g.vec = vec;
    return g;
}
inline int walk_grid(const Walk& g) { return capped_grid((int)(g.ntiles < (uint32_t)kMostBlocks ? g.ntiles : (uint32_t)kMostBlocks), g.ntiles, GF_DISPLAY); }
inline int vec_of(int W, const void* a, const void* b, const void* c) { return W % 8 == 0 && !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15); }

template <int D, bool TABLE>
hipError_t launch_sums(const SumArgs& a, hipStream_t st) {
    const int grid = walk_grid(a.g);
    if (a.k <= 4)
        hipLaunchKernelGGL((mz_sums_kernel<D, 4, TABLE>), dim3((unsigned)grid), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((mz_sums_kernel<D, 8, TABLE>), dim3((unsigned)grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_mzones_clear(uint32_t* d_cnt, int* d_lo, int* d_hi, int Z, int D, hipStream_t st) {
    if (!d_cnt || !d_lo || !d_hi || Z < 1 || Z > 65535 || D < 1 || D > 4) return hipErrorInvalidValue;
    const size_t fields = (size_t)Z + 1;
    hipLaunchKernelGGL(mz_clear_kernel, dim3((unsigned)stride_grid(fields, 1 << 16, GF_DISPLAY)), dim3(256), 0, st, d_cnt, d_lo, d_hi, fields, D);
    return hipGetLastError();
}

hipError_t launch_mzones_stats(const int16_t* d_feat, int D, int H, int W, int y0, int y1, const uint16_t* d_labels, int Z, uint32_t* d_cnt, int* d_lo,
                               int* d_hi, hipStream_t st) {
    if (bad_call(d_feat, d_labels, D, H, W, y0, y1, Z, 2) || !d_cnt || !d_lo || !d_hi) return hipErrorInvalidValue;
    const size_t plane = (size_t)H * W;
    const Walk g = walk_of(W, y0, y1, vec_of(W, d_feat, d_labels, nullptr));
    const int grid = walk_grid(g);
    switch (D) {
    case 1: hipLaunchKernelGGL(mz_stats_kernel<1>, dim3((unsigned)grid), dim3(256), 0, st, d_feat, plane, d_labels, g, (uint32_t)Z, d_cnt, d_lo, d_hi); break;
    case 2: hipLaunchKernelGGL(mz_stats_kernel<2>, dim3((unsigned)grid), dim3(256), 0, st, d_feat, plane, d_labels, g, (uint32_t)Z, d_cnt, d_lo, d_hi); break;
    case 3: hipLaunchKernelGGL(mz_stats_kernel<3>, dim3((unsigned)grid), dim3(256), 0, st, d_feat, plane, d_labels, g, (uint32_t)Z, d_cnt, d_lo, d_hi); break;
    default: hipLaunchKernelGGL(mz_stats_kernel<4>, dim3((unsigned)grid), dim3(256), 0, st, d_feat, plane, d_labels, g, (uint32_t)Z, d_cnt, d_lo, d_hi); break;
    }
    return hipGetLastError();
}

hipError_t launch_mzones_start(const uint32_t* d_cnt, const int* d_lo, const int* d_hi, int Z, int k, int D, long long least, uint8_t* d_status,
                               int* d_centres, hipStream_t st) {
    if (!d_cnt || !d_lo || !d_hi || !d_status || !d_centres || Z < 1 || Z > 65535 || k < 2 || k > 8 || D < 1 || D > 4 || least < 1) return hipErrorInvalidValue;
    const size_t fields = (size_t)Z + 1;
    hipLaunchKernelGGL(mz_start_kernel, dim3((unsigned)stride_grid(fields * k, 1 << 16, GF_DISPLAY)), dim3(256), 0, st, d_cnt, d_lo, d_hi, fields, k, D, least,
                       d_status, d_centres);
    return hipGetLastError();
}

hipError_t launch_mzones_accumulate(const int16_t* d_feat, int D, int H, int W, int y0, int y1, const uint16_t* d_labels, int Z, int k,
                                    const int* d_centres, const uint8_t* d_status, const uint8_t* d_zone, unsigned long long* d_acc, hipStream_t st) {
    if (bad_call(d_feat, d_labels, D, H, W, y0, y1, Z, k) || !d_acc || (!d_zone && (!d_centres || !d_status))) return hipErrorInvalidValue;
    SumArgs a{};
    a.feat = d_feat; a.plane = (size_t)H * W; a.labels = d_labels; a.zone = d_zone;
    a.g = walk_of(W, y0, y1, vec_of(W, d_feat, d_labels, d_zone));
    a.Z = (uint32_t)Z; a.k = k; a.centres = d_centres; a.status = d_status; a.acc = d_acc;
    if (d_zone) {
        switch (D) {
        case 1: return launch_sums<1, true>(a, st);
        case 2: return launch_sums<2, true>(a, st);
        case 3: return launch_sums<3, true>(a, st);
        default: return launch_sums<4, true>(a, st);
        }
    }
    switch (D) {
    case 1: return launch_sums<1, false>(a, st);
    case 2: return launch_sums<2, false>(a, st);
    case 3: return launch_sums<3, false>(a, st);
    default: return launch_sums<4, false>(a, st);
    }
}

hipError_t launch_mzones_update(unsigned long long* d_acc, int Z, int k, int D, const uint8_t* d_status, int* d_centres, uint32_t* d_changed, hipStream_t st) {
    if (!d_acc || !d_status || !d_centres || !d_changed || Z < 1 || Z > 65535 || k < 2 || k > 8 || D < 1 || D > 4) return hipErrorInvalidValue;
    const size_t fields = (size_t)Z + 1;
    hipLaunchKernelGGL(mz_update_kernel, dim3((unsigned)stride_grid(fields * k, 1 << 16, GF_DISPLAY)), dim3(256), 0, st, d_acc, fields, k, D, d_status, d_centres,
                       d_changed);
    return hipGetLastError();
}

hipError_t launch_mzones_rank(const int* d_centres, int Z, int k, int D, const uint8_t* d_status, uint8_t* d_zone_of, int* d_ranked, hipStream_t st) {
    if (!d_centres || !d_status || !d_zone_of || !d_ranked || Z < 1 || Z > 65535 || k < 2 || k > 8 || D < 1 || D > 4) return hipErrorInvalidValue;
    const size_t fields = (size_t)Z + 1;
    hipLaunchKernelGGL(mz_rank_kernel, dim3((unsigned)stride_grid(fields * k, 1 << 16, GF_DISPLAY)), dim3(256), 0, st, d_centres, fields, k, D, d_status,
                       d_zone_of, d_ranked);
    return hipGetLastError();
}

hipError_t launch_mzones_assign(const int16_t* d_feat, int D, int H, int W, int y0, int y1, const uint16_t* d_labels, int Z, int k, const int* d_centres,
                                const uint8_t* d_status, const uint8_t* d_zone_of, uint8_t* d_zone, hipStream_t st) {
    if (bad_call(d_feat, d_labels, D, H, W, y0, y1, Z, k) || !d_centres || !d_status || !d_zone_of || !d_zone) return hipErrorInvalidValue;
    const size_t plane = (size_t)H * W;
    const uint32_t G = ((uint32_t)W + kPx - 1) / kPx;
    const int vec = vec_of(W, d_feat, d_labels, d_zone);
    const int grid = stride_grid((size_t)(y1 - y0) * G, 1 << 16, GF_DISPLAY);
#define MZ_ASSIGN(DD)                                                                                                                                   \
    hipLaunchKernelGGL(mz_assign_kernel<DD>, dim3((unsigned)grid), dim3(256), 0, st, d_feat, plane, d_labels, (uint32_t)W, (uint32_t)y0, (uint32_t)y1, G, vec, \
                       (uint32_t)Z, k, d_centres, d_status, d_zone_of, d_zone)
    switch (D) {
    case 1: MZ_ASSIGN(1); break;
    case 2: MZ_ASSIGN(2); break;
    case 3: MZ_ASSIGN(3); break;
    default: MZ_ASSIGN(4); break;
    }
#undef MZ_ASSIGN
    return hipGetLastError();
}

hipError_t launch_mzones_mode(const uint8_t* d_src, const uint16_t* d_labels, int H, int W, int y0, int y1, int k, uint8_t* d_dst, hipStream_t st) {
    if (!d_src || !d_labels || !d_dst || d_src == d_dst || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || y0 < 0 || y0 >= y1 || y1 > H || k < 2 || k > 8)
        return hipErrorInvalidValue;
    const uint32_t G = ((uint32_t)W + kPx - 1) / kPx;
    const int grid = stride_grid((size_t)(y1 - y0) * G, 1 << 16, GF_DISPLAY);
    hipLaunchKernelGGL(mz_mode_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_src, d_labels, (uint32_t)H, (uint32_t)W, (uint32_t)y0, (uint32_t)y1, G,
                       vec_of(W, d_src, d_labels, d_dst), k, d_dst);
    return hipGetLastError();
}

}  // namespace s2sr
