// Polygon rasterisation to zone labels: features made of rings -> a uint16 label raster and, optionally, the pixels
// per label.  The tables' checks and the binning of features to tiles are host code (zone_bins.h); the policy around it -- GeoJSON,
// projection, quantisation, labels -- is Python (s2sr/zones.py).
//
// Definition (integers; tests/zones_model.py restates it in numpy and in Python integers):
//   coordinates   int32 in 1/256 of a label pixel, |x|, |y| <= 2^29; the centre of pixel (r, c) is (cx, cy) = (256 c + 128, 256 r + 128)
//   an edge       with its endpoints exchanged so that ya < yb (ya == yb: never counts) counts for a centre iff
//                 ya <= cy < yb  and  (cx - xa) (yb - ya) < (xb - xa) (cy - ya)
//   inside        a centre is inside a feature iff the count over all edges of all its rings is odd
//   per row       dy = yb - ya, N = (xb - xa) (cy - ya) + (xa - 128) dy: the edge toggles exactly the columns c with 256 c dy < N
//   labels        the pixel gets the label of the LAST feature of the list that holds its centre, 0 when none does
//   area          uint64 [Z + 1]: the pixels per label, row 0 the unlabelled ones (added to)
//
// One wave per tile of 64 x 64 pixels, one lane per row; a workgroup is one wave, so everything that depends on the tile and the
// feature only -- the candidate, its rings, an edge's endpoints -- is provably wave-uniform and lives in scalar registers: a ring's
// vertices arrive 64 at a time, one per lane in one coalesced load, and are handed round lane by lane (v_readlane), so a ring of
// thousands of vertices costs no memory latency per edge; and each lane first judges the edge that ends in its own vertex against the
// tile, so the wave walks only the edges that can toggle a pixel of it (a ballot): the bench scene's 2000-vertex ring costs a tile
// 32 loads and ballots, not 2000 turns of a scalar loop.  The
// tile's candidates (zone_bins.h: the features whose bounding box meets it, ascending) are walked latest first.  Per candidate a lane
// XORs, for every edge that crosses its row, the mask of the tile's columns the edge toggles into a 64-bit parity word: with
// N' = N - 256 c0 dy (c0 the tile's first column) that is the columns j of the tile with j (256 dy) < N', found WITHOUT a division by
// six compare-and-add steps over the shifted divisor (64-bit; the quotient has 6 bits).  Edges wholly above or below the tile's rows,
// or wholly left of its first centre, never reach the walk; an edge wholly right of its last centre toggles the whole row.
// XOR commutes: no order of edges or rings matters.  The bits set and not yet taken get the candidate's label, in LDS; a tile whose
// 64 words are full stops early (the inside of a field: one candidate).  Columns beyond W and rows outside the band count as taken
// from the start, so they neither hold the walk up nor are ever stored.
//
// Leaving the tile: the 8 KB of labels lie in LDS as 64 rows of 128 B (+ 16 B of padding per row, which spreads the lanes' row
// writes over the banks); lane l of step i takes the 16 bytes of chunk 64 i + l, 8 lanes per row: one 16-byte store per lane where
// W is a multiple of 8, two 8-byte stores where it is a multiple of 4 (every x4 product), single samples otherwise.  Every pixel of
// the band is stored exactly once and nothing of the raster is read.  Magnitudes: |xb - xa|, dy <= 2^30, |cy - ya| < 2^31 (cy is
// clamped to 2^30: above every coordinate), |xa - 128 - 256 c0| < 2^31 (c0 clamped likewise), so |N'| < 2^62.
//
// area.  A lane knows how many pixels of its row a candidate labelled: the population count of the bits it took.  The wave adds
// them up and one lane adds the sum to the label's counter: one atomic per candidate and tile that labelled anything, and one for
// the pixels left at 0.  (Counting the finished labels in the store pass, a lane's runs as atomics wherever the wave holds more than
// one label, was the first version: with fields of ~120 pixels most tiles hold a border, and 3 x 10^7 atomics on 16 k addresses cost
// more than everything else together; profiles/zones_bench_line.json has this version's figure.)  Integer adds: exact, and no order
// changes them.
#include "s2sr_internal.h"

namespace s2sr {

namespace {

constexpr int kTile = 64;
constexpr int kRowBytes = 144;                                   // 128 B of labels + 16 B of padding
constexpr int32_t kFar = 1 << 30;                                // beyond every coordinate

struct ZoneArgs {
    uint32_t W, tiles_x, ty0, ntiles, y0, y1;                    // the band: rows [y0, y1), its first tile row, its tiles
    uint32_t vec;                                                // 16 / 8 / 2: the bytes of one store
};

__device__ __forceinline__ uint32_t half_of(const uint4& v, int j) {
    const uint32_t w = j < 2 ? v.x : j < 4 ? v.y : j < 6 ? v.z : v.w;
    return (j & 1) ? w >> 16 : w & 0xffffu;
}

// the sum of n over the wave's lanes, added to *dst by one lane (nothing when it is zero)
__device__ __forceinline__ void wave_add(unsigned long long* dst, uint32_t n, uint32_t lane) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n += (uint32_t)__shfl_xor((int)n, m);
    if (lane == 0 && n) atomicAdd(dst, (unsigned long long)n);
}

// The tables are kernel arguments of their own, const and __restrict__: nothing the kernel stores aliases them, so their wave-uniform
// loads may stay on the scalar unit across the tile loop's stores.
__global__ void __launch_bounds__(kTile) zones_kernel(const int32_t* __restrict__ xy, const int32_t* __restrict__ ring_start,
                                                      const int32_t* __restrict__ feat_start, const uint16_t* __restrict__ label,
                                                      const uint32_t* __restrict__ tile_start, const int32_t* __restrict__ tile_feat,
                                                      uint16_t* __restrict__ out, unsigned long long* __restrict__ area, const ZoneArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[kTile * kRowBytes];
    const uint32_t lane = threadIdx.x;
    for (uint32_t it = blockIdx.x; it < p.ntiles; it += gridDim.x) {
        const uint32_t tyr = it / p.tiles_x, tx = it - tyr * p.tiles_x, ty = p.ty0 + tyr;
        const uint32_t t = ty * p.tiles_x + tx, c0 = tx * kTile, r0 = ty * kTile, r = r0 + lane;
        const uint32_t wcols = p.W - c0 < (uint32_t)kTile ? p.W - c0 : (uint32_t)kTile;
        const unsigned long long colmask = wcols == (uint32_t)kTile ? ~0ull : (1ull << wcols) - 1;
        unsigned long long taken = r >= p.y0 && r < p.y1 ? ~colmask : ~0ull;
        unsigned char* const row = tile + lane * kRowBytes;
#pragma unroll
        for (int j = 0; j < 8; ++j) ((uint4*)row)[j] = make_uint4(0, 0, 0, 0);
        // the live rows of the tile and the tile's first column, in coordinate units, clamped beyond every coordinate
        const uint32_t rlo = r0 > p.y0 ? r0 : p.y0, rhi = r0 + kTile < p.y1 ? r0 + kTile : p.y1;      // rows [rlo, rhi)
        const long long far = kFar;
        const int32_t cy = (int32_t)min(256ll * r + 128, far);
        const int32_t cy_top = (int32_t)min(256ll * rlo + 128, far), cy_bot = (int32_t)min(256ll * (rhi - 1) + 128, far);
        const int32_t X0 = (int32_t)min(256ll * c0, far);
        const int32_t cx_first = X0 + 128, cx_last = X0 + 256 * (kTile - 1) + 128;
        const uint32_t i0 = tile_start[t];
        for (uint32_t i = tile_start[t + 1]; i > i0;) {
            --i;
            if (__ballot(taken != ~0ull) == 0) break;            // every pixel of the tile has its label
            const int32_t f = tile_feat[i];
            unsigned long long par = 0;
            const int32_t ring1 = feat_start[f + 1];
            for (int32_t ring = feat_start[f]; ring < ring1; ++ring) {
                const int32_t v0 = ring_start[ring], v1 = ring_start[ring + 1];
                int32_t px = xy[2 * (size_t)(v1 - 1)], py = xy[2 * (size_t)(v1 - 1) + 1];
                for (int32_t base = v0; base < v1; base += kTile) {       // 64 vertices at a time: one coalesced load, then lane by lane
                  const int32_t cnt = v1 - base < kTile ? v1 - base : kTile;
                  int2 mine = make_int2(0, 0);
                  if ((int32_t)lane < cnt) mine = ((const int2*)xy)[(size_t)base + lane];
                  // lane k holds the edge that ends in vertex base + k: it starts in the lane below's vertex, lane 0's in the one carried
                  // over.  Each lane judges its own edge against the tile -- flat, wholly above or below the live rows, wholly left of
                  // the first centre: it toggles nothing here -- and the wave walks the edges that are left.
                  int32_t sx = __shfl_up(mine.x, 1), sy = __shfl_up(mine.y, 1);
                  if (lane == 0) { sx = px; sy = py; }
                  const int32_t ylo = min(sy, mine.y), yhi = max(sy, mine.y);
                  unsigned long long todo = __ballot((int32_t)lane < cnt && ylo != yhi && yhi > cy_top && ylo <= cy_bot && max(sx, mine.x) > cx_first);
                  px = __builtin_amdgcn_readlane(mine.x, cnt - 1);
                  py = __builtin_amdgcn_readlane(mine.y, cnt - 1);
                  while (todo) {
                    const int k = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const int32_t qx = __builtin_amdgcn_readlane(mine.x, k), qy = __builtin_amdgcn_readlane(mine.y, k);
                    const int32_t ox = __builtin_amdgcn_readlane(sx, k), oy = __builtin_amdgcn_readlane(sy, k);
                    const bool up = oy < qy;
                    const int32_t xa = up ? ox : qx, ya = up ? oy : qy, xb = up ? qx : ox, yb = up ? qy : oy;
                    const bool hit = ya <= cy && cy < yb;
                    if (min(xa, xb) > cx_last) {                                      // right of every centre: the whole row
                        par ^= hit ? ~0ull : 0ull;
                        continue;
                    }
                    const int32_t dy = yb - ya;
                    const long long D = (long long)dy << 8;
                    const long long N = (long long)(xb - xa) * (cy - ya) + (long long)(xa - 128 - X0) * dy;
                    long long acc = 0;
                    uint32_t m = 0;                              // the largest j in 0..63 with j D < N (N > 0)
#pragma unroll
                    for (int s = 5; s >= 0; --s) {
                        const long long next = acc + (D << s);
                        const bool below = next < N;
                        acc = below ? next : acc;
                        m += below ? 1u << s : 0u;
                    }
                    par ^= hit && N > 0 ? (2ull << m) - 1 : 0ull;                      // columns 0..m of the tile
                  }
                }
            }
            const unsigned long long fresh = par & ~taken;
            taken |= fresh;
            if (__ballot(fresh != 0) == 0) continue;             // a candidate by its bounding box only
            const uint32_t lab = label[f];
            const uint32_t w = lab | lab << 16;
#pragma unroll
            for (int j = 0; j < 8; ++j) {                        // the row in chunks of 8 pixels: a whole chunk is one 16-byte write
                const uint32_t b = (uint32_t)(fresh >> (8 * j)) & 0xffu;
                if (b == 0xffu) {
                    ((uint4*)row)[j] = make_uint4(w, w, w, w);
                } else if (b) {                                  // the chunk was zeroed and no pixel is taken twice: OR is assignment
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t m = ((b >> (2 * k)) & 1u ? 0xffffu : 0u) | ((b >> (2 * k + 1)) & 1u ? 0xffff0000u : 0u);
                        if (m) atomicOr((uint32_t*)(row + 16 * j + 4 * k), w & m);
                    }
                }
            }
            if (area) wave_add(area + lab, (uint32_t)__popcll(fresh), lane);
        }
        if (area) wave_add(area, (uint32_t)__popcll(~taken), lane);       // the pixels no feature holds
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
            const uint32_t q = i * kTile + lane, rr = q >> 3, ch = q & 7;
            const uint32_t y = r0 + rr, x = c0 + 8 * ch;
            const uint4 v = *(const uint4*)(tile + rr * kRowBytes + 16 * ch);
            const uint32_t n = y >= p.y0 && y < p.y1 && x < p.W ? (p.W - x < 8u ? p.W - x : 8u) : 0u;
            if (n) {
                uint16_t* dst = out + (size_t)y * p.W + x;
                if (p.vec == 16 && n == 8) {
                    *(uint4*)dst = v;
                } else if (p.vec >= 8 && (n == 4 || n == 8)) {
                    *(uint2*)dst = make_uint2(v.x, v.y);
                    if (n == 8) *(uint2*)(dst + 4) = make_uint2(v.z, v.w);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if ((uint32_t)j < n) dst[j] = (uint16_t)half_of(v, j);
                }
            }
        }
        __syncthreads();                                         // the next tile's zeroes come behind this one's reads
    }
}

}  // namespace

hipError_t launch_zones_rasterize(const int32_t* d_xy, const int32_t* d_ring_start, const int32_t* d_feat_start, const uint16_t* d_label,
                                  const uint32_t* d_tile_start, const int32_t* d_tile_feat, int H, int W, int y0, int y1, uint16_t* d_out,
                                  unsigned long long* d_area, hipStream_t st) {
    if (!d_xy || !d_ring_start || !d_feat_start || !d_label || !d_tile_start || !d_tile_feat || !d_out || ((uintptr_t)d_out & 15) ||
        ((uintptr_t)d_area & 7) || ((uintptr_t)d_xy & 7) || ((uintptr_t)d_tile_start & 3) || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL ||
        y0 < 0 || y0 >= y1 || y1 > H)
        return hipErrorInvalidValue;
    ZoneArgs a{};
    a.W = (uint32_t)W; a.tiles_x = ((uint32_t)W + kTile - 1) / kTile;
    a.ty0 = (uint32_t)y0 / kTile;
    const long long ntiles = (long long)(((uint32_t)y1 + kTile - 1) / kTile - a.ty0) * a.tiles_x;
    a.ntiles = (uint32_t)ntiles;
    a.y0 = (uint32_t)y0; a.y1 = (uint32_t)y1;
    a.vec = W % 8 == 0 ? 16 : W % 4 == 0 ? 8 : 2;
    const int grid = capped_grid((int)(ntiles < 16384 ? ntiles : 16384), ntiles, GF_DISPLAY);
    hipLaunchKernelGGL(zones_kernel, dim3((unsigned)grid), dim3(kTile), 0, st, d_xy, d_ring_start, d_feat_start, d_label, d_tile_start, d_tile_feat, d_out,
                       d_area, a);
    return hipGetLastError();
}

}  // namespace s2sr
