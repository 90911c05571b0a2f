// Fields from the image: an int16 index raster -> uint16 zone labels, the inverse of zones.hip.  A threshold mask, a
// separable binary morphology, block-based union-find labelling and a numbering by prefix sum, all in integers.  The host side is
// engine_fields.hip; the rings around the labels are host code (ring_trace.h); the policy -- index units, hectares, GeoJSON -- is
// Python (s2sr/fields.py).
//
// Definition (tests/fields_model.py restates it in numpy):
//   mask          m0 = idx != -32768 and lo <= idx <= hi
//   morphology    binary, the (2 r + 1) x (2 r + 1) square: erode is the AND, dilate the OR over the neighbours INSIDE the image;
//                 open = dilate(erode(m0, r_open), r_open), close = erode(dilate(open, r_close), r_close), m = close and idx != -32768
//   components    of m under conn 4 or 8; a component's key is the smallest linear index y W + x among its pixels; components of
//                 fewer than min_pixels pixels become 0, the rest are numbered 1, 2, ... by ascending key; `found` counts them; a
//                 number above Z is written as 0
//   fields        int64 [Z + 1][6] = pixels, key, x0, y0, x1, y1 (half-open box); row 0: the unlabelled pixels, then zeros
//
// Mask planes are uint8, one thread per group of 8 pixels of a row (one 16-byte load of the index, 8-byte loads and stores of the
// planes where W is a multiple of 8, single samples otherwise).  The element is a square, so a pass is a running OR over at most 17
// samples of a row or a column; erode is dilate of the complement, and a neighbour outside the image is 0 in either: it takes no part.
//
// Labelling, every step a launch of its own (no workgroup ever waits for another; order comes from the stream):
//   local    one workgroup per 64 x 64 tile, the tile's union-find in LDS.  A row of the tile is one wave, so a ballot gives each
//            pixel the start of its horizontal run as its first parent; the vertical (and diagonal) joins are atomicMin unions, one
//            per run overlap, not per pixel.  Out go the global linear index of the local root (-1: background) and, at the local
//            roots, the local component's pixel count (0 elsewhere): the sizes are pre-aggregated here.
//   border   one thread per pixel below a horizontal or right of a vertical tile line joins its 1 (conn 4) or 3 (conn 8)
//            neighbours across the line.  find follows parents, union is an atomicMin retry on the larger root.
//   flatten  every pixel's parent becomes its root; a local root that is no root adds its count to its root's: one atomicAdd per
//            local component and tile.
// parent[p] <= p holds throughout: parents only ever decrease, every find terminates, the root is the component's smallest linear
// index -- its key -- whatever order the atomics land in.  Loads that may meet another workgroup's store go to the device-coherent
// level (a stale parent would still be an ancestor, so even that would cost a turn of the loop and no more).
//
// Numbering: flag = parent[p] == p and size[p] >= min_pixels; chunks of 1024 pixels count their flags, one workgroup scans the
// counts, the chunks apply: the root's size entry becomes its rank (0: too small) and fields gets pixels and key.  The last pass
// writes the labels a tile at a time, gathers each label's box in an LDS table (the keys are claimed by compare-and-swap, a label
// that finds no place within 8 probes goes to the global row directly) and issues one atomicMin / atomicMax set per label and tile.
#include "s2sr_internal.h"

namespace s2sr {

namespace {

constexpr int kTile = 64;
constexpr int kChunk = 1024;                                     // pixels per numbering chunk: 256 threads x 4
constexpr int kHash = 512;                                       // entries of the labels pass's box table
constexpr int kProbes = 8;

__device__ __forceinline__ int coherent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// bit j = sample j of the group at `base` is set, j < n
__device__ __forceinline__ uint32_t load_bits(const uint8_t* __restrict__ p, size_t base, uint32_t n, bool vec) {
    uint32_t bits = 0;
    if (vec) {
        const uint2 v = *(const uint2*)(p + base);
#pragma unroll
        for (int j = 0; j < 4; ++j) bits |= ((v.x >> (8 * j)) & 1u) << j | ((v.y >> (8 * j)) & 1u) << (4 + j);
    } else {
        for (uint32_t j = 0; j < n; ++j) bits |= (p[base + j] ? 1u : 0u) << j;
    }
    return bits;
}
__device__ __forceinline__ void store_bits(uint8_t* __restrict__ p, size_t base, uint32_t n, bool vec, uint32_t bits) {
    if (vec) {
        uint2 v = make_uint2(0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v.x |= ((bits >> j) & 1u) << (8 * j);
            v.y |= ((bits >> (4 + j)) & 1u) << (8 * j);
        }
        *(uint2*)(p + base) = v;
    } else {
        for (uint32_t j = 0; j < n; ++j) p[base + j] = (uint8_t)((bits >> j) & 1u);
    }
}
// bit j = the index sample is data (and, with a range, inside it)
__device__ __forceinline__ uint32_t index_bits(const int16_t* __restrict__ idx, size_t base, uint32_t n, bool vec, int lo, int hi) {
    uint32_t bits = 0;
    if (vec) {
        const uint4 v = *(const uint4*)(idx + base);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int s = (int16_t)(w[j >> 1] >> (16 * (j & 1)));
            bits |= (s != -32768 && s >= lo && s <= hi ? 1u : 0u) << j;
        }
    } else {
        for (uint32_t j = 0; j < n; ++j) {
            const int s = idx[base + j];
            bits |= (s != -32768 && s >= lo && s <= hi ? 1u : 0u) << j;
        }
    }
    return bits;
}

// and_into 0: mask = in range; 1: mask &= is data (lo, hi span every value)
__global__ void __launch_bounds__(256) fields_mask_kernel(const int16_t* __restrict__ idx, uint8_t* __restrict__ mask, uint32_t H, uint32_t W,
                                                          uint32_t G, int lo, int hi, int and_into, int vec) {
    const size_t items = (size_t)H * G;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const uint32_t y = (uint32_t)(i / G), x0 = (uint32_t)(i - (size_t)y * G) * 8;
        const uint32_t n = W - x0 < 8u ? W - x0 : 8u;
        const size_t base = (size_t)y * W + x0;
        uint32_t bits = index_bits(idx, base, n, vec, lo, hi);
        if (and_into) bits &= load_bits(mask, base, n, vec);
        store_bits(mask, base, n, vec, bits);
    }
}

// one pass of the morphology: along the row (kCol false) or the column (true); erode as the dilate of the complement
template <bool kCol>
__global__ void __launch_bounds__(256) fields_morph_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t H, uint32_t W,
                                                           uint32_t G, int r, int erode, int vec) {
    const size_t items = (size_t)H * G;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const uint32_t y = (uint32_t)(i / G), x0 = (uint32_t)(i - (size_t)y * G) * 8;
        const uint32_t n = W - x0 < 8u ? W - x0 : 8u;
        const uint32_t live = (1u << n) - 1;
        uint32_t out;
        if (kCol) {
            const uint32_t ya = y > (uint32_t)r ? y - r : 0u, yb = y + r < H - 1 ? y + r : H - 1;
            uint32_t acc = 0;
            for (uint32_t yy = ya; yy <= yb; ++yy) {
                const uint32_t b = load_bits(src, (size_t)yy * W + x0, n, vec);
                acc |= erode ? ~b & live : b;
            }
            out = erode ? ~acc & live : acc;
        } else {
            // the 24 samples [x0 - 8, x0 + 16) as bits, those outside the image 0
            uint32_t m = 0, in_image = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const long long xs = (long long)x0 - 8 + 8 * k;
                if (xs < 0 || xs >= (long long)W) continue;
                const uint32_t nn = W - (uint32_t)xs < 8u ? W - (uint32_t)xs : 8u;
                m |= load_bits(src, (size_t)y * W + (size_t)xs, nn, vec) << (8 * k);
                in_image |= ((1u << nn) - 1) << (8 * k);
            }
            const uint32_t in = erode ? ~m & in_image : m;
            uint32_t d = in;
            for (int s = 1; s <= r; ++s) d |= in >> s | in << s;
            d = (d >> 8) & live;
            out = erode ? ~d & live : d;
        }
        store_bits(dst, (size_t)y * W + x0, n, vec, out);
    }
}

// ---- union-find ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(const volatile int* P, int x) {
    int p;
    while ((p = P[x]) != x) x = p;
    return x;
}
// Both are roots' descendants of one tile; the larger root is hung below the smaller.  Each turn max(a, b) strictly decreases.
__device__ __forceinline__ void lds_union(int* P, int a, int b) {
    a = lds_find(P, a);
    b = lds_find(P, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&P[a], b);
        if (old == a) break;                                     // a was a root and now hangs below b
        a = lds_find(P, old);                                    // a had a parent already: that one and b are still to be joined
        b = lds_find(P, b);
    }
}
__device__ __forceinline__ int dev_find(const int* parent, int x) {
    int p;
    while ((p = coherent(parent + x)) != x) x = p;
    return x;
}
__device__ __forceinline__ void dev_union(int* parent, int a, int b) {
    a = dev_find(parent, a);
    b = dev_find(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[a], b);
        if (old == a) break;
        a = dev_find(parent, old);
        b = dev_find(parent, b);
    }
}

__global__ void __launch_bounds__(256) fields_local_kernel(const uint8_t* __restrict__ mask, int* __restrict__ parent, uint32_t* __restrict__ size,
                                                           uint32_t H, uint32_t W, uint32_t tiles_x, uint32_t ntiles, int conn8) {
    __shared__ int P[kTile * kTile];
    __shared__ uint32_t cnt[kTile * kTile];
    __shared__ unsigned long long rowbits[kTile];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x, y0 = ty * kTile, x0 = tx * kTile;
        // a row is a wave: every pixel's first parent is the start of its horizontal run; the run's start holds the run's length
        for (uint32_t ly = wave; ly < (uint32_t)kTile; ly += 4) {
            const uint32_t y = y0 + ly, x = x0 + lane;
            const bool fg = y < H && x < W && mask[(size_t)y * W + x] != 0;
            const unsigned long long bits = __ballot(fg);
            if (lane == 0) rowbits[ly] = bits;
            const unsigned long long below = ~bits & ((1ull << lane) - 1);           // the background left of this pixel
            const uint32_t start = below ? 64u - (uint32_t)__clzll((long long)below) : 0u;
            const unsigned long long above = ~bits >> lane;                           // bit 0 is this pixel: 0 when fg
            const uint32_t len = above ? (uint32_t)__ffsll((long long)above) - 1u : 64u - lane;
            P[ly * kTile + lane] = fg ? (int)(ly * kTile + start) : -1;
            cnt[ly * kTile + lane] = fg && start == lane ? len : 0u;
        }
        __syncthreads();
        // joins with the row above: one per overlap of two runs (a pixel whose left neighbour and that one's upper neighbour are both
        // set is joined through them)
        for (uint32_t ly = wave; ly < (uint32_t)kTile; ly += 4) {
            if (ly == 0) continue;
            const unsigned long long cur = rowbits[ly], up = rowbits[ly - 1];
            const bool me = (cur >> lane) & 1, u = (up >> lane) & 1;
            const bool l = lane > 0 && ((cur >> (lane - 1)) & 1), ul = lane > 0 && ((up >> (lane - 1)) & 1);
            const bool ur = lane < 63 && ((up >> (lane + 1)) & 1);
            const int i = (int)(ly * kTile + lane);
            if (me) {
                if (u) {
                    if (!(l && ul)) lds_union(P, i, i - kTile);
                } else if (conn8) {
                    if (ul && !l) lds_union(P, i, i - kTile - 1);
                    if (ur) lds_union(P, i, i - kTile + 1);
                }
            }
        }
        __syncthreads();
        // the run starts carry their run's length to the root; a start that is a root keeps it
        for (uint32_t ly = wave; ly < (uint32_t)kTile; ly += 4) {
            const int i = (int)(ly * kTile + lane);
            const uint32_t c = cnt[i];                           // written before the barrier; only roots are added to below
            if (c) {
                const int root = lds_find(P, i);
                if (root != i) atomicAdd(&cnt[root], c);
            }
        }
        __syncthreads();
        for (uint32_t ly = wave; ly < (uint32_t)kTile; ly += 4) {
            const uint32_t y = y0 + ly, x = x0 + lane;
            const int i = (int)(ly * kTile + lane);
            if (y < H && x < W) {
                const size_t p = (size_t)y * W + x;
                const int v = P[i];
                if (v < 0) {
                    parent[p] = -1;
                    size[p] = 0;
                } else {
                    const int root = lds_find(P, i);             // P is settled: nothing writes it behind the barrier
                    parent[p] = (int)((y0 + ((uint32_t)root >> 6)) * W + x0 + ((uint32_t)root & 63u));
                    size[p] = root == i ? cnt[i] : 0u;
                }
            }
        }
        __syncthreads();                                         // the next tile's parents come behind this one's reads
    }
}

// nh pixels below horizontal tile lines, then the pixels right of vertical ones
__global__ void __launch_bounds__(256) fields_border_kernel(int* __restrict__ parent, uint32_t H, uint32_t W, size_t nh, size_t items, int conn8) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        if (i < nh) {
            const uint32_t k = (uint32_t)(i / W), x = (uint32_t)(i - (size_t)k * W), y = kTile * (k + 1);
            const int p = (int)(y * W + x), q = p - (int)W;
            if (coherent(parent + p) < 0) continue;
            if (coherent(parent + q) >= 0) dev_union(parent, p, q);
            if (conn8) {
                if (x > 0 && coherent(parent + q - 1) >= 0) dev_union(parent, p, q - 1);
                if (x + 1 < W && coherent(parent + q + 1) >= 0) dev_union(parent, p, q + 1);
            }
        } else {
            const size_t j = i - nh;
            const uint32_t k = (uint32_t)(j / H), y = (uint32_t)(j - (size_t)k * H), x = kTile * (k + 1);
            const int p = (int)(y * W + x), q = p - 1;
            if (coherent(parent + p) < 0) continue;
            if (coherent(parent + q) >= 0) dev_union(parent, p, q);
            if (conn8) {
                if (y > 0 && coherent(parent + q - (int)W) >= 0) dev_union(parent, p, q - (int)W);
                if (y + 1 < H && coherent(parent + q + (int)W) >= 0) dev_union(parent, p, q + (int)W);
            }
        }
    }
}

__global__ void __launch_bounds__(256) fields_flatten_kernel(int* __restrict__ parent, uint32_t* __restrict__ size, size_t N) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        const int p = (int)i;
        const int v = coherent(parent + p);
        if (v < 0) continue;
        const int root = dev_find(parent, v);
        if (root != v) __hip_atomic_store(parent + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t c = size[p];                              // a local root's count: nobody adds to one that is no root
        if (c && root != p) atomicAdd(&size[root], c);
    }
}

// ---- numbering -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_field(const int* __restrict__ parent, const uint32_t* __restrict__ size, size_t p, size_t N, uint32_t min_pixels) {
    return p < N && parent[p] == (int)p && size[p] >= min_pixels;
}

__global__ void __launch_bounds__(256) fields_count_kernel(const int* __restrict__ parent, const uint32_t* __restrict__ size, size_t N,
                                                           uint32_t min_pixels, uint32_t nchunks, uint32_t* __restrict__ sums) {
    __shared__ uint32_t wtot[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        uint32_t n = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) n += (uint32_t)__popcll(__ballot(is_field(parent, size, (size_t)c * kChunk + k * 256 + threadIdx.x, N, min_pixels)));
        if (lane == 0) wtot[wave] = n;
        __syncthreads();
        if (threadIdx.x == 0) sums[c] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
}

// one workgroup: sums becomes its exclusive prefix sum, *found the total.  It walks the sums 256 at a time with two barriers a turn:
// 1024 turns at 16384 x 16384, 8192 at the H W limit (2^21 sums), serial by construction; profiles/fields_bench_line.json has what
// that costs next to the other stages.  A two-level scan in plain launches would shorten it.
__global__ void __launch_bounds__(256) fields_scan_kernel(uint32_t* __restrict__ sums, uint32_t nchunks, unsigned long long* __restrict__ found) {
    __shared__ uint32_t wtot[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t s = 0; s < nchunks; s += 256) {
        const uint32_t i = s + threadIdx.x;
        const uint32_t v = i < nchunks ? sums[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= (uint32_t)d) incl += o;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        uint32_t off = 0;
        for (uint32_t w = 0; w < wave; ++w) off += wtot[w];
        if (i < nchunks) sums[i] = carry + off + incl - v;
        carry += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) *found = carry;
}

// the root's size entry becomes its rank, 0 for a root that is too small; rows 1 .. Z of fields get pixels and key, and the box
// (huge, huge, 0, 0) that the labels pass narrows
__global__ void __launch_bounds__(256) fields_apply_kernel(const int* __restrict__ parent, uint32_t* __restrict__ size, size_t N, uint32_t min_pixels,
                                                           uint32_t nchunks, const uint32_t* __restrict__ sums, uint32_t Z,
                                                           unsigned long long* __restrict__ fields) {
    __shared__ uint32_t wtot[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        uint32_t running = sums[c];
        for (int k = 0; k < 4; ++k) {
            const size_t p = (size_t)c * kChunk + k * 256 + threadIdx.x;
            const bool root = p < N && parent[p] == (int)p;
            const uint32_t pixels = root ? size[p] : 0u;
            const bool f = root && pixels >= min_pixels;
            const unsigned long long b = __ballot(f);
            if (lane == 0) wtot[wave] = (uint32_t)__popcll(b);
            __syncthreads();
            uint32_t off = 0;
            for (uint32_t w = 0; w < wave; ++w) off += wtot[w];
            const uint32_t rank = running + off + (uint32_t)__popcll(b & ((1ull << lane) - 1)) + 1u;
            if (root) size[p] = f ? rank : 0u;
            if (f && rank <= Z) {
                unsigned long long* row = fields + (size_t)rank * 6;
                row[0] = pixels; row[1] = p; row[2] = ~0ull >> 1; row[3] = ~0ull >> 1; row[4] = 0; row[5] = 0;
            }
            running += wtot[0] + wtot[1] + wtot[2] + wtot[3];
            __syncthreads();
        }
    }
}

__device__ __forceinline__ void box_add(uint32_t* hkey, int* hbox, unsigned long long* __restrict__ fields, uint32_t lab, int xa, int xb, int y) {
    uint32_t s = (lab * 40503u) >> 7;
    for (int t = 0; t < kProbes; ++t, ++s) {
        s &= kHash - 1;
        const uint32_t prev = atomicCAS(&hkey[s], 0u, lab);
        if (prev == 0u || prev == lab) {
            atomicMin(&hbox[4 * s], xa); atomicMin(&hbox[4 * s + 1], y); atomicMax(&hbox[4 * s + 2], xb); atomicMax(&hbox[4 * s + 3], y + 1);
            return;
        }
    }
    unsigned long long* row = fields + (size_t)lab * 6;            // the table is crowded: straight to the row
    atomicMin(row + 2, (unsigned long long)xa); atomicMin(row + 3, (unsigned long long)y);
    atomicMax(row + 4, (unsigned long long)xb); atomicMax(row + 5, (unsigned long long)(y + 1));
}

__global__ void __launch_bounds__(256) fields_labels_kernel(const int* __restrict__ parent, const uint32_t* __restrict__ size, uint32_t H, uint32_t W,
                                                            uint32_t tiles_x, uint32_t ntiles, uint32_t Z, uint16_t* __restrict__ labels,
                                                            unsigned long long* __restrict__ fields, int vec) {
    __shared__ uint32_t hkey[kHash];
    __shared__ int hbox[4 * kHash];
    __shared__ uint32_t zeros;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
        for (uint32_t s = threadIdx.x; s < (uint32_t)kHash; s += 256) {
            hkey[s] = 0;
            hbox[4 * s] = 0x7fffffff; hbox[4 * s + 1] = 0x7fffffff; hbox[4 * s + 2] = 0; hbox[4 * s + 3] = 0;
        }
        if (threadIdx.x == 0) zeros = 0;
        __syncthreads();
        uint32_t nz = 0;
#pragma unroll 1
        for (int it = 0; it < 2; ++it) {
            const uint32_t y = ty * kTile + it * 32 + (threadIdx.x >> 3), xs = tx * kTile + (threadIdx.x & 7) * 8;
            if (y >= H || xs >= W) continue;
            const uint32_t n = W - xs < 8u ? W - xs : 8u;
            const size_t base = (size_t)y * W + xs;
            uint32_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            uint32_t cur = 0, from = xs;
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                if (j >= n) break;
                const int root = parent[base + j];
                uint32_t lab = root < 0 ? 0u : size[root];
                if (lab > Z) lab = 0;
                out[j] = lab;
                nz += lab == 0;
                if (lab != cur) {
                    if (cur) box_add(hkey, hbox, fields, cur, (int)from, (int)(xs + j), (int)y);
                    cur = lab;
                    from = xs + j;
                }
            }
            if (cur) box_add(hkey, hbox, fields, cur, (int)from, (int)(xs + n), (int)y);
            if (vec) {
                *(uint4*)(labels + base) = make_uint4(out[0] | out[1] << 16, out[2] | out[3] << 16, out[4] | out[5] << 16, out[6] | out[7] << 16);
            } else {
                for (uint32_t j = 0; j < n; ++j) labels[base + j] = (uint16_t)out[j];
            }
        }
        if (nz) atomicAdd(&zeros, nz);
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < (uint32_t)kHash; s += 256) {
            const uint32_t lab = hkey[s];
            if (!lab) continue;
            unsigned long long* row = fields + (size_t)lab * 6;
            atomicMin(row + 2, (unsigned long long)hbox[4 * s]); atomicMin(row + 3, (unsigned long long)hbox[4 * s + 1]);
            atomicMax(row + 4, (unsigned long long)hbox[4 * s + 2]); atomicMax(row + 5, (unsigned long long)hbox[4 * s + 3]);
        }
        if (threadIdx.x == 0 && zeros) atomicAdd(fields, (unsigned long long)zeros);
        __syncthreads();                                         // the next tile's table comes behind this one's reads
    }
}

inline bool bad_image(int H, int W) { return H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL; }
inline uint32_t groups(int W) { return ((uint32_t)W + 7) / 8; }
inline int vec_of(int W, const void* a, const void* b) { return W % 8 == 0 && !(((uintptr_t)a | (uintptr_t)b) & 15); }
inline uint32_t tiles_of(int n) { return ((uint32_t)n + kTile - 1) / kTile; }

}  // namespace

hipError_t launch_fields_mask(const int16_t* d_idx, int H, int W, int lo, int hi, int and_into, uint8_t* d_mask, hipStream_t st) {
    if (!d_idx || !d_mask || bad_image(H, W)) return hipErrorInvalidValue;
    const uint32_t G = groups(W);
    const int grid = stride_grid((size_t)H * G, 1 << 16, GF_DISPLAY);
    hipLaunchKernelGGL(fields_mask_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_idx, d_mask, (uint32_t)H, (uint32_t)W, G, lo, hi, and_into,
                       vec_of(W, d_idx, d_mask));
    return hipGetLastError();
}

hipError_t launch_fields_morph(const uint8_t* d_src, uint8_t* d_dst, int H, int W, int r, int erode, int column, hipStream_t st) {
    if (!d_src || !d_dst || d_src == d_dst || bad_image(H, W) || r < 1 || r > 8) return hipErrorInvalidValue;
    const uint32_t G = groups(W);
    const int grid = stride_grid((size_t)H * G, 1 << 16, GF_DISPLAY);
    if (column)
        hipLaunchKernelGGL(fields_morph_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, d_src, d_dst, (uint32_t)H, (uint32_t)W, G, r, erode,
                           vec_of(W, d_src, d_dst));
    else
        hipLaunchKernelGGL(fields_morph_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, d_src, d_dst, (uint32_t)H, (uint32_t)W, G, r, erode,
                           vec_of(W, d_src, d_dst));
    return hipGetLastError();
}

hipError_t launch_fields_local(const uint8_t* d_mask, int* d_parent, uint32_t* d_size, int H, int W, int conn, hipStream_t st) {
    if (!d_mask || !d_parent || !d_size || bad_image(H, W) || (conn != 4 && conn != 8)) return hipErrorInvalidValue;
    const long long ntiles = (long long)tiles_of(H) * tiles_of(W);
    const int grid = capped_grid((int)(ntiles < 16384 ? ntiles : 16384), ntiles, GF_DISPLAY);
    hipLaunchKernelGGL(fields_local_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_mask, d_parent, d_size, (uint32_t)H, (uint32_t)W, tiles_of(W),
                       (uint32_t)ntiles, conn == 8);
    return hipGetLastError();
}

hipError_t launch_fields_border(int* d_parent, int H, int W, int conn, hipStream_t st) {
    if (!d_parent || bad_image(H, W) || (conn != 4 && conn != 8)) return hipErrorInvalidValue;
    const size_t nh = (size_t)(tiles_of(H) - 1) * W, nv = (size_t)(tiles_of(W) - 1) * H;
    if (nh + nv == 0) return hipSuccess;                          // one tile: no line to cross
    const int grid = stride_grid(nh + nv, 1 << 16, GF_DISPLAY);
    hipLaunchKernelGGL(fields_border_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_parent, (uint32_t)H, (uint32_t)W, nh, nh + nv, conn == 8);
    return hipGetLastError();
}

hipError_t launch_fields_flatten(int* d_parent, uint32_t* d_size, int H, int W, hipStream_t st) {
    if (!d_parent || !d_size || bad_image(H, W)) return hipErrorInvalidValue;
    const size_t N = (size_t)H * W;
    const int grid = stride_grid(N, 1 << 18, GF_DISPLAY);
    hipLaunchKernelGGL(fields_flatten_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_parent, d_size, N);
    return hipGetLastError();
}

size_t fields_chunks(int H, int W) { return ((size_t)H * W + kChunk - 1) / kChunk; }

hipError_t launch_fields_count(const int* d_parent, const uint32_t* d_size, int H, int W, uint32_t min_pixels, uint32_t* d_sums, hipStream_t st) {
    if (!d_parent || !d_size || !d_sums || bad_image(H, W) || min_pixels < 1) return hipErrorInvalidValue;
    const long long nchunks = (long long)fields_chunks(H, W);
    const int grid = capped_grid((int)(nchunks < 65536 ? nchunks : 65536), nchunks, GF_DISPLAY);
    hipLaunchKernelGGL(fields_count_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_parent, d_size, (size_t)H * W, min_pixels, (uint32_t)nchunks, d_sums);
    return hipGetLastError();
}

hipError_t launch_fields_scan(uint32_t* d_sums, int H, int W, unsigned long long* d_found, hipStream_t st) {
    if (!d_sums || !d_found || bad_image(H, W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fields_scan_kernel, dim3(1), dim3(256), 0, st, d_sums, (uint32_t)fields_chunks(H, W), d_found);
    return hipGetLastError();
}

hipError_t launch_fields_apply(const int* d_parent, uint32_t* d_size, int H, int W, uint32_t min_pixels, uint32_t Z, const uint32_t* d_sums,
                               unsigned long long* d_fields, hipStream_t st) {
    if (!d_parent || !d_size || !d_sums || !d_fields || bad_image(H, W) || min_pixels < 1 || Z < 1 || Z > 65535) return hipErrorInvalidValue;
    const long long nchunks = (long long)fields_chunks(H, W);
    const int grid = capped_grid((int)(nchunks < 65536 ? nchunks : 65536), nchunks, GF_DISPLAY);
    hipLaunchKernelGGL(fields_apply_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_parent, d_size, (size_t)H * W, min_pixels, (uint32_t)nchunks, d_sums, Z,
                       d_fields);
    return hipGetLastError();
}

hipError_t launch_fields_labels(const int* d_parent, const uint32_t* d_size, int H, int W, uint32_t Z, uint16_t* d_labels, unsigned long long* d_fields,
                                hipStream_t st) {
    if (!d_parent || !d_size || !d_labels || !d_fields || bad_image(H, W) || Z < 1 || Z > 65535) return hipErrorInvalidValue;
    const long long ntiles = (long long)tiles_of(H) * tiles_of(W);
    const int grid = capped_grid((int)(ntiles < 16384 ? ntiles : 16384), ntiles, GF_DISPLAY);
    hipLaunchKernelGGL(fields_labels_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_parent, d_size, (uint32_t)H, (uint32_t)W, tiles_of(W),
                       (uint32_t)ntiles, Z, d_labels, d_fields, vec_of(W, d_labels, d_labels));
    return hipGetLastError();
}

}  // namespace s2sr
