// Touching fields split: the kernels behind s2sr_fields_split_i16.  The mask, the components and the numbering are
// fields.hip's; here are the edge test, the capped squared Euclidean distance, the cores and the geodesic growth from them, all in
// integers.  The host side is engine_fields_split.hip; tests/fields_split_model.py restates the definition in numpy.
//
// Definition (include/s2sr.h has it in full):
//   interior  I = m minus the edge pixels; p is an edge pixel iff gx^2 + gy^2 > (8 n T)^2 for the 3 x 3 Sobel sums of the box sums B
//             of the index ((2 r + 1)^2 = n samples; a sample outside the image or on nodata is replaced by the box's centre, a
//             Sobel neighbour outside the image or on nodata by B(p))
//   distance  D2(p) = min(255^2, min |p - q|^2 over the pixels q of the image outside I) on I, 0 elsewhere
//   cores     per component of I: all of it when Dmax2 < core_px^2, else the pixels with D2 >= core_px^2 and 10^6 D2 >= core_q^2 Dmax2
//   markers   the components of the cores, keyed by their smallest linear index
//   growth    every pixel of I goes to the marker with the smallest (steps inside I, marker key); every pixel of m \ I to the owner
//             with the smallest (steps through m \ I from any pixel of I, that pixel's owner's key)
//   fields    a field is what one owner got; its key is ITS smallest linear index; sizes and numbering as in fields.hip
//
// Distance: a column pass writes g = the vertical distance to the nearest pixel outside I, capped at 255 (uint8): one thread per
// column and band of 256 rows, which starts 255 rows above its band with "nothing seen" and comes back from 255 rows below it.  A
// row pass then takes D2(x) = min over |dx| < g(x) of dx^2 + g(x + dx)^2: the bound is exact (a pixel outside I at vertical
// distance g(x) gives g(x)^2 at dx = 0), and with the cap no tap lies further than 254 columns away, so a workgroup stages 8 rows
// of 256 + 2 x 255 samples in LDS (6 KB) whatever W is.  Taps beyond the image are skipped.
//
// Growth: a pixel's state is one 64-bit word, steps << 32 | key, all ones = unreached.  The kernel is in pull form: a pixel that
// may change (it lies in `a` and not in `b`) takes the minimum of its own word and its neighbours' words plus one step; nobody
// else writes it, so there are no atomics, and an aligned 64-bit load or store does not tear.  A workgroup loads a 64 x 64 tile
// and a ring of one pixel into LDS, iterates the tile to its fixed point (Jacobi: new values in registers between two barriers),
// stores what changed and bumps a counter.  The host launches until a round changes nothing; from the second round on a tile runs only
// if it or one of its eight neighbours stored something in the round before.  Every word ever stored is the
// length and key of a real path, words only decrease, and a round that stores nothing read settled words only, so the state then
// satisfies w(p) <= w(n) + 1 along every edge: it is the least pair of every pixel, whatever order the workgroups ran in.
#include "s2sr_internal.h"

namespace s2sr {

namespace {

constexpr int kTile = 64;
constexpr int kCap = 255;                                        // the distance cap, pixels
constexpr int kBand = 256;                                       // rows per thread of the column pass
constexpr int kSeg = 256, kSegRows = 8;                          // the row pass: pixels and rows per workgroup
constexpr unsigned long long kFar = ~0ull;                       // an unreached growth word
constexpr unsigned long long kStep = 1ull << 32;

inline bool bad_image(int H, int W) { return H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL; }
inline uint32_t tiles_of(int n) { return ((uint32_t)n + kTile - 1) / kTile; }

__device__ __forceinline__ unsigned long long coherent64(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the edge test ---------------------------------------------------------------------------------------------------------------------
// One workgroup per 64 x 64 tile: the index with a halo of r + 1 in LDS (-32768 also stands for "outside the image": both are
// replaced alike), the box sums with a halo of 1 behind it (|B| <= 81 * 32767 < 2^22), then the Sobel in int64.
__global__ void __launch_bounds__(256) fsplit_edge_kernel(const int16_t* __restrict__ idx, const uint8_t* __restrict__ m, uint8_t* __restrict__ interior,
                                                          uint32_t H, uint32_t W, uint32_t tiles_x, uint32_t ntiles, int r, long long limit) {
    __shared__ int16_t S[(kTile + 10) * (kTile + 10)];
    __shared__ int B[(kTile + 2) * (kTile + 2)];
    const int halo = r + 1, sw = kTile + 2 * halo, bw = kTile + 2;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
        const int y0 = (int)(ty * kTile), x0 = (int)(tx * kTile);
        for (int i = threadIdx.x; i < sw * sw; i += 256) {
            const int y = y0 - halo + i / sw, x = x0 - halo + i % sw;
            S[i] = y >= 0 && y < (int)H && x >= 0 && x < (int)W ? idx[(size_t)y * W + x] : (int16_t)-32768;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < bw * bw; i += 256) {
            const int by = i / bw, bx = i % bw;                    // B's (by, bx) is S's (by + r, bx + r)
            const int c = S[(by + r) * sw + bx + r];
            int sum = 0;
            if (c != -32768) {
                for (int dy = -r; dy <= r; ++dy)
                    for (int dx = -r; dx <= r; ++dx) {
                        const int v = S[(by + r + dy) * sw + bx + r + dx];
                        sum += v == -32768 ? c : v;
                    }
            }
            B[i] = sum;                                            // (unused where the centre is no data)
        }
        __syncthreads();
        for (int i = threadIdx.x; i < kTile * kTile; i += 256) {
            const int ly = i >> 6, lx = i & 63;
            const uint32_t y = (uint32_t)y0 + ly, x = (uint32_t)x0 + lx;
            if (y >= H || x >= W) continue;
            const size_t p = (size_t)y * W + x;
            uint8_t keep = m[p];
            if (keep) {                                            // m holds no nodata pixel
                const int b = B[(ly + 1) * bw + lx + 1];
                auto nb = [&](int dy, int dx) -> long long {
                    const bool data = S[(ly + halo + dy) * sw + lx + halo + dx] != -32768;
                    return data ? B[(ly + 1 + dy) * bw + lx + 1 + dx] : b;
                };
                const long long gx = (nb(-1, 1) + 2 * nb(0, 1) + nb(1, 1)) - (nb(-1, -1) + 2 * nb(0, -1) + nb(1, -1));
                const long long gy = (nb(1, -1) + 2 * nb(1, 0) + nb(1, 1)) - (nb(-1, -1) + 2 * nb(-1, 0) + nb(-1, 1));
                if (gx * gx + gy * gy > limit) keep = 0;
            }
            interior[p] = keep;
        }
        __syncthreads();                                         // the next tile's samples come behind this one's reads
    }
}

// ---- the distance ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fsplit_column_kernel(const uint8_t* __restrict__ interior, uint8_t* __restrict__ g, uint32_t H, uint32_t W,
                                                            uint32_t bands) {
    const size_t items = (size_t)bands * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const uint32_t b = (uint32_t)(i / W), x = (uint32_t)(i - (size_t)b * W);
        const uint32_t ya = b * kBand, yb = ya + kBand < H ? ya + kBand : H;                    // the band [ya, yb)
        int c = kCap;                                              // nothing outside I seen yet
        for (uint32_t y = ya > (uint32_t)kCap ? ya - kCap : 0u; y < yb; ++y) {
            c = interior[(size_t)y * W + x] ? (c < kCap ? c + 1 : kCap) : 0;
            if (y >= ya) g[(size_t)y * W + x] = (uint8_t)c;
        }
        c = kCap;
        const uint32_t ye = yb + kCap < H ? yb + kCap : H;
        for (uint32_t y = ye; y-- > ya;) {
            c = interior[(size_t)y * W + x] ? (c < kCap ? c + 1 : kCap) : 0;
            if (y < yb && c < (int)g[(size_t)y * W + x]) g[(size_t)y * W + x] = (uint8_t)c;
        }
    }
}

__global__ void __launch_bounds__(256) fsplit_row_kernel(const uint8_t* __restrict__ g, uint16_t* __restrict__ d2, uint32_t H, uint32_t W, uint32_t segs,
                                                         uint32_t items) {
    constexpr int kRowLds = kSeg + 2 * kCap;                       // 766
    __shared__ uint8_t S[kSegRows * kRowLds];
    for (uint32_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t rg = it / segs, sg = it - rg * segs;
        const uint32_t y0 = rg * kSegRows;
        const long long xs = (long long)sg * kSeg - kCap;            // the image column of S's column 0
        for (int i = threadIdx.x; i < kSegRows * kRowLds; i += 256) {
            const uint32_t y = y0 + i / kRowLds;
            const long long x = xs + i % kRowLds;
            S[i] = y < H && x >= 0 && x < (long long)W ? g[(size_t)y * W + (size_t)x] : (uint8_t)0;          // (never read beyond the image)
        }
        __syncthreads();
        const uint32_t x = sg * kSeg + threadIdx.x;
        if (x < W) {
            for (int ry = 0; ry < kSegRows; ++ry) {
                const uint32_t y = y0 + ry;
                if (y >= H) break;
                const uint8_t* row = S + ry * kRowLds + kCap + threadIdx.x;
                const int gc = row[0];
                int best = gc * gc;                                 // dx = 0; 0 outside I
                const int left = (int)x < gc - 1 ? (int)x : gc - 1, right = (int)(W - 1 - x) < gc - 1 ? (int)(W - 1 - x) : gc - 1;
                for (int dx = 1; dx <= left && dx * dx < best; ++dx) {
                    const int v = row[-dx], c = dx * dx + v * v;
                    best = c < best ? c : best;
                }
                for (int dx = 1; dx <= right && dx * dx < best; ++dx) {
                    const int v = row[dx], c = dx * dx + v * v;
                    best = c < best ? c : best;
                }
                d2[(size_t)y * W + x] = (uint16_t)best;             // <= 255^2: g is capped
            }
        }
        __syncthreads();
    }
}

// ---- the cores -------------------------------------------------------------------------------------------------------------------------
// dmax (zeroed by the caller) gets, at every root of I's components, the largest D2 of the component: a maximum, whatever order the
// atomics land in.  Most pixels of a wide field sit at the cap and find it there already.
__global__ void __launch_bounds__(256) fsplit_dmax_kernel(const int* __restrict__ parent, const uint16_t* __restrict__ d2, uint32_t* __restrict__ dmax, size_t N) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        const int root = parent[i];
        if (root < 0) continue;
        const uint32_t d = d2[i];
        if (d > __hip_atomic_load(dmax + root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dmax + root, d);
    }
}

__global__ void __launch_bounds__(256) fsplit_core_kernel(const int* __restrict__ parent, const uint16_t* __restrict__ d2, const uint32_t* __restrict__ dmax,
                                                          uint8_t* __restrict__ cores, size_t N, uint32_t core_q2, uint32_t core_px2) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        const int root = parent[i];
        uint8_t c = 0;
        if (root >= 0) {
            const unsigned long long d = d2[i], top = dmax[root];
            c = top < core_px2 || (d >= core_px2 && 1000000ull * d >= (unsigned long long)core_q2 * top);
        }
        cores[i] = c;
    }
}

// ---- the growth ------------------------------------------------------------------------------------------------------------------------
// seeds: word = the marker's key on a core pixel (parent: the roots of the cores' components), unreached elsewhere
__global__ void __launch_bounds__(256) fsplit_seed_kernel(const int* __restrict__ parent, unsigned long long* __restrict__ word, size_t N) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        const int root = parent[i];
        word[i] = root < 0 ? kFar : (unsigned long long)(uint32_t)root;
    }
}
// between the two growths: every owned pixel (all of them lie in I) becomes a source at step 0
__global__ void __launch_bounds__(256) fsplit_restart_kernel(unsigned long long* __restrict__ word, size_t N) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        const unsigned long long w = word[i];
        if (w != kFar && (w >> 32)) word[i] = w & 0xffffffffull;
    }
}

// One round.  A pixel may change iff a[p] and not b[p] (b may be null).  *changed counts the tiles that stored something.  A tile
// that stores marks itself and its eight neighbours in dirty_out; with dirty_in (the round before's marks; null: every tile) a tile
// that nobody marked is passed over: neither it nor its ring has changed since it last reached its fixed point.  (A tile that read
// a neighbour's word of the round before was marked by that neighbour's store.)
__global__ void __launch_bounds__(256) fsplit_grow_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, unsigned long long* __restrict__ word,
                                                          uint32_t H, uint32_t W, uint32_t tiles_x, uint32_t ntiles, int conn8, uint32_t* __restrict__ changed,
                                                          const uint8_t* __restrict__ dirty_in, uint8_t* __restrict__ dirty_out) {
    constexpr int lw = kTile + 2;
    __shared__ unsigned long long L[lw * lw];
    __shared__ unsigned long long live[kTile];                     // per tile row: the pixels that may change
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        if (dirty_in && !dirty_in[t]) continue;                    // (one byte for the whole workgroup: no barrier is left out by some)
        const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
        const int y0 = (int)(ty * kTile), x0 = (int)(tx * kTile);
        int any = 0;
        for (uint32_t ly = wave; ly < (uint32_t)kTile; ly += 4) {
            const uint32_t y = (uint32_t)y0 + ly, x = (uint32_t)x0 + lane;
            bool on = false;
            if (y < H && x < W) {
                const size_t p = (size_t)y * W + x;
                on = a[p] != 0 && !(b && b[p]);
            }
            const unsigned long long bits = __ballot(on);
            if (lane == 0) live[ly] = bits;
            any |= bits != 0;
        }
        if (!__syncthreads_or(any)) continue;                      // nothing here may change (the barrier also guards `live`)
        for (int i = threadIdx.x; i < lw * lw; i += 256) {
            const int y = y0 - 1 + i / lw, x = x0 - 1 + i % lw;
            L[i] = y >= 0 && y < (int)H && x >= 0 && x < (int)W ? coherent64(word + (size_t)y * W + x) : kFar;
        }
        __syncthreads();
        unsigned long long first[16], cur[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t ly = wave + 4 * k;
            first[k] = cur[k] = L[(ly + 1) * lw + lane + 1];
        }
        for (;;) {
            int moved = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t ly = wave + 4 * k;
                if (!((live[ly] >> lane) & 1)) continue;
                const unsigned long long* c = L + (ly + 1) * lw + lane + 1;
                unsigned long long best = c[-lw] < c[lw] ? c[-lw] : c[lw];
                best = c[-1] < best ? c[-1] : best;
                best = c[1] < best ? c[1] : best;
                if (conn8) {
                    best = c[-lw - 1] < best ? c[-lw - 1] : best;
                    best = c[-lw + 1] < best ? c[-lw + 1] : best;
                    best = c[lw - 1] < best ? c[lw - 1] : best;
                    best = c[lw + 1] < best ? c[lw + 1] : best;
                }
                if (best != kFar && best + kStep < cur[k]) {
                    cur[k] = best + kStep;
                    moved = 1;
                }
            }
            __syncthreads();                                     // every read of this turn is done
#pragma unroll
            for (int k = 0; k < 16; ++k) L[(wave + 4 * k + 1) * lw + lane + 1] = cur[k];
            if (!__syncthreads_or(moved)) break;
        }
        int stored = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (cur[k] != first[k]) {                              // only a live pixel moves, and those lie inside the image
                const size_t p = (size_t)((uint32_t)y0 + wave + 4 * k) * W + (uint32_t)x0 + lane;
                __hip_atomic_store(word + p, cur[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                stored = 1;
            }
        }
        if (__syncthreads_or(stored)) {
            if (threadIdx.x < 9) {
                const int ny = (int)ty + (int)(threadIdx.x / 3) - 1, nx = (int)tx + (int)(threadIdx.x % 3) - 1;
                if (ny >= 0 && ny < (int)(ntiles / tiles_x) && nx >= 0 && nx < (int)tiles_x) dirty_out[(uint32_t)ny * tiles_x + (uint32_t)nx] = 1;
            }
            if (threadIdx.x == 0) atomicAdd(changed, 1u);
        }
    }
}

// ---- the remap -------------------------------------------------------------------------------------------------------------------------
// The lanes of a wave that hold the same owner as the first live lane go together: one atomic per run of a row inside a field.
// key[owner] (all ones from the caller) = the smallest linear index the owner holds: i ascends with the lane, so the run's first
// lane holds the run's minimum.
__global__ void __launch_bounds__(256) fsplit_key_kernel(const unsigned long long* __restrict__ word, uint32_t* __restrict__ key, size_t N) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t span = ((N + 255) / 256) * 256;                   // whole waves take every turn: the ballots need them
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < span; i += (size_t)gridDim.x * 256) {
        const unsigned long long w = i < N ? word[i] : kFar;
        const uint32_t owner = (uint32_t)w;
        unsigned long long todo = __ballot(w != kFar);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const uint32_t o = (uint32_t)__shfl((int)owner, lead);
            const unsigned long long same = __ballot(w != kFar && owner == o) & todo;
            if ((int)lane == lead) atomicMin(key + o, (uint32_t)i);
            todo &= ~same;
        }
    }
}
// parent = the key of the pixel's owner, -1 for a pixel nobody owns
__global__ void __launch_bounds__(256) fsplit_parent_kernel(const unsigned long long* __restrict__ word, const uint32_t* __restrict__ key,
                                                            int* __restrict__ parent, size_t N) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        const unsigned long long w = word[i];
        parent[i] = w == kFar ? -1 : (int)key[(uint32_t)w];
    }
}
// size (zeroed by the caller) at a field's key = its pixels
__global__ void __launch_bounds__(256) fsplit_size_kernel(const int* __restrict__ parent, uint32_t* __restrict__ size, size_t N) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t span = ((N + 255) / 256) * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < span; i += (size_t)gridDim.x * 256) {
        const int root = i < N ? parent[i] : -1;
        unsigned long long todo = __ballot(root >= 0);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int r = __shfl(root, lead);
            const unsigned long long same = __ballot(root == r) & todo;
            if ((int)lane == lead) atomicAdd(size + r, (uint32_t)__popcll(same));
            todo &= ~same;
        }
    }
}

}  // namespace

hipError_t launch_fsplit_edge(const int16_t* d_idx, const uint8_t* d_m, uint8_t* d_interior, int H, int W, int edge, int edge_r, hipStream_t st) {
    if (!d_idx || !d_m || !d_interior || d_m == d_interior || bad_image(H, W) || edge < 1 || edge > 32767 || edge_r < 0 || edge_r > 4)
        return hipErrorInvalidValue;
    const long long n = (2 * edge_r + 1) * (2 * edge_r + 1), lim = 8 * n * edge;
    const long long ntiles = (long long)tiles_of(H) * tiles_of(W);
    const int grid = capped_grid((int)(ntiles < 16384 ? ntiles : 16384), ntiles, GF_DISPLAY);
    hipLaunchKernelGGL(fsplit_edge_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_idx, d_m, d_interior, (uint32_t)H, (uint32_t)W, tiles_of(W),
                       (uint32_t)ntiles, edge_r, lim * lim);
    return hipGetLastError();
}

hipError_t launch_fsplit_distance(const uint8_t* d_interior, uint8_t* d_g, uint16_t* d_d2, int H, int W, hipStream_t st) {
    if (!d_interior || !d_g || !d_d2 || bad_image(H, W)) return hipErrorInvalidValue;
    const uint32_t bands = ((uint32_t)H + kBand - 1) / kBand;
    int grid = stride_grid((size_t)bands * W, 1 << 16, GF_DISPLAY);
    hipLaunchKernelGGL(fsplit_column_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_interior, d_g, (uint32_t)H, (uint32_t)W, bands);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t segs = ((uint32_t)W + kSeg - 1) / kSeg;
    const long long items = (long long)segs * (((uint32_t)H + kSegRows - 1) / kSegRows);       // < 2^31 / 2048 + H + W
    grid = capped_grid((int)(items < 65536 ? items : 65536), items, GF_DISPLAY);
    hipLaunchKernelGGL(fsplit_row_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_g, d_d2, (uint32_t)H, (uint32_t)W, segs, (uint32_t)items);
    return hipGetLastError();
}

hipError_t launch_fsplit_cores(const int* d_parent, const uint16_t* d_d2, uint32_t* d_dmax, uint8_t* d_cores, int H, int W, int core_q, int core_px,
                               hipStream_t st) {
    if (!d_parent || !d_d2 || !d_dmax || !d_cores || bad_image(H, W) || core_q < 1 || core_q > 1000 || core_px < 0 || core_px > 255)
        return hipErrorInvalidValue;
    const size_t N = (size_t)H * W;
    hipError_t e = hipMemsetAsync(d_dmax, 0, N * 4, st);
    if (e != hipSuccess) return e;
    const int grid = stride_grid(N, 1 << 18, GF_DISPLAY);
    hipLaunchKernelGGL(fsplit_dmax_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_parent, d_d2, d_dmax, N);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(fsplit_core_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_parent, d_d2, d_dmax, d_cores, N, (uint32_t)(core_q * core_q),
                       (uint32_t)(core_px * core_px));
    return hipGetLastError();
}

hipError_t launch_fsplit_seed(const int* d_parent, unsigned long long* d_word, int H, int W, hipStream_t st) {
    if (!d_parent || !d_word || bad_image(H, W)) return hipErrorInvalidValue;
    const size_t N = (size_t)H * W;
    const int grid = stride_grid(N, 1 << 18, GF_DISPLAY);
    hipLaunchKernelGGL(fsplit_seed_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_parent, d_word, N);
    return hipGetLastError();
}

hipError_t launch_fsplit_restart(unsigned long long* d_word, int H, int W, hipStream_t st) {
    if (!d_word || bad_image(H, W)) return hipErrorInvalidValue;
    const size_t N = (size_t)H * W;
    const int grid = stride_grid(N, 1 << 18, GF_DISPLAY);
    hipLaunchKernelGGL(fsplit_restart_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_word, N);
    return hipGetLastError();
}

size_t fsplit_tiles(int H, int W) { return (size_t)tiles_of(H) * tiles_of(W); }

hipError_t launch_fsplit_grow(const uint8_t* d_a, const uint8_t* d_b, unsigned long long* d_word, int H, int W, int conn, uint32_t* d_changed,
                              const uint8_t* d_dirty_in, uint8_t* d_dirty_out, hipStream_t st) {
    if (!d_a || !d_word || !d_changed || !d_dirty_out || d_dirty_in == d_dirty_out || bad_image(H, W) || (conn != 4 && conn != 8)) return hipErrorInvalidValue;
    const long long ntiles = (long long)tiles_of(H) * tiles_of(W);
    const int grid = capped_grid((int)(ntiles < 65536 ? ntiles : 65536), ntiles, GF_DISPLAY);
    hipLaunchKernelGGL(fsplit_grow_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_a, d_b, d_word, (uint32_t)H, (uint32_t)W, tiles_of(W),
                       (uint32_t)ntiles, conn == 8, d_changed, d_dirty_in, d_dirty_out);
    return hipGetLastError();
}

hipError_t launch_fsplit_remap(const unsigned long long* d_word, int* d_parent, uint32_t* d_size, int H, int W, hipStream_t st) {
    if (!d_word || !d_parent || !d_size || bad_image(H, W)) return hipErrorInvalidValue;
    const size_t N = (size_t)H * W;
    hipError_t e = hipMemsetAsync(d_size, 0xff, N * 4, st);          // the keys: all ones is above every linear index
    if (e != hipSuccess) return e;
    const int grid = stride_grid(N, 1 << 18, GF_DISPLAY);
    hipLaunchKernelGGL(fsplit_key_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_word, d_size, N);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(fsplit_parent_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_word, d_size, d_parent, N);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_size, 0, N * 4, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(fsplit_size_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_parent, d_size, N);
    return hipGetLastError();
}

}  // namespace s2sr
