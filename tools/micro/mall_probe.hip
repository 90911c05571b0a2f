// Probe of the Infinity Cache (256 MB, memory side) on MI355X: (A) streaming-read bandwidth against the size of the buffer that is read
// over and over -- where the cache stops serving it; (B) are freshly WRITTEN bytes retained: a buffer is written by one kernel and then read
// once by another, over and over -- the read's bandwidth against (A) for the same size; (C) the control: the same with 512 MB of other
// writes between the write and the read.  Decides whether a schedule that keeps a launch group's dense tensor (100 - 200 MB, written layer by
// layer) cache-resident can be fed at the rate profiles/r05_mfma_ceiling.txt measured from a read-only source.
// (D) does the DIRECTION of the next launch matter: a buffer larger than the cache is swept front to back like a conv launch, then
// re-read front to back or back to front (profiles/serpentine_mall_probe.txt).
//   hipcc -O3 --offload-arch=gfx950 tools/micro/mall_probe.hip -o /tmp/mall_probe && /tmp/mall_probe      (`mall_probe D`: D alone)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

__global__ void __launch_bounds__(256) read_kernel(const uint4* __restrict__ src, size_t n16, uint32_t* __restrict__ sink) {
    uint32_t acc = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {            // four independent 16-B loads in flight per lane
        const uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z ^ d.w;
    }
    for (; i < n16; i += stride) { const uint4 a = src[i]; acc ^= a.x ^ a.y ^ a.z ^ a.w; }
    if (acc == 0x12345678u) sink[0] = acc;                      // (keeps the loads alive)
}

__global__ void __launch_bounds__(256) write_kernel(uint4* __restrict__ dst, size_t n16, uint32_t seed) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const uint32_t v = (uint32_t)i * 2654435761u + seed;
        dst[i] = make_uint4(v, v ^ 0x9e3779b9u, v + 0x7f4a7c15u, ~v);
    }
}

// Protocol D, kernel 1: one conv launch's traffic -- the whole buffer is read front to back and every sixth 4-KB block of it is rewritten.
__global__ void __launch_bounds__(256) sweep_kernel(uint4* __restrict__ buf, size_t n16, uint32_t seed, uint32_t* __restrict__ sink) {
    uint32_t acc = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const uint4 a = buf[i];
        acc ^= a.x ^ a.y ^ a.z ^ a.w;
        if ((i >> 8) % 6 == 0) buf[i] = make_uint4(a.x + seed, a.y, a.z, a.w);
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

// Protocol D, kernel 2: the next launch's reads in four rounds of n16 / 4; backwards = the rounds in the opposite order (within a round the
// workgroups run side by side, as the patches of one round of a conv launch do).
__global__ void __launch_bounds__(256) rounds_kernel(const uint4* __restrict__ src, size_t n16, int backwards, uint32_t* __restrict__ sink) {
    uint32_t acc = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x, per = n16 / 4;
    for (int r = 0; r < 4; ++r) {
        const uint4* p = src + (size_t)(backwards ? 3 - r : r) * per;
        size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        for (; i + 3 * stride < per; i += 4 * stride) {
            const uint4 a = p[i], b = p[i + stride], c = p[i + 2 * stride], d = p[i + 3 * stride];
            acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z ^ d.w;
        }
        for (; i < per; i += stride) { const uint4 a = p[i]; acc ^= a.x ^ a.y ^ a.z ^ a.w; }
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

static int cmp_double(const void* a, const void* b);

// D: does the direction of the next launch matter?  Kernel 1 sweeps F MB front to back; kernel 2 re-reads them (a) front to back, (b) back to
// front.  Every launch is timed alone; the two arms alternate so that drift hits both; median and min..max of kernel 2 over the repeats.
static void protocol_d(hipStream_t st, hipEvent_t e0, hipEvent_t e1, char* buf, uint32_t* sink, int grid) {
    const size_t MB = 1 << 20;
    const size_t fsizes[] = {200, 270, 335, 400, 670};
    const int reps = 15;
    printf("D: a front-to-back sweep (reads F, rewrites F/6), then F re-read in 4 rounds (a) front to back, (b) back to front; TB/s of the re-read,\n"
           "   median [min..max] of %d repeats, the arms alternating; last column the sweep itself\n", reps);
    for (size_t s : fsizes) {
        const size_t n16 = s * MB / 16;
        double tbs[2][reps], sweep_ms = 0;
        for (int r = -2; r < reps; ++r)
            for (int back = 0; back < 2; ++back) {
                float ms = 0;
                CHECK(hipEventRecord(e0, st));
                hipLaunchKernelGGL(sweep_kernel, dim3(grid), dim3(256), 0, st, (uint4*)buf, n16, (uint32_t)(r + 3), sink);
                CHECK(hipEventRecord(e1, st));
                CHECK(hipStreamSynchronize(st));
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) sweep_ms += ms;
                CHECK(hipEventRecord(e0, st));
                hipLaunchKernelGGL(rounds_kernel, dim3(grid), dim3(256), 0, st, (const uint4*)buf, n16, back, sink);
                CHECK(hipEventRecord(e1, st));
                CHECK(hipStreamSynchronize(st));
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) tbs[back][r] = (double)s * MB / (ms * 1e-3) / 1e12;
            }
        for (int back = 0; back < 2; ++back) qsort(tbs[back], reps, sizeof(double), cmp_double);
        printf("  %5zu MB  (a) %5.2f [%5.2f..%5.2f]   (b) %5.2f [%5.2f..%5.2f]   (b)/(a) %.3f   sweep %5.2f TB/s read\n", s,
               tbs[0][reps / 2], tbs[0][0], tbs[0][reps - 1], tbs[1][reps / 2], tbs[1][0], tbs[1][reps - 1], tbs[1][reps / 2] / tbs[0][reps / 2],
               (double)s * MB * 2 * reps / (sweep_ms * 1e-3) / 1e12);
        fflush(stdout);
    }
}

static int cmp_double(const void* a, const void* b) { const double x = *(const double*)a, y = *(const double*)b; return x < y ? -1 : x > y; }

int main(int argc, char** argv) {
    const bool only_d = argc > 1 && argv[1][0] == 'D';          // "mall_probe D": protocol D alone
    const size_t MB = 1 << 20, cap = 1024 * MB;
    char *buf, *other;
    uint32_t* sink;
    CHECK(hipMalloc(&buf, cap));
    CHECK(hipMalloc(&other, 512 * MB));
    CHECK(hipMalloc(&sink, 4));
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const int grid = 256 * 8;      // 8 workgroups of 256 per CU
    hipLaunchKernelGGL(write_kernel, dim3(grid), dim3(256), 0, st, (uint4*)buf, cap / 16, 1u);
    hipLaunchKernelGGL(write_kernel, dim3(grid), dim3(256), 0, st, (uint4*)other, 512 * MB / 16, 2u);
    CHECK(hipStreamSynchronize(st));
    if (only_d) { protocol_d(st, e0, e1, buf, sink, grid); return 0; }

    const size_t sizes[] = {8, 16, 32, 64, 100, 150, 200, 230, 256, 300, 400, 1024};
    printf("A: the same buffer read over and over (GB/s by size)\n");
    for (size_t s : sizes) {
        const size_t n16 = s * MB / 16;
        const int reps = (int)(20000 / s) + 4;                 // ~20 GB per measurement
        for (int r = 0; r < 3; ++r) hipLaunchKernelGGL(read_kernel, dim3(grid), dim3(256), 0, st, (const uint4*)buf, n16, sink);
        CHECK(hipEventRecord(e0, st));
        for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(read_kernel, dim3(grid), dim3(256), 0, st, (const uint4*)buf, n16, sink);
        CHECK(hipEventRecord(e1, st));
        CHECK(hipStreamSynchronize(st));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        printf("  %5zu MB  %8.1f GB/s  (%d passes, %.1f us each)\n", s, (double)s * MB * reps / (ms * 1e-3) / 1e9, reps, ms * 1e3 / reps);
        fflush(stdout);
    }

    const size_t wsizes[] = {32, 100, 200, 400};
    for (int variant = -1; variant < 2; ++variant) {
        printf(variant < 0 ? "A1: read, then read again, each launch timed alone (the protocol of B and C; first column the second read)\n"
               : variant == 0 ? "B: written by one kernel, then read once by another; read bandwidth (GB/s), write bandwidth (GB/s)\n"
                              : "C: the same with 512 MB of other writes between the write and the read\n");
        for (size_t s : wsizes) {
            const size_t n16 = s * MB / 16;
            const int reps = (int)(8000 / s) + 4;
            double rd_ms = 0, wr_ms = 0;
            for (int r = -2; r < reps; ++r) {
                CHECK(hipEventRecord(e0, st));
                if (variant < 0) hipLaunchKernelGGL(read_kernel, dim3(grid), dim3(256), 0, st, (const uint4*)buf, n16, sink);
                else hipLaunchKernelGGL(write_kernel, dim3(grid), dim3(256), 0, st, (uint4*)buf, n16, (uint32_t)r);
                CHECK(hipEventRecord(e1, st));
                CHECK(hipStreamSynchronize(st));
                float ms = 0;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) wr_ms += ms;
                if (variant == 1) hipLaunchKernelGGL(write_kernel, dim3(grid), dim3(256), 0, st, (uint4*)other, 512 * MB / 16, (uint32_t)r);
                CHECK(hipEventRecord(e0, st));
                hipLaunchKernelGGL(read_kernel, dim3(grid), dim3(256), 0, st, (const uint4*)buf, n16, sink);
                CHECK(hipEventRecord(e1, st));
                CHECK(hipStreamSynchronize(st));
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) rd_ms += ms;
            }
            printf("  %5zu MB  read %8.1f GB/s   %s %8.1f GB/s\n", s, (double)s * MB * reps / (rd_ms * 1e-3) / 1e9, variant < 0 ? "first read" : "write", (double)s * MB * reps / (wr_ms * 1e-3) / 1e9);
            fflush(stdout);
        }
    }
    protocol_d(st, e0, e1, buf, sink, grid);
    return 0;
}
