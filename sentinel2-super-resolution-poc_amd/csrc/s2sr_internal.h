// Internal declarations shared by the translation units of libs2sr.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <functional>
#include <mutex>
#include <vector>

#include "../../include/s2sr.h"
#include "conv_forms.h"   // Epilogue, ConvForm, the kernel-form tables and picks (host-only)

// The library carries only the kernel forms that run.  The ones the measurements buried (the row-Winograd trunk form, the fp16
// loader-wave form, the one-wave-per-SIMD tail convs, the 8-wave RDB path, the non-default fp8 conv1-4 forms, the upsample-on-load
// up-convs, every stamped build) are recorded in DESIGN.md section 9 and profiles/; their code is in git history.

namespace s2sr {

// ------------------------------------------------------------------------------------------
// The device gate.  While a stream captures a hipGraph, the runtime refuses device-wide operations from EVERY thread of the
// process (hipDeviceSynchronize, hipFree, legacy-stream hipMemcpy / hipMemset ...: "operation not permitted when stream is
// capturing") and voids the capture with them.  Handles are independent objects used from different threads (the x4 and the
// anime-6B engines under Starlette's pool, reference main.py:602,670-675), so one handle's workspace regrow met another's capture
// (found by tools/soak_jobs.py, r04).  Rule of this library: no legacy-stream call anywhere (copy_blocking / fill_blocking in
// engine.hip run on the handle's own stream), and every device-wide call goes through the wrappers below, which hold the same
// process-wide mutex the capture section holds.  Captures are ~1 ms of host work and device-wide calls are rare (allocation,
// regrow, teardown), so the gate costs nothing in steady state.
// ------------------------------------------------------------------------------------------
std::recursive_mutex& device_gate();
struct DeviceGate {
    std::lock_guard<std::recursive_mutex> lk;
    DeviceGate() : lk(device_gate()) {}
};
static inline hipError_t dev_sync() { DeviceGate g; return hipDeviceSynchronize(); }
// Red zones (redzone.h, redzone.hip; the diagnostic mode of s2sr_debug_redzone / S2SR_REDZONE): with a zone size Z > 0 every
// allocation is [Z patterned bytes | the caller's bytes | Z patterned bytes] and dev_free checks both zones before it frees.  Z is
// a multiple of 4096, so the pointer handed out keeps every alignment hipMalloc's has.  Off (the default), the cost is one atomic
// load here and one in dev_free; allocations made while the mode was off are freed as ever.
extern std::atomic<size_t> g_redzone_bytes;     // Z of the allocations made from now on
extern std::atomic<bool> g_redzone_ever;        // the mode has been on at some point: dev_free looks its pointer up
hipError_t redzone_malloc(void** p, size_t bytes, size_t zone);   // both with the device gate held
hipError_t redzone_free(void* p);
// Poison (redzone.h namespace poison, redzone.hip; the diagnostic mode of s2sr_debug_poison / S2SR_POISON): with a pattern in force
// dev_malloc and host_malloc fill the caller's bytes with it before they hand the pointer out, so nobody finds the zeros fresh memory
// reads as.  With and without zones; off (the default), the cost is one atomic load per allocation.
extern std::atomic<int> g_poison;               // 0 off, 1 all 0xFF, 2 position-dependent
hipError_t poison_device(void* p, size_t bytes, int pat);   // with the device gate held; on the red-zone I/O stream
void poison_host(void* p, size_t bytes, int pat);
template <class T> static inline hipError_t dev_malloc(T** p, size_t bytes) {
    DeviceGate g;
    const size_t z = g_redzone_bytes.load(std::memory_order_relaxed);
    const hipError_t e = z ? redzone_malloc((void**)p, bytes, z) : hipMalloc((void**)p, bytes);
    if (e != hipSuccess) return e;
    if (const int pat = g_poison.load(std::memory_order_relaxed)) {
        const hipError_t ep = poison_device(*p, bytes, pat);
        if (ep != hipSuccess) {                       // nothing half-poisoned is handed out
            (void)(g_redzone_ever.load(std::memory_order_relaxed) ? redzone_free(*p) : hipFree(*p));
            *p = nullptr;
            return ep;
        }
    }
    return e;
}
static inline hipError_t dev_free(void* p) {
    DeviceGate g;
    if (g_redzone_ever.load(std::memory_order_relaxed)) return redzone_free(p);
    return hipFree(p);
}
// a zone of `back` bytes behind the `bytes` of `plane`, a piece of the zoned allocation `parent` (the workspace planes)
hipError_t redzone_add_plane(void* parent, void* plane, size_t bytes, size_t back);
static inline hipError_t host_malloc(void** p, size_t bytes, unsigned flags) {
    DeviceGate g;
    const hipError_t e = hipHostMalloc(p, bytes, flags);
    if (e != hipSuccess) return e;
    if (const int pat = g_poison.load(std::memory_order_relaxed)) poison_host(*p, bytes, pat);
    return e;
}
static inline hipError_t host_free(void* p) { DeviceGate g; return hipHostFree(p); }

// ------------------------------------------------------------------------------------------
// Activation tensors in HBM: "blocked-16 with a physical zero halo".
//
//   fp16 tensor, C channels (C % 16 == 0):   [N][C/16][Hp][Wp][16]   -> 32 B per (block, pixel)
//   fp32 trunk tensors, 64 channels:         [N][8]   [Hp][Wp][8]    -> 32 B per (block, pixel)
//   element (n, y, x) of block b sits at ((n*NB + b)*Hp + y+1)*Wp + x+1  (units of 32 B)
//   with Hp = roundup(H,32)+2, Wp = roundup(W,32)+2.
//
// Why: the conv kernel consumes 16 input channels per pipeline stage.  With one plane per
// 16-channel block a slab row (34 pixels) is 1088 CONTIGUOUS bytes, so every LDS-DMA
// instruction (64 lanes x 16 B) reads 8 whole 128-B lines instead of 32 partial ones (the
// NHWC layout of the first version cost ~20 % in the loader and produced multi-microsecond
// stalls), and every epilogue store instruction writes 1 KiB contiguously.
// Kernels only store to pixels with y<H, x<W, so halo and round-up slack stay zero from the
// allocation-time memset: that IS the zero padding of the reference convs
// (cnn_super_resolution.py:78-82) and it removes every bounds check from the loader.
// The channel concatenation of the dense block (torch.cat, cnn_super_resolution.py:87-90) is
// just "the first k blocks of the dense tensor": [x(4 blocks) | x1(2) | x2(2) | x3(2) | x4(2)].
// ------------------------------------------------------------------------------------------
static inline int roundup32(int v) { return (v + 31) & ~31; }
static inline int padded(int v) { return roundup32(v) + 2; }

struct ConvParams {
    const char* src;         // first input block of image 0 (fp16 blocked tensor)
    uint64_t src_img;        // bytes between images of src
    int32_t nstage;          // pipeline stages per patch = nseg * seg_len
    // Split-operand ("hp") convs run the K loop over segments of seg_len stages that all accumulate
    // into the same fp32 accumulator.  Bit s of seg_lo_mask says segment s reads the src_lo tensor.
    //   conv_first: (x, w_hi) (x, w_lo), both fp16 (x is an exact integer);
    //   cin-64 convs (the split forms of ConvForm): 4 fp16 stages (x_hi, w_hi), then the 4 e4m3 planes of src_lo
    //   [x_lo*2^11 p0, p1, x_hi p0, p1] against [w_hi, w_hi, w_lo*2^11, w_lo*2^11] on the fp8 MFMA.
    // Plain convs: seg_len == nstage, mask 0.
    const char* src_lo;      // second operand tensor (same padded geometry as src: fp16 lo blocks or e4m3 planes), or null
    uint64_t lo_img;         // bytes between images of src_lo
    int32_t seg_len;
    int32_t seg_lo_mask;
    const void* wpack;       // packed fp16 weights (pack_conv_weights)
    const float* bias;       // [64] fp32, zero padded
    int32_t N, H, W;         // output logical dims (images in this launch)
    int32_t Hp, Wp;          // padded dims at output resolution
    int32_t sHp, sWp;        // padded dims of the source tensor (== Hp,Wp unless upsample-on-load)
    int32_t tilesX, tilesY;  // filled by the launcher
    char* dst;               // first OUTPUT block of image 0 (fp16 blocked tensor)
    uint64_t dst_img;        // bytes between images of dst
    char* T;                 // 'lo' OUTPUT tensor: fp16 blocked-16, 4 blocks, image stride 4 blocks.  conv_first / conv5:
                             // the trunk lo (trunk = x + lo); hp convs: the 4 e4m3 planes of their 64-channel output
    float* R; float* F;      // fp32 blocked-8 skip tensors (RRDB input, global skip), 8 blocks
    float* out_f32;          // EPI_LAST / EPI_DEBUG: [N,cout,H,W] fp32 (may be null)
    uint8_t* out_u8;         // EPI_LAST: [N,H,W,3] u8 (may be null)
    int32_t cout;            // real output channels (EPI_LAST: 3; EPI_DEBUG: Cout)
    int32_t act;             // EPI_DEBUG: apply lrelu
    int32_t fold_lo;         // EPI_LAST: couts 8..8+cout-1 carry w_lo (pack_conv_weights fold): out[c] = acc[c] + acc[8+c]
    float in_scale;          // EPI_FIRST: 1/255 (inputs are fed as exact integers 0..255)
    // fp8 trunk mode (S2SR_PREC_FP8, conv_trunk.hip conv_trunk_f8): src / dst are e4m3 PLANES of 32 channels (32 B per
    // pixel, the geometry of an fp16 block-16 plane); nstage = planes per patch padded to an even count, seg_len = real
    // planes (a phantom plane re-reads plane 0 against zero weights); the trunk itself is carried in fp16:
    const char* xh_in;       // conv5: trunk x (fp16 blocked-16, 4 blocks) -- the residual operand
    const char* xh_skip;     // conv5 of rdb3: the RRDB's input x (fp16, 4 blocks).  Also used by conv_trunk_f16 (fp16 modes):
                             // there the RRDB skip is the fp16 PAIR (xh_skip, lo_skip) of the trunk at the RRDB's input, read
                             // in place of the fp32 R tensor (-256 B per pixel: no R store, two 8-B halves instead of 16 B)
    const char* lo_skip;     // ... its lo half (fp16, 4 blocks, image stride as T)
    char* xh_out;            // conv5: new trunk x (fp16, 4 blocks); may alias xh_skip (same lane reads, then writes)
    uint64_t xh_img;         // bytes between images of the three
    const int32_t* wscale;   // [64] E8M0 bytes 127 - k_co of the per-output-channel weight scales 2^k_co
    int32_t x_exp, g_exp;    // activation scales: x planes hold e4m3(x * 2^x_exp), growth planes e4m3(x_k * 2^g_exp)
    int32_t f8_form;         // unused (kept so that every kernel argument stays at its offset)
    int32_t f16_form;        // reserved, always 0 (the form switches travel as FormSwitches, conv_forms.h; kept like f8_form)
    int32_t tail_form;       // reserved, always 0
    int32_t lo_exp;          // conv_trunk_f16 conv5: the trunk's lo half is stored as e4m3(lo * 2^lo_exp) planes (xh_in, T, lo_skip)
    // Window mosaics (the AOI path, engine.hip forward_dev): equal-size windows of `_tile_process` (cnn_super_resolution.py:249-257) laid
    // out on a grid inside ONE image with a single zero row / column between neighbours -- the conv zero padding of both, at
    // every layer, because no launch ever stores to a separator pixel: at the scale of the coordinates the epilogue works in,
    // (y, x) is live iff y % mos_py < mos_ry and x % mos_px < mos_rx (period = window + 1, real extent = window).  0 = off.
    // 276-pixel windows then cost 280 x 280 of patch area instead of 288 x 288.
    int32_t mos_py, mos_ry, mos_px, mos_rx;
    uint32_t mos_my, mos_mx;             // floor(2^32 / mos_py) + 1, floor(2^32 / mos_px) + 1 (patch_live); 0: take the modulo route
    int32_t mos_kx, mos_ky, mos_count;   // EPI_LAST: grid of a mosaic and the number of windows in this launch: window t = (n * ky + wy) * kx + wx
                                         // is written as image t of [count, ry, rx]; slots past the count are not written
    char* trash;             // >= 4 KiB scratch: out-of-image lanes park their (unconditional) stores here
    const float* slope;      // EPI_PRELU / EPI_CFIRST (SRVGGNetCompact): [64] fp32 PReLU slopes, one per output channel, next to `bias`.
                             // (Takes the slot of the retired `trace` pointer, so the struct keeps its size and every kernel
                             // argument its offset: the RRDB kernels compile to the parent's instructions.)
                             // EPI_CLAST takes the packed input (fp16 blocked-16, one block: channels 0..2 = the pixel's exact 0..255
                             // values, for the nearest-x4 base) as src_lo / lo_img: the loader never reads src_lo of a plain conv
    int32_t dbg;                 // bit 0: walk the launch's patches back to front (tile -> ntiles - 1 - tile; same patches, same bytes: the
                                 // launch order of engine.hip's schedules, engine_internal.h serp_bit).  Took an unused slot: no argument moved
};

// is output pixel (y, x) of this launch one the reference writes (inside the image, and not a mosaic separator)?
__device__ __forceinline__ bool px_live(const ConvParams& p, int y, int x) {
    bool ok = (y < p.H) && (x < p.W);
    if (p.mos_py) ok = ok && (y % p.mos_py < p.mos_ry) && (x % p.mos_px < p.mos_rx);
    return ok;
}
// The same predicate for the pixels of ONE patch (first row y0, first column x0, at most 32 x 32) without a division per row
// and lane: the residues of y0 and x0 are taken once per patch (wave-uniform; multiply-high by the host's 2^32 / period, exact
// for coordinates below 65536), a pixel's residue is that plus its offset, wrapped at most once (periods of 32 and more;
// shorter periods -- toy windows in tests -- take the modulo route).
struct PatchLive { int ry0, rx0; bool fast; };
__device__ __forceinline__ PatchLive patch_live(const ConvParams& p, int y0, int x0) {
    PatchLive L{0, 0, false};
    if (p.mos_py && p.mos_py >= 32 && p.mos_px >= 32 && p.mos_my) {
        L.fast = true;
        L.ry0 = y0 - (int)__umulhi((uint32_t)y0, (uint32_t)p.mos_my) * p.mos_py;
        L.rx0 = x0 - (int)__umulhi((uint32_t)x0, (uint32_t)p.mos_mx) * p.mos_px;
    }
    return L;
}
__device__ __forceinline__ bool px_live(const ConvParams& p, const PatchLive& L, int y0, int x0, int y, int x) {
    bool ok = (y < p.H) && (x < p.W);
    if (p.mos_py) {
        if (L.fast) {
            int a = L.ry0 + (y - y0), b = L.rx0 + (x - x0);
            a = a >= p.mos_py ? a - p.mos_py : a;
            b = b >= p.mos_px ? b - p.mos_px : b;
            ok = ok && a < p.mos_ry && b < p.mos_rx;
        } else {
            ok = ok && (y % p.mos_py < p.mos_ry) && (x % p.mos_px < p.mos_rx);
        }
    }
    return ok;
}

// Per-device launch state of ONE persistent-workgroup kernel: the dynamic-LDS opt-in and the CU count.  Each launcher instantiation
// keeps one static instance.  The opt-in is per device: a process may hold handles on several GPUs, driven from different threads
// (each handle has its own mutex, so this table needs one of its own).
struct KernelLaunchState {
    std::mutex mu;
    bool attr_set[64] = {false};
    int ncu_dev[64] = {0};
    // first launch on the current device: opt the kernel in to lds_bytes of dynamic LDS; always: *ncu = the device's CU count
    hipError_t prepare(const void* kernel, int lds_bytes, int* ncu) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
        std::lock_guard<std::mutex> lk(mu);
        if (!attr_set[dev]) {
            hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
            if (e != hipSuccess) return e;
            int n = 256;
            (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
            ncu_dev[dev] = n;
            attr_set[dev] = true;
        }
        *ncu = ncu_dev[dev];
        return hipSuccess;
    }
};
// Grid cap (gridcap.hip; the diagnostic mode of s2sr_debug_grid_cap / S2SR_GRID_CAP; DESIGN.md section 2, "Capped grids"): every
// launch whose kernel loops over gridDim.x takes its grid through capped_grid, so that a small image can send each workgroup
// through its loop several times.  `grid` is what the launch would take, `items` what the loop deals out (patches, tiles, or blocks' worth of elements),
// `quantum` what the grid must stay a multiple of.  Off (the default): one relaxed atomic load, and the grid is what it was.  A
// launch that the cap made smaller is counted per family, with ceil(items / grid): what the tests read to know that the second
// trip ran (s2sr_debug_grid_cap_stats).  Launches whose blockIdx IS the work item must not come here: see the list in DESIGN.md.
enum GridFam : int { GF_CONV, GF_TRUNK_F16, GF_TRUNK_F8, GF_PACK, GF_TILES, GF_RESAMPLE, GF_DISPLAY, GF_NODATA, GF_CONSISTENCY, GF_BANDS,
                     GF_POSTPROCESS, GF_COUNT };
inline constexpr const char* kGridFamName[GF_COUNT] = {"conv",    "trunk_f16", "trunk_f8",    "pack",  "tiles",      "resample",
                                                       "display", "nodata",    "consistency", "bands", "postprocess"};
extern std::atomic<int> g_grid_cap;             // 0 off
void grid_cap_note(int fam, long long items, int grid);
static inline int capped_grid(int grid, long long items, int fam, int quantum = 1) {
    int cap = g_grid_cap.load(std::memory_order_relaxed);
    if (!cap) return grid;
    if (quantum > 1) cap = (cap & ~(quantum - 1)) < quantum ? quantum : cap & ~(quantum - 1);   // quantum: a power of two
    if (cap >= grid) return grid;
    grid_cap_note(fam, items, cap);
    return cap;
}
// grid of persistent workgroups: occ per CU, a multiple of 8 (one round over the XCDs); fewer tiles than that: the tiles, rounded up to 8.
// The kernels' tile schedulers turn blockIdx into a slot of the round as (blockIdx % 8) * (grid / 8) + blockIdx / 8, which is a
// permutation only while the grid is a multiple of 8: so a cap of c gives max(8, c & ~7).
static inline int persistent_grid(int ncu, int occ, int ntiles, int fam) {
    const int grid = (ncu * occ) & ~7;
    return capped_grid(ntiles < grid ? (ntiles + 7) & ~7 : grid, ntiles, fam, 8);
}
// grid of a grid-stride loop over `total` elements, 256 per block, at most `most` blocks
static inline int stride_grid(size_t total, int most, int fam) {
    const size_t blocks = (total + 255) / 256;
    return capped_grid((int)(blocks > (size_t)most ? (size_t)most : blocks), (long long)blocks, fam);
}

// conv3x3.hip: the conv of `form` on the row of kTailForms that pick_tail_form (conv_forms.h) answers for the launch
hipError_t launch_conv(const ConvParams& p, ConvForm form, hipStream_t st, const FormSwitches& sw);
// the RRDB trunk convs as one-wave-per-SIMD workgroups (conv_trunk.hip): ct 1 + EPI_LRELU (conv1..4), ct 2 + EPI_RDB5 /
// EPI_RDB5_RRDB (conv5), on the row of kTrunkForms that pick_trunk_form (conv_forms.h) answers.  hipErrorNotSupported = not a
// trunk form, or a hook number no row answers to.
// force_form (the per-layer parity hook, s2sr_debug_conv_trunk's `form`): 0 = by launch size, else the row whose `hook` it is.
// form (optional): the instantiation the launch took (s2sr_debug_trunk_taps' form record), written when the launch was issued
hipError_t launch_conv_trunk(const ConvParams& p, int ct, int epi, hipStream_t st, const FormSwitches& sw, int force_form = 0,
                             s2sr_debug_trunk_form* form = nullptr);
// the same convs on e4m3 operands, block-scaled fp8 MFMA (K = 64 = two planes per instruction)
hipError_t launch_conv_trunk_f8(const ConvParams& p, int ct, int epi, hipStream_t st, int force_form = 0, s2sr_debug_trunk_form* form = nullptr);
// per-plane weight stages for conv_trunk_f8: [plane][tap][ct][16-B half][cout row 0..31][16 channel bytes] e4m3 of
// w * 2^k_co, planes padded to an even count with a zero plane; wscale_out[co] = 127 - k_co
size_t conv_wpack_bytes_f8(int cin, int cout);
void pack_conv_weights_f8(const float* w, int cin, int cout, void* dst_host, int32_t* wscale_out /*[64]*/);
// device-side repack of the RDB convs' weights (pack.hip) and gather of all biases into [nconv][64]
hipError_t launch_pack_trunk_f16(const float* d_w, int cin, int cout, void* d_out, hipStream_t st);
hipError_t launch_pack_trunk_f8(const float* d_w, int cin, int cout, void* d_out, int32_t* d_wscale /*[64]*/, hipStream_t st);
hipError_t launch_gather_bias(const float* d_blob, const uint64_t* d_off, const int32_t* d_cout, int nconv, float* d_out, hipStream_t st);
hipError_t launch_absmax_f16(const void* d, size_t n_halves, float* d_out, hipStream_t st);               // fp8 calibration
hipError_t launch_absmax_e4m3(const void* d, size_t n_bytes, int exp2, float* d_out, hipStream_t st);
hipError_t launch_xh_to_fp8(const char* xh, size_t xh_img, int N, int Hp, int Wp, int x_exp, char* out, size_t out_img, hipStream_t st);
size_t conv_wpack_bytes(int cin, int cout);
// host-side repack: OIHW fp32 -> fp16 A-fragment order [stage][tap][ct][lane][8]
// nseg 1: [w_hi]; 2: [w_hi][w_lo] (exact-integer inputs: conv_first); 3: [w_hi][w_hi][w_lo]
// fold (cout <= 8 only): every segment is [w_hi at couts 0.., w_lo at couts 8..] so a conv with idle
// output channels gets x*w_hi and x*w_lo from one pass over x (conv_last in hp mode: 2 segments, x_hi and x_lo)
void pack_conv_weights(const float* w, int cin, int cout, int nseg, void* dst_host, bool fold = false);
size_t conv_wpack_bytes_seg(int cin, int cout, int nseg);
// SRVGGNetCompact's last conv (64 -> 48 = 3 colours x 4 x 4 sub-pixels): which state-dict output channel sits in row
// `row` (0..63) of the packed weights / bias, -1 = an idle (zero) row.  Chosen so that a lane's 16 accumulators of cout tile ct
// are [colour 0..2][dx 0..3] of HR row dy = 2 * half-wave + ct (EPI_CLAST): 12 contiguous u8 / 3 x 16 contiguous fp32 bytes.
int compact_last_row_channel(int row);
// split-operand convs with fp8 correction terms (cin == 64): 4 fp16 stages [w_hi] + 4 e4m3 stages
// [w_hi ch 0-31][w_hi ch 32-63][w_lo*2^11 ch 0-31][w_lo*2^11 ch 32-63]; an fp8 stage fragment is
// [tap][ct][16-B half][cout row 0..31][16 channel bytes].  Same size as nseg = 2.
// fold (cout <= 8, conv_last): 4 fp16 stages [w_hi at couts 0.. | w_lo at couts 8..] + the two e4m3 w_hi planes (6 stages)
void pack_conv_weights_f8hp(const float* w, int cin, int cout, void* dst_host, bool fold = false);
// sub-pixel form of the split-operand up-convs: four 2x2-tap kernels (one per output parity), same stage layout
void pack_conv_weights_phase_f8hp(const float* w, int cin, int cout, int phase, void* dst_host);
size_t conv_wpack_bytes_phase(int cin, int cout);
hipError_t launch_conv_phase(const ConvParams& p, int row_parity, hipStream_t st, bool f8, const FormSwitches& sw);
uint8_t f32_to_e4m3(float f);   // OCP e4m3fn, round to nearest even, saturating at +-448

// display rendering of 16-bit images (display.hip): the samples [s0, s1) of a uint16 [H, W, 3] image (a band of whole rows; at
// most 2^30 for the histogram).  d_img: 16-byte aligned and readable up to the next multiple of 16 bytes behind its last sample;
// d_out is addressed from the image's first sample like d_img.  hist: uint64 [3][65536], added to; nodata -1: none.
hipError_t launch_display_hist(const uint16_t* d_img, size_t s0, size_t s1, int nodata, unsigned long long* d_hist, hipStream_t st);
hipError_t launch_display_apply(const uint16_t* d_img, size_t s0, size_t s1, const uint8_t* d_lut, uint8_t* d_out, hipStream_t st);

// nodata-aware enhance (nodata.hip).  fill: the invalid pixels of d_img [H, W, 3] take their nearest valid neighbour's
// samples within `radius` (1..64), in place; d_valid: uint8 [H, W], nonzero = valid.  mask: out_nodata into the scale x scale output
// pixels of every invalid input pixel, rows [yb, ye) of d_out [scale H, scale W, 3] (the image's base); scale 2 or 4.
hipError_t launch_nodata_fill(uint8_t* d_img, const uint8_t* d_valid, int H, int W, int radius, hipStream_t st);
hipError_t launch_nodata_fill(uint16_t* d_img, const uint8_t* d_valid, int H, int W, int radius, hipStream_t st);
hipError_t launch_nodata_mask(const uint8_t* d_valid, int H, int W, int scale, int yb, int ye, int out_nodata, uint8_t* d_out, hipStream_t st);
hipError_t launch_nodata_mask(const uint8_t* d_valid, int H, int W, int scale, int yb, int ye, int out_nodata, uint16_t* d_out, hipStream_t st);

// radiometric consistency (consistency.hip), in place on block rows [by0, by1) of d_img [S H, S W, 3]; d_lr: the input
// [H, W, 3]; S 2 or 4.  form 0: the residuals n v - sum of those block rows into d_e (int32 [H, W, 3]; the image is only read);
// form 1: the exact step; form 2: the smooth step, then the exact one -- it reads d_e of block rows by0 - 1 .. by1 (clamped to the
// image), which form 0 must have filled from the untouched image.  d_cnt: uint64[3], the inexact blocks per channel, added to.
// swap: image channel c belongs to input channel 2 - c.
hipError_t launch_consistency(int form, uint8_t* d_img, const uint8_t* d_lr, int32_t* d_e, unsigned long long* d_cnt, int H, int W, int S,
                              int by0, int by1, int swap, hipStream_t st);
hipError_t launch_consistency(int form, uint16_t* d_img, const uint16_t* d_lr, int32_t* d_e, unsigned long long* d_cnt, int H, int W, int S,
                              int by0, int by1, int lo, int hi, hipStream_t st);

// carrying an extra band to the SR grid (bands.hip).  d_q: the guide, uint16 [S H, S W, 3]; d_band: uint16 [H, W];
// d_valid: uint8 [H, W], nonzero = valid, or null; S 2 or 4; w: the three guide weights (0..255, not all zero).  coeffs: A (int32
// [H, W], Q16) and C (int64 [H, W]) of pixel rows [y0, y1) -- it reads the guide, the band and the mask of rows y0 - r .. y1 - 1 + r
// (cut at the image).  apply: block rows [by0, by1) of d_out (uint16 [S H, S W]) -- it reads A and C of rows by0 - 1 .. by1 (clamped
// to the image); d_cnt: one uint64, the inexact valid blocks, added to; fill goes over the invalid blocks.
hipError_t launch_band_coeffs(const uint16_t* d_q, const uint16_t* d_band, const uint8_t* d_valid, int32_t* d_A, long long* d_C, int H, int W,
                              int S, int y0, int y1, int lo, int hi, const int w[3], int r, long long eps, hipStream_t st);
hipError_t launch_band_apply(const uint16_t* d_q, const uint16_t* d_band, const uint8_t* d_valid, const int32_t* d_A, const long long* d_C,
                             uint16_t* d_out, unsigned long long* d_cnt, int H, int W, int S, int by0, int by1, int lo, int hi, const int w[3],
                             int fill, hipStream_t st);

// normalised-difference indices (index.hip): rows [y0, y1) of the index of channel ca of d_a ([H, W, ac], ac 1 or 3) and
// channel cb of d_b.  d_valid [ceil(H / vs)][ceil(W / vs)] or null; d_zones likewise at zs, with d_zonal (uint64 [Z + 1][3], two's
// complement sums, added to); d_lut uint8 [65536][4] (required with d_rgba); d_hist uint64 [2 K + 1] and d_undefined are added to.
// Every output may be null.  Bases 16-byte aligned and readable up to the next multiple of 16 bytes; H W < 2^31.
hipError_t launch_index_nd(const uint16_t* d_a, int ac, int ca, const uint16_t* d_b, int bc, int cb, int H, int W, int y0, int y1, int offset,
                           int L, int K, const uint8_t* d_valid, int vs, const uint16_t* d_zones, int zs, int Z, const uint8_t* d_lut,
                           int16_t* d_out, unsigned long long* d_hist, unsigned long long* d_zonal, uint8_t* d_rgba,
                           unsigned long long* d_undefined, hipStream_t st);
// rows [y0, y1) of an int16 index raster through the LUT: -32768 gives 0, 0, 0, 0
hipError_t launch_index_render(const int16_t* d_idx, int H, int W, int y0, int y1, const uint8_t* d_lut, uint8_t* d_rgba, hipStream_t st);

// Polygon rasterisation to zone labels (zones.hip): rows [y0, y1) of the uint16 label raster d_out [H, W] (16-byte
// aligned) from tables that zone_check_tables accepted and the bins zone_build_bins made of them (zone_bins.h), all on the device;
// d_area (uint64 [Z + 1], or null) is added to.  Every pixel of the rows is stored exactly once.
hipError_t launch_zones_rasterize(const int32_t* d_xy, const int32_t* d_ring_start, const int32_t* d_feat_start, const uint16_t* d_label,
                                  const uint32_t* d_tile_start, const int32_t* d_tile_feat, int H, int W, int y0, int y1, uint16_t* d_out,
                                  unsigned long long* d_area, hipStream_t st);

// Fields from the image (fields.hip), one launcher per stage, all on whole H x W planes (H W < 2^31):
//   mask     d_mask = idx is data and lo <= idx <= hi; with and_into: d_mask &= idx is data
//   morph    one erode (or dilate) pass of radius r in 1..8 along the rows (or, with column, the columns), d_src -> d_dst
//   local    the 64 x 64 tiles' components: d_parent int32 = the global linear index of the local root, -1 for background; d_size
//            uint32 = the local component's pixels at its local root, 0 elsewhere.  Every pixel of both planes is written.
//   border   the unions across the tile lines; flatten: parent = root, the local counts added up at the roots
//   count, scan, apply (the numbering)   d_sums uint32 [fields_chunks(H, W)] is scratch; *d_found the components of at least min_pixels; at the roots d_size
//            becomes the rank (0: too small); rows 1 .. min(found, Z) of d_fields (uint64 [Z + 1][6], zeroed by the caller) get
//            pixels, key and an empty box
//   labels   d_labels uint16 = the rank of the pixel's root, 0 above Z; narrows the boxes and adds the unlabelled pixels to row 0
hipError_t launch_fields_mask(const int16_t* d_idx, int H, int W, int lo, int hi, int and_into, uint8_t* d_mask, hipStream_t st);
hipError_t launch_fields_morph(const uint8_t* d_src, uint8_t* d_dst, int H, int W, int r, int erode, int column, hipStream_t st);
hipError_t launch_fields_local(const uint8_t* d_mask, int* d_parent, uint32_t* d_size, int H, int W, int conn, hipStream_t st);
hipError_t launch_fields_border(int* d_parent, int H, int W, int conn, hipStream_t st);
hipError_t launch_fields_flatten(int* d_parent, uint32_t* d_size, int H, int W, hipStream_t st);
size_t fields_chunks(int H, int W);
hipError_t launch_fields_count(const int* d_parent, const uint32_t* d_size, int H, int W, uint32_t min_pixels, uint32_t* d_sums, hipStream_t st);
hipError_t launch_fields_scan(uint32_t* d_sums, int H, int W, unsigned long long* d_found, hipStream_t st);
hipError_t launch_fields_apply(const int* d_parent, uint32_t* d_size, int H, int W, uint32_t min_pixels, uint32_t Z, const uint32_t* d_sums,
                               unsigned long long* d_fields, hipStream_t st);
hipError_t launch_fields_labels(const int* d_parent, const uint32_t* d_size, int H, int W, uint32_t Z, uint16_t* d_labels, unsigned long long* d_fields,
                                hipStream_t st);

// Touching fields split (fields_split.hip), one launcher per step, all on whole H x W planes (H W < 2^31):
//   edge      d_interior = d_m minus the edge pixels (edge in 1..32767, edge_r in 0..4); d_interior is another plane than d_m
//   distance  d_g uint8 = the vertical distance to the nearest pixel outside the interior, capped at 255 (scratch); d_d2 uint16 =
//             the squared Euclidean distance to it, capped at 255^2, 0 outside the interior.  Every pixel of both is written.
//   cores     d_parent: the roots of the interior's components (launch_fields_local, _border, _flatten); d_dmax uint32 per pixel is
//             scratch (cleared here; a component's largest D2 at its root); d_cores uint8 = 1 on core pixels
//   seed      d_word uint64 per pixel = the marker's key (d_parent: the roots of the cores' components), all ones elsewhere
//   grow      one round: a pixel of d_a that is not in d_b (null: none is) takes the least of its word and its neighbours' plus one
//             step; *d_changed (cleared by the caller) counts the tiles that stored something; such a tile marks itself and its eight
//             neighbours in d_dirty_out (uint8 [fsplit_tiles(H, W)], cleared by the caller), and a tile that d_dirty_in (the round
//             before's; null: the first round) does not mark is passed over.  restart: every reached pixel to step 0
//   remap     d_parent = the smallest linear index of the pixel's owner's pixels (-1: no owner), d_size = the pixels at that index:
//             what launch_fields_count, _scan, _apply and _labels take
hipError_t launch_fsplit_edge(const int16_t* d_idx, const uint8_t* d_m, uint8_t* d_interior, int H, int W, int edge, int edge_r, hipStream_t st);
hipError_t launch_fsplit_distance(const uint8_t* d_interior, uint8_t* d_g, uint16_t* d_d2, int H, int W, hipStream_t st);
hipError_t launch_fsplit_cores(const int* d_parent, const uint16_t* d_d2, uint32_t* d_dmax, uint8_t* d_cores, int H, int W, int core_q, int core_px,
                               hipStream_t st);
hipError_t launch_fsplit_seed(const int* d_parent, unsigned long long* d_word, int H, int W, hipStream_t st);
hipError_t launch_fsplit_restart(unsigned long long* d_word, int H, int W, hipStream_t st);
size_t fsplit_tiles(int H, int W);
hipError_t launch_fsplit_grow(const uint8_t* d_a, const uint8_t* d_b, unsigned long long* d_word, int H, int W, int conn, uint32_t* d_changed,
                              const uint8_t* d_dirty_in, uint8_t* d_dirty_out, hipStream_t st);
hipError_t launch_fsplit_remap(const unsigned long long* d_word, int* d_parent, uint32_t* d_size, int H, int W, hipStream_t st);

// Management zones (mzones.hip), one launcher per step.  d_feat: int16 [D][H][W] (D in 1..4), d_labels: uint16 [H][W],
// H W < 2^31, Z in 1..65535, k in 2..8; the pixel passes take the rows [y0, y1) of the image.  The tables, Z + 1 rows each:
//   d_cnt uint32, d_lo / d_hi int32 [D]       the members and their minimum / maximum per feature (clear, then stats band by band)
//   d_status uint8                            0 absent, 1 skipped (fewer than `least` = k min_per_zone members), 2 zoned
//   d_centres int32 [k][D]                    start writes them, update moves them
//   d_acc uint64 [k][1 + D]                   n, s_d of one iteration: zero before the first accumulate, left at zero by update;
//                                             with d_zone (the table pass) [k][1 + 2 D]: n, then s_d, q_d per feature, zeroed by the caller
//   d_zone_of uint8 [k], d_ranked int32 [k][D]   rank: the zone id of cluster j, and the centres in zone order
//   *d_changed                                update ORs 1 into it when a centre moved
// accumulate without d_zone assigns each member to its nearest centre; with d_zone the cluster is the raster's id - 1.
// assign writes every pixel of its rows of d_zone; mode is one Jacobi pass of the 3 x 3 filter, d_src the whole previous raster.
hipError_t launch_mzones_clear(uint32_t* d_cnt, int* d_lo, int* d_hi, int Z, int D, hipStream_t st);
hipError_t launch_mzones_stats(const int16_t* d_feat, int D, int H, int W, int y0, int y1, const uint16_t* d_labels, int Z, uint32_t* d_cnt, int* d_lo,
                               int* d_hi, hipStream_t st);
hipError_t launch_mzones_start(const uint32_t* d_cnt, const int* d_lo, const int* d_hi, int Z, int k, int D, long long least, uint8_t* d_status,
                               int* d_centres, hipStream_t st);
hipError_t launch_mzones_accumulate(const int16_t* d_feat, int D, int H, int W, int y0, int y1, const uint16_t* d_labels, int Z, int k,
                                    const int* d_centres, const uint8_t* d_status, const uint8_t* d_zone, unsigned long long* d_acc, hipStream_t st);
hipError_t launch_mzones_update(unsigned long long* d_acc, int Z, int k, int D, const uint8_t* d_status, int* d_centres, uint32_t* d_changed, hipStream_t st);
hipError_t launch_mzones_rank(const int* d_centres, int Z, int k, int D, const uint8_t* d_status, uint8_t* d_zone_of, int* d_ranked, hipStream_t st);
hipError_t launch_mzones_assign(const int16_t* d_feat, int D, int H, int W, int y0, int y1, const uint16_t* d_labels, int Z, int k, const int* d_centres,
                                const uint8_t* d_status, const uint8_t* d_zone_of, uint8_t* d_zone, hipStream_t st);
hipError_t launch_mzones_mode(const uint8_t* d_src, const uint16_t* d_labels, int H, int W, int y0, int y1, int k, uint8_t* d_dst, hipStream_t st);

// XYZ tile pyramid (tiles.hip)
hipError_t launch_warp_bilinear(const uint8_t* d_rgb, int H, int W, const float* d_grid, int gh, int gw, int step, int OH, int OW,
                                uint8_t* d_out, hipStream_t st);
// ... with the validity mask d_valid [ceil(H / vs)][ceil(W / vs)], nonzero = valid
hipError_t launch_warp_bilinear_masked(const uint8_t* d_rgb, int H, int W, const uint8_t* d_valid, int vs, const float* d_grid, int gh,
                                       int gw, int step, int OH, int OW, uint8_t* d_out, hipStream_t st);
hipError_t launch_tiles_base(const uint8_t* d_rgba, int W, const int32_t* d_col_lo, const int32_t* d_col_hi, const int32_t* d_row_lo,
                             const int32_t* d_row_hi, int nx, int ny, uint8_t* d_out, hipStream_t st);
hipError_t launch_tiles_overview(const uint8_t* d_child, int cnx, int cny, int ox, int oy, int pnx, int pny, uint8_t* d_out,
                                 hipStream_t st);

// resampled tile levels (resample.hip): tap tables in, no notion of a filter.  level: the source is a tile-major level sb tiles
// wide (else a raster sb pixels wide); the horizontal pass fills the intermediate's rows [r0, r0 + nrows) of the source
hipError_t launch_resample_h(const uint8_t* d_src, bool level, int sb, const int32_t* d_first, const int32_t* d_count,
                             const int32_t* d_coef, int nx, int r0, int nrows, uint8_t* d_inter, hipStream_t st);
hipError_t launch_resample_v(const uint8_t* d_inter, int r0, const int32_t* d_first, const int32_t* d_count, const int32_t* d_coef,
                             int nx, int ny, uint8_t* d_out, hipStream_t st);

// PNG encoding of a tile level on the device (pngdev.hip): stats kernel -> host plan (Huffman codes, sizes) -> emit kernel.
struct PngTilePlan {
    std::vector<uint8_t> mode;            // 0 nothing to write, 1 device stream, 2 host encoder (stored blocks are smaller)
    std::vector<uint32_t> adler, deflate_bytes, eob;
    std::vector<uint64_t> eob_at, out_word;
    // what the emit kernel reads: [n][512] token table, [n][160] block header words, [n] TileMeta (pngdev.hip) -- in this order in
    // ONE block of upload_bytes: the caller's page-locked arena when it gave one (arena / arena_bytes), else `own`
    uint32_t* tb = nullptr;
    uint32_t* hdr = nullptr;
    uint8_t* meta = nullptr;
    size_t upload_bytes = 0;
    void* arena = nullptr;
    size_t arena_bytes = 0;
    std::vector<uint8_t> own;
    bool failed = false;                  // a planning thread threw (out of memory): the plan is incomplete
};
hipError_t launch_png_tile_stats(const uint8_t* d_tiles, int ntiles, uint32_t* d_hist, uint32_t* d_adler, uint32_t* d_flags, bool row_threads,
                                 hipStream_t st);
hipError_t launch_png_tile_emit(const uint8_t* d_tiles, int ntiles, const void* d_meta, const uint32_t* d_tb, const uint32_t* d_hdr,
                                uint32_t* d_out, bool row_threads, hipStream_t st);
size_t png_plan_bytes(int n);      // bytes of the upload block of n tiles
size_t png_plan_tiles(int n, const uint32_t* hist, const uint32_t* adler_rows, const uint32_t* flags, const char* const* paths,
                      bool skip_transparent, bool force_host, PngTilePlan* plan);
bool png_write_tile_file(const char* path, const uint32_t* words, uint32_t deflate_bytes, uint32_t eob, uint64_t eob_at, uint32_t adler,
                         std::vector<uint8_t>& buf);
bool png_parallel_for(int n, const std::function<void(int)>& body);   // false: a body threw (the other indices still ran)

// data-movement kernels (pack.hip)
// What a forward reads: B tiles of th x tw on the device, [B,th,tw,3] u8 or u16 (value range lo < hi) or [B,3,th,tw] fp32 in [0, 1].
// src_h x src_w (0: th x tw): what the single u8 image holds when it is one short of th / tw (scale 2, odd image).
enum TileKind { TILE_U8, TILE_U16, TILE_F32 };
struct TileIn {
    TileKind kind = TILE_U8;
    const void* p = nullptr;
    int lo = 0, hi = 0;
    int src_h = 0, src_w = 0;
    static TileIn u8(const void* p, int src_h = 0, int src_w = 0) { return TileIn{TILE_U8, p, 0, 0, src_h, src_w}; }
    static TileIn u16(const void* p, int lo, int hi) { return TileIn{TILE_U16, p, lo, hi, 0, 0}; }
    static TileIn f32(const void* p) { return TileIn{TILE_F32, p, 0, 0, 0, 0}; }
    // the same input from tile t0 on (src_h x src_w filled in: every kind stores 3 * src_h * src_w samples per tile)
    TileIn from(size_t t0) const {
        TileIn r = *this;
        r.p = (const char*)p + t0 * 3 * src_h * src_w * (kind == TILE_U8 ? 1 : kind == TILE_U16 ? 2 : 4);
        return r;
    }
    bool operator==(const TileIn& o) const { return kind == o.kind && p == o.p && lo == o.lo && hi == o.hi && src_h == o.src_h && src_w == o.src_w; }
};
// B tiles of `in` -> the one-block input plane blk of the h x w trunk grid; the layouts are stated at the family in pack.hip.
// unshuffle 2: pixel_unshuffle(x, 2) on the way, tiles of 2h x 2w.  f32 values leave as x * f32_scale.  kx > 0: a window mosaic of
// kx x ky cells per image.  hipErrorInvalidValue for a combination that is not built.
hipError_t launch_pack_tiles(const TileIn& in, int unshuffle, float f32_scale, int B, int h, int w, int kx, int ky, char* blk, int Hp, int Wp,
                             hipStream_t st);
// [N,C,H,W] fp32 -> NB blocks per image, any channel count (launch_pack_tiles' plain f32 form; the per-layer test hooks)
hipError_t launch_pack_f32_nchw(const float* d_x, int N, int C, int H, int W, float scale, char* blk, int NB,
                                int Hp, int Wp, hipStream_t st);
hipError_t launch_trunk_to_fp8(const char* hi, size_t hi_img, const char* lo, size_t lo_img, int lo_e4m3_exp, int N, int Hp, int Wp, char* out,
                               hipStream_t st);
hipError_t launch_swap_rb_u8(const uint8_t* d_in, size_t npx, uint8_t* d_out, hipStream_t st);
// T windows (d_rects: y1, y2, x1, x2 each) of wh x ww out of an H x W image.  reflect: windows of the reflect-padded image (scale 2,
// odd H or W): row H reads row H - 2, column W column W - 2.  2-byte samples: scale 4 only, no reflect form.
hipError_t launch_gather_windows(const uint8_t* d_img, int H, int W, const int32_t* d_rects, int T, int wh, int ww, bool reflect,
                                 uint8_t* d_tiles, hipStream_t st);
hipError_t launch_gather_windows(const uint16_t* d_img, int H, int W, const int32_t* d_rects, int T, int wh, int ww, uint16_t* d_tiles,
                                 hipStream_t st);
// crop + paste through the paste maps into an HWC image: u8 tiles [T,oth,otw,3], fp32 tiles [T,3,oth,otw]
hipError_t launch_stitch(const uint8_t* d_tiles, int tilesX, int oth, int otw, const int32_t* d_rowmap, const int32_t* d_colmap, int OH,
                         int OW, uint8_t* d_out, hipStream_t st);
hipError_t launch_stitch(const float* d_tiles, int tilesX, int oth, int otw, const int32_t* d_rowmap, const int32_t* d_colmap, int OH,
                         int OW, float* d_out, hipStream_t st);
// crop + paste + quantise: planar fp32 tiles [.., 3, oth, otw] -> OH rows of an HWC u16 image, q = lo + rint(clamp(y, 0, 1) * (hi - lo)).
// d_rowmap points at the first row of the band (d_out likewise); window (ty, tx) is tile ty * tilesX + tx - tile0 of d_tiles.
// d_rowmap == nullptr: a plain batch (output row oy = row oy % oth of tile oy / oth); d_colmap == nullptr: identity columns.
// OW must be a multiple of 4 and d_out 8-byte aligned (hipErrorInvalidValue otherwise).
hipError_t launch_stitch_quant_u16(const float* d_tiles, int tilesX, int tile0, int oth, int otw, const int32_t* d_rowmap,
                                   const int32_t* d_colmap, int OH, int OW, int lo, int hi, uint16_t* d_out, hipStream_t st);
// seam-blended stitch (blend_plan.h): planar fp32 tiles -> OH rows of an HWC image, cross-faded inside the ramps of the blend tables
// d_rows (already at the band's first row, d_out likewise) and d_cols; window (ty, tx) is tile ty * tilesX + tx - tile0 of d_tiles
// (tile0 may be negative: a buffer with rows in front of the chunk's).  u8: trunc(clip(v * 255, 0, 255)), optionally with R and B
// exchanged; u16: lo + rint(clamp(v, 0, 1) * (hi - lo)); fp32: v.
hipError_t launch_stitch_blend(const float* d_tiles, int tilesX, int tile0, int oth, int otw, const int32_t* d_rows, const int32_t* d_cols,
                               int OH, int OW, bool swap_rb, uint8_t* d_out, hipStream_t st);
hipError_t launch_stitch_blend(const float* d_tiles, int tilesX, int tile0, int oth, int otw, const int32_t* d_rows, const int32_t* d_cols,
                               int OH, int OW, int lo, int hi, uint16_t* d_out, hipStream_t st);
hipError_t launch_stitch_blend(const float* d_tiles, int tilesX, int tile0, int oth, int otw, const int32_t* d_rows, const int32_t* d_cols,
                               int OH, int OW, float* d_out, hipStream_t st);

// post-process kernels (postprocess.hip)
hipError_t launch_postprocess(const uint8_t* d_rgb, int B, int H, int W, const s2sr_pp_params& prm, uint8_t* d_out,
                              void* d_work, size_t work_bytes, hipStream_t st);
size_t postprocess_work_bytes(int B, int H, int W, const s2sr_pp_params& prm);
// nullptr, or why `prm` is refused (clahe_grid outside 1..64; unsharp stage with a sigma whose kernel is wider than the device's 17 taps)
const char* pp_params_error(const s2sr_pp_params& prm);
// ... over ONE image in row bands (an AOI's mosaic arrives band by band; CLAHE's grid is image-global): histograms as the bands
// arrive, LUTs once, then apply (R rows ahead) + sharpen band by band.  d_work = postprocess_work_bytes(1, H, W, prm) bytes; bgr:
// the image's bytes are B,G,R; swap_out: R and B exchanged in the rows written.  Same bytes as launch_postprocess.
int pp_band_radius(const s2sr_pp_params& prm);
hipError_t launch_pp_band_begin(int H, int W, const s2sr_pp_params& prm, void* d_work, hipStream_t st);
hipError_t launch_pp_band_hist(const uint8_t* d_img, int H, int W, const s2sr_pp_params& prm, int bgr, int y0, int y1, void* d_work,
                               hipStream_t st);
hipError_t launch_pp_band_lut(int H, int W, const s2sr_pp_params& prm, void* d_work, hipStream_t st);
hipError_t launch_pp_band_apply(const uint8_t* d_img, int H, int W, const s2sr_pp_params& prm, int bgr, int y0, int y1, void* d_work,
                                hipStream_t st);
hipError_t launch_pp_band_sharpen(int H, int W, const s2sr_pp_params& prm, int bgr, int swap_out, int y0, int y1, void* d_work,
                                  uint8_t* d_out, hipStream_t st);

// measured MFMA ceilings (ceiling.hip): bare / LDS-fed / LDS-DMA-fed fp16 32x32x16 loops at conv_trunk_f16's operand traffic
hipError_t launch_mfma_ceiling(int mode, char* d_src, size_t src_bytes, bool fill, float* d_sink, int grid, int stages, char* d_store,
                               size_t store_bytes, hipStream_t st);
double mfma_ceiling_flop_per_launch(int mode, int grid, int stages);
double mfma_ceiling_dma_bytes_per_launch(int mode, int grid, int stages);

// diagnostic prototype (persist.hip): an RDB-shaped loop whose workgroups stay across layers, planes handed over through flags
hipError_t launch_rdb_persistent(int variant, const char* d_wts, size_t wts_bytes, char* d_ws, uint32_t* d_flags, float* d_sink, int grid, int P,
                                 int rdbs, uint32_t* d_timeouts, hipStream_t st);
size_t rdb_persistent_ws_bytes(int variant, int grid, int P);
double rdb_persistent_flop_per_launch(int grid, int P, int rdbs);

}  // namespace s2sr
