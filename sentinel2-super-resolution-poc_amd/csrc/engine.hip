// libs2sr engine: handle, weights, workspace planes and the layer schedule of
// RRDBNet.forward / RealESRGAN.enhance (reference server/app/cnn_super_resolution.py:140-158,
// 217-280) on top of the conv kernel in conv_mfma.hip.  This file is the C ABI of
// include/s2sr.h.  There is no CPU fallback anywhere in this library.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "png_internal.h"
#include "s2sr_internal.h"

using namespace s2sr;

std::recursive_mutex& s2sr::device_gate() {      // see s2sr_internal.h
    static std::recursive_mutex m;
    return m;
}

namespace {

thread_local std::string g_create_error;

struct ConvW {
    int cin = 0, cout = 0, nstage = 0, ct = 0;
    int seg_len = 0, seg_lo_mask = 0;   // split-operand convs (precision S2SR_PREC_F16_HP), see ConvParams
    bool fold = false;                  // conv_last in hp mode: w_lo folded into idle couts (pack_conv_weights)
    bool f8 = false;                    // hp mode, cin 64: fp16 main term + e4m3 correction planes (pack_conv_weights_f8hp)
    void* d_wphase[2] = {nullptr, nullptr};   // hp up-convs: the 2x2 sub-pixel kernels per output row parity (pack_conv_weights_phase_f8hp)
    void* d_wpack = nullptr;
    float* d_bias = nullptr;
    // fp8 trunk mode (S2SR_PREC_FP8), the 345 RDB convs: e4m3 weight planes (pack_conv_weights_f8; nstage = planes padded
    // to even, seg_len = real planes) + per-output-channel E8M0 scale bytes
    bool f8trunk = false;
    int32_t* d_wscale = nullptr;
    bool pooled = false;                // d_wpack / d_wscale point into the handle's pools
    float* d_slope = nullptr;           // SRVGGNetCompact: the 64 PReLU slopes behind this conv (in pool_b, next to the bias)
};

// kernel families for the HIP-event statistics
enum Fam { F_PACK, F_FIRST, F_RDB14, F_RDB5, F_BODY, F_UP, F_HR, F_LAST, F_POST, F_MISC, F_CFIRST, F_CBODY, F_CLAST, F_COUNT };
const char* kFamName[F_COUNT] = {"pack_u8",   "conv_first", "rdb_conv1-4", "rdb_conv5",   "conv_body",
                                 "conv_up",   "conv_hr",    "conv_last",   "postprocess", "misc",
                                 "compact_first", "compact_body", "compact_last"};

struct Workspace {
    int G = 0, H = 0, W = 0;   // capacity (images) and logical LR dims
    char* base = nullptr;
    size_t bytes = 0;
    // LR tensors (blocked-16 fp16 / blocked-8 fp32, see s2sr_internal.h)
    char *P0 = nullptr;                  // input, 1 block
    char *D[3] = {nullptr, nullptr, nullptr};   // dense-block tensors, 12 blocks: [x(4) | x1 | x2 | x3 | x4]; three of them rotate
                                         // through an RRDB (rdb k reads D[k], writes the next x into D[(k+1)%3]), so the
                                         // RRDB's input D[0] is still there when rdb3's conv5 needs it as the skip
    char *U0 = nullptr;                  // 4 blocks
    char *T = nullptr;                   // trunk lo as fp16 (4 blocks): conv_first writes it, conv_body's packer reads it (8-wave path: every conv5 too)
    char *Tr[3] = {nullptr, nullptr, nullptr};  // one-wave-per-SIMD path: trunk lo of D[0..2] as e4m3(lo * 2^lo_exp), 2 planes of 32 channels
    float *R = nullptr, *F = nullptr;    // fp32 RRDB skip / global skip (8 blocks of 8)
    // 2x and 4x tensors, 4 blocks each
    char *U1 = nullptr, *U2 = nullptr, *U3 = nullptr;
    // split-operand mode only: e4m3 correction planes of U0..U3 and of the trunk, 4 planes of 32 B per
    // pixel each ([lo*2^11 p0, p1, hi p0, p1]) -- the size of a 4-block fp16 tensor
    char *U0lo = nullptr, *U1lo = nullptr, *U2lo = nullptr, *U3lo = nullptr, *T8 = nullptr;
    // fp8 trunk mode only: the dense-block tensors as e4m3 planes of 32 channels [x(2) | x1 | x2 | x3 | x4], the trunk x in
    // fp16 (three rotating buffers: an RRDB's input stays readable until its last conv5 has used it as the skip), and
    // an all-zero "trunk lo" for conv_body's split-operand path
    char *D8[2] = {nullptr, nullptr};
    char *Xh[3] = {nullptr, nullptr, nullptr};
    char *Tz = nullptr;
    bool hp = false, fp8 = false;
    int mos_py = 0, mos_px = 0;          // separator periods of the window mosaic these planes were zeroed for (0: plain images)
    int Hp = 0, Wp = 0, Hp2 = 0, Wp2 = 0, Hp4 = 0, Wp4 = 0;
    size_t blk1 = 0, blk2 = 0, blk4 = 0;   // bytes of one block plane at 1x / 2x / 4x
};

struct EvRec {
    int fam;
    hipEvent_t e0, e1;
    double flops, bytes;
    int n = 1;           // launches between the two events (a span of consecutive launches of one family)
};

// One captured group (pack + the whole layer schedule) for fixed shapes and buffers.  A net is
// 351 dependent launches; small groups are launch-bound (~15 us per launch against a few us of
// work), so the second time the same (shape, buffers) group shows up it is captured into a
// hipGraph and replayed from then on.
// Window mosaic geometry of one forward (see ConvParams::mos_*): kx x ky windows of wh x ww per image, `count` windows in all.
struct Mosaic {
    int kx = 1, ky = 1, wh = 0, ww = 0, count = 0;
    bool on() const { return wh > 0; }
};

struct GraphEntry {
    int n = 0, th = 0, tw = 0;
    int sh = 0, sw = 0;              // input rows / columns as stored (forward_dev src_h / src_w)
    int mos_kx = 0, mos_ky = 0, mos_count = 0;
    const void *in_u8 = nullptr, *in_f32 = nullptr;
    void *out_u8 = nullptr, *out_f32 = nullptr;
    hipStream_t st = nullptr;
    hipGraphExec_t exec = nullptr;   // null until captured
    bool refused = false;            // capture failed once: stay on direct launches
    uint64_t last_use = 0;
};

// s2sr_debug_trunk_taps while its batch runs: the RDB range whose fields run_net copies out (trunk_tap) and where the form
// records of the range's conv launches go
// s2sr_debug_compact_taps while its batch runs: run_net_compact copies the chosen layers' activations out
struct CompactTap {
    s2sr_debug_compact_fields* t = nullptr;
};

struct TrunkTap {
    int first = 0, count = 0;
    s2sr_debug_trunk_fields* t = nullptr;
    s2sr_debug_trunk_form spare[5];     // the records of RDBs outside the range
    s2sr_debug_trunk_form* forms(int g) { return t->form && g >= first && g < first + count ? t->form + 5 * (g - first) : spare; }
};

}  // namespace

struct s2sr_handle {
    s2sr_config cfg{};
    // RealESRGAN_x2plus (cfg.scale 2) runs pixel_unshuffle(x, 2) and then the x4 net on the half grid.  Every entry takes input
    // sizes: the trunk (workspace, mosaic, launch groups, graphs) is input / unshuffle(), the output input * cfg.scale.
    int unshuffle() const { return cfg.scale == 2 ? 2 : 1; }
    bool compact() const { return cfg.arch == S2SR_ARCH_COMPACT; }   // SRVGGNetCompact: cfg.num_block carries num_conv
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string err;
    std::vector<ConvW> convs;
    // the packed weights of the 345 RDB convs, their fp8 scales and every conv's bias live in three pooled allocations
    // (ConvW pointers point into them); only the six head/tail convs own separate buffers (pooled == false)
    char* pool_w = nullptr;
    int32_t* pool_s = nullptr;
    float* pool_b = nullptr;
    bool has_weights = false;
    char* d_trash = nullptr;      // parking area for out-of-image epilogue stores
    Workspace ws;
    // scratch device buffers (grown on demand)
    void* d_scratch[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t scratch_bytes[6] = {0, 0, 0, 0, 0, 0};
    int capture_failures = 0;            // captures voided by a device-wide call of another runtime user; 3 -> graphs off
    int tiles_slot = -1;                 // scratch slot that still holds the tile level the last pyramid call produced (-1: none)
    int tiles_nx = 0, tiles_ny = 0;
    int warp_slot = -1, warp_h = 0, warp_w = 0;   // ... and the RGBA raster the last warp produced (s2sr_tiles_base_u8 with rgba == NULL)
    // profiling
    int prof = 0;                 // 0 off, N>=1: bracket every N-th launch of each family with events
    bool span_on = false;         // a sampled span of consecutive launches of ONE family is open (span_begin / span_end): its launches
    EvRec span;                   // add their work to it instead of recording events of their own.  Two marker packets between two
    int64_t span_count = 0;       // kernels cost ~2 us of a 70-us launch (r03: 71.6 us by events against 69.0 by rocprofv3); one pair around
                                  // the four conv1-4 launches of an RDB spreads that over four
    int64_t fam_count[16] = {0};
    std::vector<EvRec> evs;
    std::vector<hipEvent_t> ev_pool;
    s2sr_kstat stats[F_COUNT];
    hipStream_t copy_stream = nullptr;          // device-to-host copies behind the compute stream
    std::vector<hipEvent_t> group_done;
    void* stage_buf[2] = {nullptr, nullptr};    // pinned staging slices of the device-to-host path (d2h_staged)
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    bool d2h_staged_on = true;                  // S2SR_D2H_STAGED=0: hipMemcpyAsync straight into the caller's (pageable) buffer
    // hipGraph replay of repeated groups
    float* d_calib = nullptr;     // fp8 calibration: [0] max |x| of the trunk, [1] max |x_k| of the growth planes (device)
    bool fp8_hp_tail = false;     // S2SR_PREC_FP8: the six head / tail convs in plain fp16 (their ~2e-3 is below the trunk's e4m3
                                  // error) unless S2SR_FP8_TAIL=hp asks for the split-operand forms
    int lo_exp = 12;              // fp16 modes, one-wave-per-SIMD trunk: the trunk's lo half as e4m3(lo * 2^lo_exp): exact to 4 bits for
                                  // |x| < 2^(20 - lo_exp) = 256, clamped beyond (S2SR_LO_EXP)
    int fp8_x_exp = 3, fp8_g_exp = 5;   // S2SR_PREC_FP8 activation scales 2^e of the x / growth planes (S2SR_FP8_XEXP, S2SR_FP8_GEXP); calibrated
                                        // on the synthetic set: profiles/r02_fp8_scale_sweep.txt (|x| up to 56, |x_k| up to 14 before clipping)
    int fp8_x_exp0 = 3, fp8_g_exp0 = 5; // ... as s2sr_create left them: every weight load starts from these again (a calibration belongs to the weights it saw)
    bool graphs_on = true;        // S2SR_GRAPH=0 turns it off
    int64_t ws_allocs = 0;        // workspace (re)allocations since s2sr_create (s2sr_debug_get_config reserved[5])
    bool last_fold = true;        // S2SR_LAST_FOLD=0: conv_last (hp) reads all four e4m3 planes (8 stages) instead of folding w_lo into idle couts
    bool f16_full = true;         // S2SR_F16_FULL=0: fp16 conv1-4 never take the whole-patch form (no px_live arithmetic in the epilogue) on 32-multiple launches
    bool small8 = true;           // S2SR_SMALL8=0: single tiles keep the 16x32-patch form of fp16 conv1-4 (default: 8x32 patches, 256 per 256x256 tile)
    bool mosaic_on = true;        // S2SR_MOSAIC=0: windows that are no multiple of the 32-pixel patch travel one per image (ConvParams::mos_*)
    // paste maps of the window plan last stitched through s2sr_stitch_rows_u8_dev (row map, column map), kept on the device:
    // an AOI is stitched band by band, the maps are uploaded once per (H, W, tile, pad)
    // (a small LRU of map sets: a service that alternates AOI sizes neither re-uploads nor synchronises the device per job)
    struct StitchMaps { int key[4] = {0, 0, 0, 0}; int32_t* d = nullptr; size_t cap = 0; uint64_t last_use = 0; };
    StitchMaps stitch_sets[4];
    uint64_t stitch_clock = 0;
    hipEvent_t host_copy_ev = nullptr;          // s2sr_copy_to_host: orders the copy stream behind the caller's stream
    void* host_arena = nullptr;                 // page-locked host block of the tile-PNG stage (stats back, plan up): grown on demand, kept
    size_t host_arena_bytes = 0;
    // the banded post-process in progress on this handle (s2sr_pp_band_*_dev, enhance_impl): geometry, channel order, how far the
    // CLAHE'd rows and the finished rows reach
    struct PPBand {
        bool open = false, lut = false;
        int H = 0, W = 0, bgr = 0, swap_out = 0, radius = 0;
        int applied_end = 0, rows_end = 0;
        s2sr_pp_params prm{};
    } ppb;
    std::vector<GraphEntry> graphs;
    uint64_t graph_clock = 0;
    int64_t graph_replays = 0, graph_captures = 0;
    // where the last run_net left the trunk output conv_body reads (it differs between the w4, fp8 and 8-wave paths);
    // read by s2sr_debug_forward_taps only
    struct TrunkRec { const char* hi = nullptr; uint64_t hi_img = 0; const char* lo = nullptr; uint64_t lo_img = 0; int lo_exp = -1; } trunk_rec;
    TrunkTap* ttap = nullptr;     // s2sr_debug_trunk_taps' batch is running (run_net taps the trunk at its RDB boundaries); null otherwise
    CompactTap* ctap = nullptr;   // s2sr_debug_compact_taps' batch is running
};

namespace {

int fail(s2sr_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    else g_create_error = msg;
    return code;
}

#define HIPCHK(h, expr)                                                                        \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) {                                                               \
            char b__[512];                                                                     \
            snprintf(b__, sizeof b__, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return fail(h, S2SR_E_HIP, b__);                                                   \
        }                                                                                      \
    } while (0)

struct ConvSpec {
    int cin, cout;
};

std::vector<ConvSpec> conv_specs(int num_block, int scale) {
    std::vector<ConvSpec> v;
    v.push_back({scale == 2 ? 12 : 3, 64});   // conv_first; scale 2 reads the 12 channels of pixel_unshuffle(x, 2)
    for (int b = 0; b < num_block; ++b)
        for (int r = 0; r < 3; ++r)
            for (int k = 1; k <= 5; ++k) v.push_back({64 + (k - 1) * 32, k < 5 ? 32 : 64});
    v.push_back({64, 64});   // conv_body
    v.push_back({64, 64});   // conv_up1
    v.push_back({64, 64});   // conv_up2
    v.push_back({64, 64});   // conv_hr
    v.push_back({64, 3});    // conv_last
    return v;
}

// SRVGGNetCompact(num_feat 64, num_conv, upscale 4): floats of its flat `body` list (conv weight, conv bias, 64 slopes, ...)
size_t compact_blob_floats(int num_conv) {
    return (size_t)(3 * 64 * 9 + 64 + 64) + (size_t)num_conv * (64 * 64 * 9 + 64 + 64) + (size_t)(64 * 48 * 9 + 48);
}
size_t handle_blob_floats(const s2sr_handle* h) {
    return h->compact() ? compact_blob_floats(h->cfg.num_block) : s2sr_expected_blob_floats_scale(h->cfg.num_block, h->cfg.scale);
}

void free_weights(s2sr_handle* h) {
    for (ConvW& c : h->convs) {
        if (!c.pooled && c.d_wpack) dev_free(c.d_wpack);
        for (int k = 0; k < 2; ++k)
            if (c.d_wphase[k]) dev_free(c.d_wphase[k]);
    }
    if (h->pool_w) dev_free(h->pool_w);
    if (h->pool_s) dev_free(h->pool_s);
    if (h->pool_b) dev_free(h->pool_b);
    h->pool_w = nullptr; h->pool_s = nullptr; h->pool_b = nullptr;
    h->convs.clear();
}

void drop_graphs(s2sr_handle* h) {   // buffers or weights moved: every captured pointer is stale
    for (GraphEntry& g : h->graphs)
        if (g.exec) hipGraphExecDestroy(g.exec);
    h->graphs.clear();
}

// A capture that another user of the runtime voided (their hipDeviceSynchronize / hipFree while this handle captured: the device
// gate only covers this library) leaves the stream in the "invalidated" state for good -- hipStreamEndCapture reports the error
// but every later operation on the stream still fails.  The host-facing calls that run on the handle's own stream check for that
// after a failure, replace the stream and run again (inputs are untouched, outputs are rewritten); after three such captures
// the handle stops capturing.  Callers that pass their own stream (the *_dev calls) get the error.
bool recover_stream(s2sr_handle* h) {
    std::lock_guard<std::mutex> lk(h->mu);
    if (hipSetDevice(h->cfg.device) != hipSuccess) return false;
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(h->stream, &status);
    (void)hipGetLastError();
    if (e == hipSuccess && status == hipStreamCaptureStatusNone) return false;       // the failure was something else
    hipStream_t fresh = nullptr;
    if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) != hipSuccess) return false;
    hipStreamDestroy(h->stream);
    (void)hipGetLastError();
    h->stream = fresh;
    drop_graphs(h);
    if (++h->capture_failures >= 3) h->graphs_on = false;
    return true;
}
#define RUN_WITH_STREAM_RECOVERY(h, call)            \
    do {                                             \
        int rc_ = (call);                            \
        if (rc_ != S2SR_OK && (h) && recover_stream(h)) rc_ = (call); \
        return rc_;                                  \
    } while (0)

int ensure_scratch(s2sr_handle* h, int slot, size_t bytes) {
    h->tiles_slot = -1;                  // whoever asks for scratch is about to overwrite it; the pyramid calls set it again
    h->warp_slot = -1;
    if (h->scratch_bytes[slot] >= bytes) return S2SR_OK;
    if (h->d_scratch[slot]) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        drop_graphs(h);
        HIPCHK(h, dev_free(h->d_scratch[slot]));
        h->d_scratch[slot] = nullptr;
        h->scratch_bytes[slot] = 0;
    }
    HIPCHK(h, dev_malloc(&h->d_scratch[slot], bytes));
    h->scratch_bytes[slot] = bytes;
    return S2SR_OK;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Blocking copies / fills go through one of the handle's own (non-blocking) streams, never the legacy stream: the runtime refuses
// any legacy-stream operation (hipMemcpy, hipMemset) while ANY stream of the process captures a graph, and it also invalidates
// that capture -- two handles on two threads (the x4 and the anime engine under Starlette's pool) hit exactly that in the r04 soak.
hipError_t copy_blocking(s2sr_handle* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, h->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}
hipError_t fill_blocking(s2sr_handle* h, void* dst, int value, size_t bytes) {
    hipError_t e = hipMemsetAsync(dst, value, bytes, h->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

// ---- the test hooks' decoders (s2sr_debug_forward_taps, s2sr_debug_trunk_taps)
float e4m3_to_f32(uint8_t b) {   // OCP e4m3fn: bias 7, subnormals, 0x7f / 0xff = NaN
    const int e = (b >> 3) & 15, m = b & 7;
    float v = e == 0 ? ldexpf((float)m, -9) : ldexpf((float)(8 + m), e - 10);
    if ((b & 0x7f) == 0x7f) v = NAN;
    return (b & 0x80) ? -v : v;
}
typedef _Float16 hf16;
struct DevBuf {   // frees on scope exit: the hooks have many early returns
    void* p = nullptr;
    ~DevBuf() { if (p) dev_free(p); }
};
// n images of `nb` planes of `blk` bytes (32 B per pixel) at `img` bytes apart -> buf (blocking, on the handle's stream)
int fetch_planes(s2sr_handle* h, std::vector<uint8_t>& buf, const char* src, uint64_t img, int n, int nb, size_t blk) {
    buf.resize((size_t)n * nb * blk);
    for (int i = 0; i < n; ++i) HIPCHK(h, copy_blocking(h, buf.data() + (size_t)i * nb * blk, src + (size_t)i * img, (size_t)nb * blk, hipMemcpyDeviceToHost));
    return S2SR_OK;
}
// fp16 blocked-16: 16 channels per plane -> dst [n][16 nb][Hp][Wp]
int decode_f16_planes(s2sr_handle* h, float* dst, const char* src, uint64_t img, int n, int nb, size_t blk) {
    std::vector<uint8_t> buf;
    if (int r = fetch_planes(h, buf, src, img, n, nb, blk)) return r;
    const size_t np = blk / 32;
    const hf16* v = (const hf16*)buf.data();
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < nb; ++b)
            for (size_t q = 0; q < np; ++q)
                for (int c = 0; c < 16; ++c)
                    dst[(((size_t)i * nb * 16 + b * 16 + c) * np) + q] = (float)v[(((size_t)i * nb + b) * np + q) * 16 + c];
    return S2SR_OK;
}
// e4m3 planes of 32 channels, plane b's values times scale[b] -> dst [n][32 nb][Hp][Wp]
int decode_e4m3_planes(s2sr_handle* h, float* dst, const char* src, uint64_t img, int n, int nb, size_t blk, const float* scale) {
    std::vector<uint8_t> buf;
    if (int r = fetch_planes(h, buf, src, img, n, nb, blk)) return r;
    const size_t np = blk / 32;
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < nb; ++b)
            for (size_t q = 0; q < np; ++q)
                for (int c = 0; c < 32; ++c)
                    dst[(((size_t)i * nb * 32 + b * 32 + c) * np) + q] = e4m3_to_f32(buf[(((size_t)i * nb + b) * np + q) * 32 + c]) * scale[b];
    return S2SR_OK;
}

int ensure_workspace(s2sr_handle* h, int G, int H, int W, int mos_py = 0, int mos_px = 0) {
    Workspace& w = h->ws;
    const bool fp8 = h->cfg.precision == S2SR_PREC_FP8;
    const bool hp = h->cfg.precision == S2SR_PREC_F16_HP || (fp8 && h->fp8_hp_tail);   // split-operand head / tail convs
    // a mosaic's separator rows / columns are conv zero padding: they must come from the allocation memset, so planes that
    // were written as plain images (or as a mosaic of another period) are not reused
    if (w.base && w.G >= G && w.H == H && w.W == W && w.hp == hp && w.fp8 == fp8 && w.mos_py == mos_py && w.mos_px == mos_px) return S2SR_OK;
    if (w.base) {
        HIPCHK(h, dev_sync());
        drop_graphs(h);
        HIPCHK(h, dev_free(w.base));
        w = Workspace();
    }
    w.G = G; w.H = H; w.W = W; w.hp = hp; w.fp8 = fp8; w.mos_py = mos_py; w.mos_px = mos_px;
    w.Hp = padded(H); w.Wp = padded(W);
    if (h->compact()) {
        // SRVGGNetCompact: the packed input (1 block) and two 64-channel fp16 tensors (D[0], D[1]: 4 blocks each) that the
        // layers ping-pong between -- 288 B per padded LR pixel; everything stays at input resolution
        w.blk1 = (size_t)w.Hp * w.Wp * 32;
        const size_t g = (size_t)G, bP0 = align256(g * w.blk1), bA = align256(g * 4 * w.blk1);
        w.bytes = bP0 + 2 * bA;
        const hipError_t em = dev_malloc(&w.base, w.bytes);
        if (em != hipSuccess) {
            (void)hipGetLastError();
            const size_t want = w.bytes;
            w = Workspace();
            char b[200];
            snprintf(b, sizeof b, "workspace of %.1f GB for %d images of %dx%d: %s", (double)want / 1e9, G, H, W, hipGetErrorString(em));
            return fail(h, em == hipErrorOutOfMemory ? S2SR_E_CAPACITY : S2SR_E_HIP, b);
        }
        HIPCHK(h, fill_blocking(h, w.base, 0, w.bytes));   // the zero halos
        ++h->ws_allocs;
        w.P0 = w.base; w.D[0] = w.base + bP0; w.D[1] = w.base + bP0 + bA;
        return S2SR_OK;
    }
    w.Hp2 = padded(2 * H); w.Wp2 = padded(2 * W);
    w.Hp4 = padded(4 * H); w.Wp4 = padded(4 * W);
    w.blk1 = (size_t)w.Hp * w.Wp * 32; w.blk2 = (size_t)w.Hp2 * w.Wp2 * 32; w.blk4 = (size_t)w.Hp4 * w.Wp4 * 32;
    size_t off = 0;
    auto take = [&](size_t b) { size_t o = off; off += align256(b); return o; };
    const size_t g = (size_t)G;
    const size_t nd = fp8 ? 0 : 12;     // the fp16 dense tensors are not used by the fp8 trunk
    const size_t oP0 = take(g * w.blk1), oD0 = take(g * nd * w.blk1), oD1 = take(g * nd * w.blk1), oD2 = take(g * nd * w.blk1),
                 oU0 = take(g * 4 * w.blk1), oT = take(g * 4 * w.blk1), oT0 = take(g * (fp8 ? 0 : 2) * w.blk1), oT1 = take(g * (fp8 ? 0 : 2) * w.blk1),
                 oT2 = take(g * (fp8 ? 0 : 2) * w.blk1), oR = take(g * 8 * w.blk1),
                 oF = take(g * 8 * w.blk1), oU1 = take(g * 4 * w.blk2), oU2 = take(g * 4 * w.blk4),
                 oU3 = take(g * 4 * w.blk4);
    size_t oU0l = 0, oU1l = 0, oU2l = 0, oU3l = 0;
    size_t oT8 = 0;
    if (hp) {
        oU0l = take(g * 4 * w.blk1); oU1l = take(g * 4 * w.blk2); oU2l = take(g * 4 * w.blk4); oU3l = take(g * 4 * w.blk4);
        oT8 = take(g * 4 * w.blk1);
    }
    size_t oD8[2] = {0, 0}, oXh[3] = {0, 0, 0}, oTz = 0;
    if (fp8) {
        for (int i = 0; i < 2; ++i) oD8[i] = take(g * 6 * w.blk1);
        for (int i = 0; i < 3; ++i) oXh[i] = take(g * 4 * w.blk1);
        oTz = take(g * 4 * w.blk1);
    }
    w.bytes = off;
    {
        const hipError_t em = dev_malloc(&w.base, w.bytes);
        if (em != hipSuccess) {                       // leave a clean "no workspace" state: the caller may retry with a smaller group
            (void)hipGetLastError();
            w = Workspace();
            char b[200];
            snprintf(b, sizeof b, "workspace of %.1f GB for %d images of %dx%d: %s", (double)off / 1e9, G, H, W, hipGetErrorString(em));
            return fail(h, em == hipErrorOutOfMemory ? S2SR_E_CAPACITY : S2SR_E_HIP, b);
        }
    }
    HIPCHK(h, fill_blocking(h, w.base, 0, w.bytes));   // the zero halos
    ++h->ws_allocs;
    w.P0 = w.base + oP0; w.D[0] = w.base + oD0; w.D[1] = w.base + oD1; w.D[2] = w.base + oD2; w.U0 = w.base + oU0;
    w.T = w.base + oT; w.Tr[0] = w.base + oT0; w.Tr[1] = w.base + oT1; w.Tr[2] = w.base + oT2; w.R = (float*)(w.base + oR); w.F = (float*)(w.base + oF);
    w.U1 = w.base + oU1; w.U2 = w.base + oU2; w.U3 = w.base + oU3;
    if (hp) { w.U0lo = w.base + oU0l; w.U1lo = w.base + oU1l; w.U2lo = w.base + oU2l; w.U3lo = w.base + oU3l; w.T8 = w.base + oT8; }
    if (fp8) {
        for (int i = 0; i < 2; ++i) w.D8[i] = w.base + oD8[i];
        for (int i = 0; i < 3; ++i) w.Xh[i] = w.base + oXh[i];
        w.Tz = w.base + oTz;
    }
    return S2SR_OK;
}

hipEvent_t get_event(s2sr_handle* h) {
    if (!h->ev_pool.empty()) {
        hipEvent_t e = h->ev_pool.back();
        h->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

struct Scope {   // brackets one launch with events when profiling is on
    s2sr_handle* h;
    hipStream_t st;
    EvRec r;
    bool on;
    Scope(s2sr_handle* h_, hipStream_t st_, int fam, double flops, double bytes) : h(h_), st(st_), on(false) {
        if (h->prof <= 0) return;
        if (h->span_on && h->span.fam == fam) { h->span.flops += flops; h->span.bytes += bytes; h->span.n += 1; return; }
        on = (h->fam_count[fam]++ % h->prof) == 0;
        if (!on) return;
        r.fam = fam; r.flops = flops; r.bytes = bytes;
        r.e0 = get_event(h); r.e1 = get_event(h);
        hipEventRecord(r.e0, st);
    }
    ~Scope() {
        if (!on) return;
        hipEventRecord(r.e1, st);
        h->evs.push_back(r);
    }
};

// a span: one event pair around the next launches of `fam` (every prof-th span is sampled, the others record nothing at all)
void span_begin(s2sr_handle* h, hipStream_t st, int fam) {
    if (h->prof <= 0 || h->span_on) return;
    const bool sample = (h->span_count++ % h->prof) == 0;
    h->span_on = true;
    h->span = EvRec();
    h->span.fam = fam; h->span.flops = 0; h->span.bytes = 0; h->span.n = 0;
    h->span.e0 = h->span.e1 = nullptr;
    if (sample) { h->span.e0 = get_event(h); h->span.e1 = get_event(h); hipEventRecord(h->span.e0, st); }
}
void span_end(s2sr_handle* h, hipStream_t st) {
    if (!h->span_on) return;
    h->span_on = false;
    if (h->span.e0 && h->span.n > 0) { hipEventRecord(h->span.e1, st); h->evs.push_back(h->span); }
    else if (h->span.e0) { h->ev_pool.push_back(h->span.e0); h->ev_pool.push_back(h->span.e1); }
}

int collect_events(s2sr_handle* h) {
    if (h->evs.empty()) return S2SR_OK;
    HIPCHK(h, dev_sync());
    for (EvRec& r : h->evs) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, r.e0, r.e1);
        s2sr_kstat& s = h->stats[r.fam];
        s.launches += r.n; s.total_ms += ms; s.flops += r.flops; s.bytes += r.bytes;
        h->ev_pool.push_back(r.e0);
        h->ev_pool.push_back(r.e1);
    }
    h->evs.clear();
    return S2SR_OK;
}

// one conv launch
int run_conv(s2sr_handle* h, hipStream_t st, int fam, const ConvW& cw, ConvParams p, int epi, bool up,
             bool lo_out = false, s2sr_debug_trunk_form* form = nullptr) {   // form: where the RDB convs record their kernel form
    p.wpack = cw.d_wpack;
    p.bias = cw.d_bias;
    p.nstage = cw.nstage;
    p.seg_len = cw.seg_len;
    p.seg_lo_mask = cw.seg_lo_mask;
    p.fold_lo = cw.fold ? 1 : 0;
    p.tail_form = h->f16_full ? 0 : 8;
    // conv_hr: a folded conv_last (the last conv) reads x_lo planes only, so the e4m3(x_hi) planes need not be written
    if (fam == F_HR && lo_out && !h->convs.empty() && h->convs.back().f8 && h->convs.back().fold) p.tail_form |= 2;
    p.trash = h->d_trash;
    const double px = (double)p.N * p.H * p.W;
    const double flops = 2.0 * 9.0 * cw.cin * cw.cout * px;
    double bytes = px * (up ? 0.25 : 1.0) * cw.cin * 2.0;   // algorithmic: every input element once
    if (epi == EPI_LAST) bytes += px * 3.0 * ((p.out_u8 ? 1.0 : 0.0) + (p.out_f32 ? 4.0 : 0.0));
    else bytes += px * cw.cout * 2.0;
    // split-operand convs (hp): the e4m3 correction planes they read (4 planes of 32 B per pixel; a folded conv_last reads the
    // two x_lo planes only) and write (4 planes; 2 when the consumer is a folded conv_last)
    if (cw.f8) bytes += px * (up ? 0.25 : 1.0) * (cw.fold ? 64.0 : 128.0);
    if (lo_out) bytes += px * ((p.tail_form & 2) ? 64.0 : 128.0);
    // the trunk's lo half travels as e4m3 planes (1 B per channel)
    if (epi == EPI_RDB5) bytes += px * 64 * 2.0;                        // lo: read + write
    if (epi == EPI_RDB5_RRDB) bytes += px * 64 * (p.xh_skip ? 5.0 : 12.0);    // lo r/w + RRDB skip: (fp16 hi, e4m3 lo) pair read, or fp32 R r/w
    if (epi == EPI_FIRST) bytes += px * 64 * 10.0;        // lo + R + F
    if (epi == EPI_BODY) bytes += px * 64 * 4.0;
    Scope sc(h, st, fam, flops, bytes);
    if (form) *form = s2sr_debug_trunk_form{};
    if ((fam == F_RDB14 || fam == F_RDB5) && !up && !lo_out && !cw.f8) {   // the RRDB trunk: conv_trunk.hip
        p.f16_form = (h->small8 ? 0 : 2) | (h->f16_full ? 0 : 4);
        HIPCHK(h, launch_conv_trunk(p, cw.ct, epi, st, 0, form));
        return S2SR_OK;
    }
    HIPCHK(h, launch_conv(p, cw.ct, epi, up, lo_out, st, cw.f8));
    return S2SR_OK;
}

// conv_up1 / conv_up2 in hp mode: "nearest-2x, then 3x3" as four 2x2-tap convs of the source image, one
// launch per output ROW parity (conv3x3.hip, PH template parameter): 4 MACs per output pixel instead of 9.
// `p` arrives filled for the upsample-on-load form (src / src_lo / dst / T and their image strides).
int run_up_subpixel(s2sr_handle* h, hipStream_t st, const ConvW& cw, ConvParams p, int n, int Hs, int Ws, int sHp, int sWp,
                    int oHp, int oWp) {
    p.N = n; p.H = Hs; p.W = Ws; p.sHp = sHp; p.sWp = sWp; p.Hp = oHp; p.Wp = oWp;
    p.bias = cw.d_bias; p.nstage = cw.f8 ? 8 : 4; p.seg_len = 4; p.seg_lo_mask = cw.f8 ? 0x2 : 0x0; p.fold_lo = 0;
    p.tail_form = h->f16_full ? 0 : 8;
    p.trash = h->d_trash;
    const double px = (double)n * Hs * Ws;
    for (int k = 0; k < 2; ++k) {
        p.wpack = cw.d_wphase[k];
        // statistics keep the nominal work of the 3x3 form (2*9*cin*cout per OUTPUT pixel; one row parity = half of them)
        // bytes per SOURCE pixel and launch: the source block once (fp16 128 B, + 128 B of e4m3 correction planes in the
        // split-operand form), two output pixels (both column parities of this row parity) of 128 B (+ 128 B of planes) each
        // (r03 counted the split-operand figure for the plain fp16 form too: 8.2 TB/s "algorithmic" in the fp8 leg)
        Scope sc(h, st, F_UP, 2.0 * 9.0 * cw.cin * cw.cout * 2.0 * px, px * (cw.f8 ? 768.0 : 384.0));
        HIPCHK(h, launch_conv_phase(p, k, st, cw.f8));
    }
    return S2SR_OK;
}

// s2sr_debug_trunk_taps: the trunk fields at the boundary in front of global RDB g (g = 3 num_block: behind the last one), called
// by run_net before RDB g's first launch.  What RDB g - 1 wrote (the trunk x, its growth planes) is still in place then, and so
// is the RRDB skip a rdb3 is about to read.  Blocking copies: the hook's batch runs eagerly.
int trunk_tap(s2sr_handle* h, hipStream_t st, int g) {
    const TrunkTap& tt = *h->ttap;
    s2sr_debug_trunk_fields* t = tt.t;
    const Workspace& w = h->ws;
    const int n = t->n, j = g - tt.first;
    if (j < 0 || j > tt.count) return S2SR_OK;
    if (w.Hp != t->Hp || w.Wp != t->Wp) return fail(h, S2SR_E_INVALID, "trunk taps: the workspace planes differ from the planned ones");
    HIPCHK(h, hipStreamSynchronize(st));
    const size_t f64 = (size_t)n * 64 * w.Hp * w.Wp;   // floats of one 64-channel field
    const int r = g % 3;
    int rc;
    if (w.fp8) {
        const float sx = ldexpf(1.0f, -h->fp8_x_exp), sg = ldexpf(1.0f, -h->fp8_g_exp), scx[2] = {sx, sx}, scg[4] = {sg, sg, sg, sg};
        if (t->x_hi && (rc = decode_f16_planes(h, t->x_hi + j * f64, w.Xh[r], 4 * w.blk1, n, 4, w.blk1))) return rc;
        if (t->x_lo && (rc = decode_e4m3_planes(h, t->x_lo + j * f64, w.D8[g & 1], 6 * w.blk1, n, 2, w.blk1, scx))) return rc;
        if (j > 0 && t->growth && (rc = decode_e4m3_planes(h, t->growth + (j - 1) * 2 * f64, w.D8[(g - 1) & 1] + 2 * w.blk1, 6 * w.blk1, n, 4, w.blk1, scg)))
            return rc;
        if (j < tt.count && r == 2 && t->skip_hi && (rc = decode_f16_planes(h, t->skip_hi + j * f64, w.Xh[0], 4 * w.blk1, n, 4, w.blk1))) return rc;
    } else {
        const float sl = ldexpf(1.0f, -h->lo_exp), scl[2] = {sl, sl};
        if (t->x_hi && (rc = decode_f16_planes(h, t->x_hi + j * f64, w.D[r], 12 * w.blk1, n, 4, w.blk1))) return rc;
        if (t->x_lo && (rc = decode_e4m3_planes(h, t->x_lo + j * f64, w.Tr[r], 2 * w.blk1, n, 2, w.blk1, scl))) return rc;
        if (j > 0 && t->growth && (rc = decode_f16_planes(h, t->growth + (j - 1) * 2 * f64, w.D[(g + 2) % 3] + 4 * w.blk1, 12 * w.blk1, n, 8, w.blk1)))
            return rc;
        if (j < tt.count && r == 2) {
            if (t->skip_hi && (rc = decode_f16_planes(h, t->skip_hi + j * f64, w.D[0], 12 * w.blk1, n, 4, w.blk1))) return rc;
            if (t->skip_lo && (rc = decode_e4m3_planes(h, t->skip_lo + j * f64, w.Tr[0], 2 * w.blk1, n, 2, w.blk1, scl))) return rc;
        }
        if (g == 0 && t->entry_lo && (rc = decode_f16_planes(h, t->entry_lo, w.T, 4 * w.blk1, n, 4, w.blk1))) return rc;
    }
    return S2SR_OK;
}

// The layer schedule for `n` images already packed into ws.P0.  Exactly the op order of
// RRDBNet.forward (cnn_super_resolution.py:140-158) with ResidualDenseBlock / RRDB inlined
// (:85-91, :103-107).  The torch.cat of the dense block is "the first k blocks of D[cur]",
// never a copy; conv5 writes the next x into the other dense tensor because neighbouring
// workgroups still read this one's x as halo.
// SRVGGNetCompact: first conv, num_conv PReLU convs ping-ponging between D[0] and D[1], the last conv with the pixel-shuffle
// tail.  Every launch works at input resolution (the x4 happens in the last conv's stores), on the 8-wave form of conv3x3.hip.
int run_net_compact(s2sr_handle* h, hipStream_t st, int n, int H, int W, float* d_out_f32, uint8_t* d_out_u8, const Mosaic& mo) {
    Workspace& w = h->ws;
    const int nc = h->cfg.num_block;
    if ((int)h->convs.size() != nc + 2) return fail(h, S2SR_E_NOWEIGHTS, "compact weights are not loaded");
    ConvParams b{};
    b.N = n; b.H = H; b.W = W; b.Hp = w.Hp; b.Wp = w.Wp; b.sHp = w.Hp; b.sWp = w.Wp;
    b.trash = h->d_trash; b.in_scale = 1.0f / 255.0f;
    if (mo.on()) {
        b.mos_py = mo.wh + 1; b.mos_ry = mo.wh; b.mos_px = mo.ww + 1; b.mos_rx = mo.ww;
        b.mos_my = (uint32_t)(0x100000000ull / (uint32_t)b.mos_py) + 1u; b.mos_mx = (uint32_t)(0x100000000ull / (uint32_t)b.mos_px) + 1u;
        b.mos_kx = mo.kx; b.mos_ky = mo.ky; b.mos_count = mo.count;
    }
    const double px = (double)n * H * W;
    auto tap = [&](int layer, const char* act) -> int {       // s2sr_debug_compact_taps only
        if (!h->ctap) return S2SR_OK;
        s2sr_debug_compact_fields* t = h->ctap->t;
        for (int k = 0; k < t->nlayers; ++k)
            if (t->layers[k] == layer && t->act[k]) {
                if (w.Hp != t->Hp || w.Wp != t->Wp) return fail(h, S2SR_E_INVALID, "compact taps: the workspace planes differ from the planned ones");
                HIPCHK(h, hipStreamSynchronize(st));
                if (int r = decode_f16_planes(h, t->act[k], act, 4 * w.blk1, n, 4, w.blk1)) return r;
            }
        return S2SR_OK;
    };
    auto launch = [&](int fam, const ConvW& cw, ConvParams p, int epi, double bytes) -> int {
        p.wpack = cw.d_wpack; p.bias = cw.d_bias; p.slope = cw.d_slope; p.nstage = cw.nstage; p.seg_len = cw.seg_len; p.seg_lo_mask = 0;
        Scope sc(h, st, fam, 2.0 * 9.0 * cw.cin * cw.cout * px, bytes);
        HIPCHK(h, launch_conv(p, cw.ct, epi, false, false, st, false));
        return S2SR_OK;
    };
    int rc, cur = 0;
    {   // first conv 3 -> 64 on the exact 0..255 input, x 1/255 in the epilogue
        ConvParams p = b;
        p.src = w.P0; p.src_img = w.blk1; p.dst = w.D[0]; p.dst_img = 4 * w.blk1;
        if ((rc = launch(F_CFIRST, h->convs[0], p, EPI_CFIRST, px * (32.0 + 128.0)))) return rc;
        if ((rc = tap(0, w.D[0]))) return rc;
    }
    for (int k = 1; k <= nc; ++k) {
        ConvParams p = b;
        p.src = w.D[cur]; p.src_img = 4 * w.blk1; p.dst = w.D[cur ^ 1]; p.dst_img = 4 * w.blk1;
        if ((rc = launch(F_CBODY, h->convs[k], p, EPI_PRELU, px * 256.0))) return rc;   // 128 B read + 128 B written per pixel
        cur ^= 1;
        if ((rc = tap(k, w.D[cur]))) return rc;
    }
    {   // last conv 64 -> 48, pixel_shuffle(4) + nearest-x4 of the input in its stores
        ConvParams p = b;
        p.src = w.D[cur]; p.src_img = 4 * w.blk1;
        p.src_lo = w.P0; p.lo_img = w.blk1;               // the base: this LR pixel's own colour (ConvParams::slope's note)
        p.out_f32 = d_out_f32; p.out_u8 = d_out_u8; p.cout = 3;
        const double ob = px * 48.0 * ((d_out_u8 ? 1.0 : 0.0) + (d_out_f32 ? 4.0 : 0.0));
        if ((rc = launch(F_CLAST, h->convs[nc + 1], p, EPI_CLAST, px * (128.0 + 32.0) + ob))) return rc;
    }
    return S2SR_OK;
}

int run_net(s2sr_handle* h, hipStream_t st, int n, int H, int W, float* d_out_f32, uint8_t* d_out_u8, const Mosaic& mo = Mosaic()) {
    if (h->compact()) return run_net_compact(h, st, n, H, W, d_out_f32, d_out_u8, mo);
    Workspace& w = h->ws;
    const int nb = h->cfg.num_block;
    // window mosaic: every launch gets the separator geometry at the scale of the coordinates its epilogue works in
    auto mosaic_at = [&](ConvParams& q, int scale) {
        if (!mo.on()) return;
        q.mos_py = (mo.wh + 1) * scale; q.mos_ry = mo.wh * scale; q.mos_px = (mo.ww + 1) * scale; q.mos_rx = mo.ww * scale;
        q.mos_my = (uint32_t)(0x100000000ull / (uint32_t)q.mos_py) + 1u; q.mos_mx = (uint32_t)(0x100000000ull / (uint32_t)q.mos_px) + 1u;
        q.mos_kx = mo.kx; q.mos_ky = mo.ky; q.mos_count = mo.count;
    };
    ConvParams b{};
    b.N = n; b.H = H; b.W = W; b.Hp = w.Hp; b.Wp = w.Wp; b.sHp = w.Hp; b.sWp = w.Wp;
    b.T = w.T; b.R = w.R; b.F = w.F;
    mosaic_at(b, 1);
    int ci = 0, rc;
    const bool fp8 = w.fp8;
    {   // conv_first: 3 -> 64 (input = one 16-channel block)
        ConvParams p = b;
        p.src = w.P0; p.src_img = w.blk1; p.in_scale = 1.0f / 255.0f;
        if (fp8) { p.dst = w.Xh[0]; p.dst_img = 4 * w.blk1; }
        else { p.dst = w.D[0]; p.dst_img = 12 * w.blk1; }
        if ((rc = run_conv(h, st, F_FIRST, h->convs[ci++], p, EPI_FIRST, false))) return rc;
    }
    int cur = 0;
    const char* trunk_hi = nullptr;   // fp16 x of the trunk after the body (conv_body's main operand)
    uint64_t trunk_hi_img = 0;
    const char* trunk_lo = nullptr;   // its lo half: fp16 (4 blocks), or e4m3(lo * 2^trunk_lo_exp) planes when trunk_lo_exp >= 0
    int trunk_lo_exp = -1;
    if (fp8) {
        // the trunk on e4m3 operands (conv_trunk.hip, conv_trunk_f8): D8[cur] planes [x(2) | x1 | x2 | x3 | x4]
        const int xe = h->fp8_x_exp, ge = h->fp8_g_exp;
        const double px = (double)n * H * W;
        {
            Scope sc(h, st, F_MISC, 0.0, (double)n * w.Hp * w.Wp * (128.0 + 64.0));
            HIPCHK(h, launch_xh_to_fp8(w.Xh[0], 4 * w.blk1, n, w.Hp, w.Wp, xe, w.D8[0], 6 * w.blk1, st));
        }
        for (int blk = 0; blk < nb; ++blk)
            for (int r = 0; r < 3; ++r) {
                s2sr_debug_trunk_form* fo = nullptr;             // s2sr_debug_trunk_taps only
                if (h->ttap) {
                    if ((rc = trunk_tap(h, st, 3 * blk + r))) return rc;
                    fo = h->ttap->forms(3 * blk + r);
                }
                span_begin(h, st, F_RDB14);                      // conv1..4 of this RDB: one sample
                for (int k = 1; k <= 5; ++k) {
                    if (k == 5) span_end(h, st);
                    const ConvW& cw = h->convs[ci++];
                    ConvParams p = b;
                    p.src = w.D8[cur]; p.src_img = 6 * w.blk1;
                    p.wpack = cw.d_wpack; p.bias = cw.d_bias; p.wscale = cw.d_wscale;
                    p.nstage = cw.nstage; p.seg_len = cw.seg_len; p.trash = h->d_trash;
                    p.x_exp = xe; p.g_exp = ge; p.xh_img = 4 * w.blk1;
                    int epi = EPI_LRELU;
                    double bytes = px * (32.0 * cw.seg_len);                     // algorithmic: every input byte once
                    if (k < 5) {
                        p.dst = w.D8[cur] + (size_t)(2 + (k - 1)) * w.blk1; p.dst_img = 6 * w.blk1;
                        bytes += px * 32.0;
                    } else {
                        p.dst = w.D8[cur ^ 1]; p.dst_img = 6 * w.blk1;
                        p.xh_in = w.Xh[r]; p.xh_out = w.Xh[(r + 1) % 3];
                        epi = EPI_RDB5;
                        bytes += px * (64.0 + 128.0 + 128.0);                     // e4m3 x out, fp16 trunk in + out
                        if (r == 2) { p.xh_skip = w.Xh[0]; epi = EPI_RDB5_RRDB; bytes += px * 128.0; }
                    }
                    Scope sc(h, st, k < 5 ? F_RDB14 : F_RDB5, 2.0 * 9.0 * cw.cin * cw.cout * px, bytes);
                    HIPCHK(h, launch_conv_trunk_f8(p, cw.ct, epi, st, fo ? fo + (k - 1) : nullptr));
                }
                if (h->d_calib) {   // s2sr_calibrate_fp8: ranges of this RDB's growth planes and of the trunk it produced
                    HIPCHK(h, launch_absmax_e4m3(w.D8[cur] + 2 * w.blk1, (size_t)4 * w.blk1, ge, h->d_calib + 1, st));
                    for (int i2 = 1; i2 < n; ++i2)
                        HIPCHK(h, launch_absmax_e4m3(w.D8[cur] + (size_t)i2 * 6 * w.blk1 + 2 * w.blk1, (size_t)4 * w.blk1, ge, h->d_calib + 1, st));
                    HIPCHK(h, launch_absmax_f16(w.Xh[(r + 1) % 3], (size_t)n * 4 * w.blk1 / 2, h->d_calib, st));
                }
                cur ^= 1;
            }
        if (h->ttap && (rc = trunk_tap(h, st, 3 * nb))) return rc;
        trunk_hi = w.Xh[0]; trunk_hi_img = 4 * w.blk1; trunk_lo = w.Tz;
    } else {
        // one-wave-per-SIMD trunk kernel: rdb r of every RRDB reads D[r] / Tr[r] and writes the next trunk (x, lo) into
        // D[(r+1)%3] / Tr[(r+1)%3]; rdb3's conv5 takes the RRDB skip from (D[0] x blocks, Tr[0]) -- still the RRDB's
        // input -- and overwrites exactly those pixels (same lane reads, then writes; nobody else touches D[0] then)
        // The lo half travels as e4m3(lo * 2^lo_exp) planes (half the bytes; 4 significant bits of it keep the net inside 3e-4,
        // DESIGN.md section 3): conv_first's fp16 lo is converted once on the way in.
        {
            Scope sc(h, st, F_MISC, 0.0, (double)n * w.Hp * w.Wp * (128.0 + 64.0));
            HIPCHK(h, launch_xh_to_fp8(w.T, 4 * w.blk1, n, w.Hp, w.Wp, h->lo_exp, w.Tr[0], 2 * w.blk1, st));
        }
        for (int blk = 0; blk < nb; ++blk)
            for (int r = 0; r < 3; ++r) {
                const int nx = (r + 1) % 3;
                s2sr_debug_trunk_form* fo = nullptr;             // s2sr_debug_trunk_taps only
                if (h->ttap) {
                    if ((rc = trunk_tap(h, st, 3 * blk + r))) return rc;
                    fo = h->ttap->forms(3 * blk + r);
                }
                span_begin(h, st, F_RDB14);                      // conv1..4 of this RDB: one sample
                for (int k = 1; k <= 4; ++k) {
                    ConvParams p = b;
                    p.src = w.D[r]; p.src_img = 12 * w.blk1;
                    p.dst = w.D[r] + (size_t)(4 + 2 * (k - 1)) * w.blk1; p.dst_img = 12 * w.blk1;
                    if ((rc = run_conv(h, st, F_RDB14, h->convs[ci++], p, EPI_LRELU, false, false, fo ? fo + (k - 1) : nullptr))) { span_end(h, st); return rc; }
                }
                span_end(h, st);
                ConvParams p = b;
                p.src = w.D[r]; p.src_img = 12 * w.blk1;
                p.dst = w.D[nx]; p.dst_img = 12 * w.blk1;
                p.xh_in = w.Tr[r]; p.T = w.Tr[nx]; p.lo_exp = h->lo_exp;
                if (r == 2) { p.xh_skip = w.D[0]; p.xh_img = 12 * w.blk1; p.lo_skip = w.Tr[0]; }
                if ((rc = run_conv(h, st, F_RDB5, h->convs[ci++], p, r == 2 ? EPI_RDB5_RRDB : EPI_RDB5, false, false, fo ? fo + 4 : nullptr))) return rc;
            }
        if (h->ttap && (rc = trunk_tap(h, st, 3 * nb))) return rc;
        trunk_hi = w.D[0]; trunk_hi_img = 12 * w.blk1; trunk_lo = w.Tr[0]; trunk_lo_exp = h->lo_exp;
    }
    h->trunk_rec = {trunk_hi, trunk_hi_img, trunk_lo, (uint64_t)(trunk_lo_exp >= 0 ? 2 : 4) * w.blk1, trunk_lo_exp};
    const bool hp = w.hp;   // split-operand head/tail: inputs as (hi, lo) pairs, outputs write both halves
    {   // conv_body + global skip; its input is the trunk: hi = x, lo = trunk lo (all zero in fp8 mode: the trunk is fp16 there)
        ConvParams p = b;
        p.src = trunk_hi; p.src_img = trunk_hi_img; p.dst = w.U0; p.dst_img = 4 * w.blk1;
        if (hp) {
            Scope sc(h, st, F_MISC, 0.0, (double)n * w.Hp * w.Wp * (256.0 + 128.0));
            HIPCHK(h, launch_trunk_to_fp8(trunk_hi, trunk_hi_img, trunk_lo, (trunk_lo_exp >= 0 ? 2 : 4) * w.blk1, trunk_lo_exp, n, w.Hp, w.Wp, w.T8, st));
            p.src_lo = w.T8; p.lo_img = 4 * w.blk1; p.T = w.U0lo;
        }
        if ((rc = run_conv(h, st, F_BODY, h->convs[ci++], p, EPI_BODY, false, hp))) return rc;
    }
    {   // conv_up1 on nearest-2x
        ConvParams p{};
        p.N = n; p.H = 2 * H; p.W = 2 * W; p.Hp = w.Hp2; p.Wp = w.Wp2; p.sHp = w.Hp; p.sWp = w.Wp;
        p.src = w.U0; p.src_img = 4 * w.blk1; p.dst = w.U1; p.dst_img = 4 * w.blk2;
        if (hp) { p.src_lo = w.U0lo; p.lo_img = 4 * w.blk1; p.T = w.U1lo; }
        mosaic_at(p, 1);                                         // sub-pixel form: the epilogue walks SOURCE pixels
        if ((rc = run_up_subpixel(h, st, h->convs[ci++], p, n, H, W, w.Hp, w.Wp, w.Hp2, w.Wp2))) return rc;
    }
    {   // conv_up2 on nearest-2x
        ConvParams p{};
        p.N = n; p.H = 4 * H; p.W = 4 * W; p.Hp = w.Hp4; p.Wp = w.Wp4; p.sHp = w.Hp2; p.sWp = w.Wp2;
        p.src = w.U1; p.src_img = 4 * w.blk2; p.dst = w.U2; p.dst_img = 4 * w.blk4;
        if (hp) { p.src_lo = w.U1lo; p.lo_img = 4 * w.blk2; p.T = w.U2lo; }
        mosaic_at(p, 2);
        if ((rc = run_up_subpixel(h, st, h->convs[ci++], p, n, 2 * H, 2 * W, w.Hp2, w.Wp2, w.Hp4, w.Wp4))) return rc;
    }
    ConvParams hr{};
    hr.N = n; hr.H = 4 * H; hr.W = 4 * W; hr.Hp = w.Hp4; hr.Wp = w.Wp4; hr.sHp = w.Hp4; hr.sWp = w.Wp4;
    mosaic_at(hr, 4);
    {
        ConvParams p = hr;
        p.src = w.U2; p.src_img = 4 * w.blk4; p.dst = w.U3; p.dst_img = 4 * w.blk4;
        if (hp) { p.src_lo = w.U2lo; p.lo_img = 4 * w.blk4; p.T = w.U3lo; }
        if ((rc = run_conv(h, st, F_HR, h->convs[ci++], p, EPI_LRELU, false, hp))) return rc;
    }
    {
        ConvParams p = hr;
        p.src = w.U3; p.src_img = 4 * w.blk4; p.out_f32 = d_out_f32; p.out_u8 = d_out_u8; p.cout = 3;
        if (hp) { p.src_lo = w.U3lo; p.lo_img = 4 * w.blk4; }
        if ((rc = run_conv(h, st, F_LAST, h->convs[ci++], p, EPI_LAST, false))) return rc;
    }
    return S2SR_OK;
}

constexpr int kCompactGroup = 16;
int group_size(const s2sr_handle* h, int B, int H, int W) {
    // default group: 16 images per launch sequence; the fp8 trunk's launches are half as long, so it takes 32 (measured:
    // 50.5 vs 51.9 ms per 32-tile step; the fp16 modes gain nothing from 32)
    int g = h->cfg.group > 0 ? h->cfg.group : (h->cfg.precision == S2SR_PREC_FP8 ? 32 : 16);
    if (h->compact()) {
        // SRVGGNetCompact: 288 B per padded LR pixel.  Default group: kCompactGroup, from the sweep of tools/bench_compact.py
        // (profiles/compact_group_sweep.txt)
        if (h->cfg.group <= 0) g = kCompactGroup;
        const double per_c = (double)padded(H) * padded(W) * 288.0;
        while (g > 1 && per_c * g > 96.0 * 1024 * 1024 * 1024) --g;
        if (g > B) g = B;
        return g < 1 ? 1 : g;
    }
    // keep the workspace within a third of the 288 GB: bytes per LR pixel 32 + 3*384 (dense) + 128 + 3*128 (lo) + 2*256
    // (fp32 skips) + 2*128 (hp planes); 2x and 4x tensors with their correction planes
    const double per_img = (double)padded(H) * padded(W) * 2500.0 + (double)padded(2 * H) * padded(2 * W) * 256.0 +
                           (double)padded(4 * H) * padded(4 * W) * 512.0;
    while (g > 1 && per_img * g > 96.0 * 1024 * 1024 * 1024) --g;
    if (g > B) g = B;
    return g < 1 ? 1 : g;
}

// Window mosaics: when the tiles are not a multiple of the 32-pixel patch (the reference's 276 x 276 windows: 288 x 288 of patch
// area each, 9 % dead MFMA work) and there are several of them, kx x ky windows share one image with a zero row / column
// between neighbours (ConvParams::mos_*): 4 x 4 windows of 276 -> 1107 x 1107 -> 1120 x 1120 of patch area, 280 per window.
// Same bytes out: every output pixel accumulates the same products in the same order wherever its window sits.
//
// B windows travel as floor(B / per) FULL mosaics of kx x ky plus, for the remainder, ONE smaller mosaic of kx' x ky' (ky' =
// the window rows the remainder needs; a single row is cut to the windows it has).  A sub-mosaic lives inside the planes of the
// full one: its first row / column past the end is a separator position of the full geometry, which no launch ever stores to.
// The choice is made on what is LAUNCHED (r03 ADVICE: dividing the mosaic's area by kx * ky assumes every mosaic is full, and a
// partly filled one costs as much as a full one -- 17 windows of 276 as two 4 x 4 mosaics launched 78 % more patches than 17 plain images).
static void mosaic_remainder(int rem, int kx, int ky, int* rkx, int* rky) {
    *rky = (rem + kx - 1) / kx;
    if (*rky > ky) *rky = ky;
    *rkx = (*rky == 1) ? rem : kx;
}
static long mosaic_area(int th, int tw, int kx, int ky) {   // 32 x 32 patches of one kx x ky mosaic image
    return (long)(roundup32(ky * (th + 1) - 1) / 32) * (roundup32(kx * (tw + 1) - 1) / 32);
}
static long mosaic_patches(int B, int th, int tw, int kx, int ky) {   // patches launched for B windows
    const int per = kx * ky, full = B / per, rem = B % per;
    long a = (long)full * mosaic_area(th, tw, kx, ky);
    if (rem) { int rkx, rky; mosaic_remainder(rem, kx, ky, &rkx, &rky); a += mosaic_area(th, tw, rkx, rky); }
    return a;
}
static Mosaic pick_mosaic_cfg(bool mosaic_on, int B, int th, int tw);
// th x tw: input windows; the mosaic is laid out on the trunk grid (its wh x ww are trunk sizes)
Mosaic pick_mosaic(const s2sr_handle* h, int B, int th, int tw) { return pick_mosaic_cfg(h->mosaic_on, B, th / h->unshuffle(), tw / h->unshuffle()); }
// pure host arithmetic (s2sr_debug_pick_mosaic exposes it to the CPU tests)
static Mosaic pick_mosaic_cfg(bool mosaic_on, int B, int th, int tw) {
    Mosaic m;
    if (!mosaic_on || B < 2) return m;
    const long plain = (long)B * (roundup32(th) / 32) * (roundup32(tw) / 32);
    if ((double)roundup32(th) * roundup32(tw) < 1.03 * (double)th * tw) return m;   // 256 x 256 tiles and friends: nothing to gain
    auto side = [](int win) {                         // windows per mosaic side: at most 8, mosaic at most ~1280 px (workspace: 4x tensors)
        int k = 1280 / (win + 1);
        return k > 8 ? 8 : (k < 1 ? 1 : k);
    };
    const int mx = side(tw), my = side(th);
    // a remainder mosaic is one more sequence of 351 launches on a small image: priced as 64 patches (its launches' floor)
    auto cost = [&](int kx, int ky) { return mosaic_patches(B, th, tw, kx, ky) + ((B % (kx * ky)) ? 64 : 0); };
    long lowest = plain;
    for (int ky = 1; ky <= my; ++ky)
        for (int kx = 1; kx <= mx; ++kx)
            if (kx * ky >= 2 && kx * ky <= B && cost(kx, ky) < lowest) lowest = cost(kx, ky);
    // the LARGEST mosaic within 2 % of the fewest patches (fewer, longer launches: whole rounds of the 256 persistent workgroups
    // and the launch floors amortise; 256 windows of 276: 3 x 3 launches 1 % fewer patches than 4 x 4 but leaves a remainder in
    // every chunk of an AOI), then the wider one
    long best = plain;
    int bkx = 1, bky = 1;
    for (int ky = 1; ky <= my; ++ky)
        for (int kx = 1; kx <= mx; ++kx) {
            if (kx * ky < 2 || kx * ky > B) continue;
            const long a = cost(kx, ky);
            if ((double)a > 1.02 * (double)lowest || a > plain) continue;
            if (kx * ky > bkx * bky || (kx * ky == bkx * bky && (a < best || (a == best && kx > bkx)))) { best = a; bkx = kx; bky = ky; }
        }
    if (bkx * bky >= 2) best = mosaic_patches(B, th, tw, bkx, bky);
    if (bkx * bky < 2 || (double)best > 0.98 * (double)plain) return Mosaic();
    m.kx = bkx; m.ky = bky; m.wh = th; m.ww = tw; m.count = B;
    return m;
}

// [B,th,tw,3] u8 (device) -> u8 [B,S th,S tw,3] and/or f32 [B,3,S th,S tw] (device), S = cfg.scale.  At scale 2 th and tw are even
// and the net runs on the th/2 x tw/2 trunk grid.  `src_h` x `src_w` (0: th x tw): the rows / columns the single input image holds
// when it is one short of th / tw (scale 2, odd image: the packer reads the reflect row / column by index).
// `plan`: the mosaic chosen for the whole job this call is a part of (a chunk of an AOI, a group of a batch) -- its geometry
// sizes the workspace, so every part of the job runs in the same planes (r03 ADVICE: re-picking the mosaic from each chunk's own
// window count gave a short last chunk another image height, and with it a workspace reallocation, a device synchronise and
// dropped graphs inside the chunk loop, on every call).  nullptr: choose from B.
int forward_dev(s2sr_handle* h, hipStream_t st, const uint8_t* d_tiles, const float* d_x_f32, int B, int th, int tw,
                uint8_t* d_out_u8, float* d_out_f32, const Mosaic* plan = nullptr, int src_h = 0, int src_w = 0) {
    if (!h->has_weights) return fail(h, S2SR_E_NOWEIGHTS, "s2sr_load_weights has not been called");
    if (B <= 0 || th <= 0 || tw <= 0) return fail(h, S2SR_E_INVALID, "bad batch/tile dims");
    const int u = h->unshuffle();
    if (th % u || tw % u) {
        char b[200];
        snprintf(b, sizeof b, "tiles of %d x %d: a scale-2 handle (pixel_unshuffle by 2) needs even tile sizes", th, tw);
        return fail(h, S2SR_E_INVALID, b);
    }
    const int sh = src_h ? src_h : th, sw = src_w ? src_w : tw;     // input rows / columns as stored
    const int TH = th / u, TW = tw / u;                            // the trunk grid: what the schedule, workspace and graphs see
    // u8 tiles may travel as window mosaics; "images" below are then mosaics of per = kx*ky windows
    const Mosaic mo = !d_tiles ? Mosaic() : (plan ? *plan : pick_mosaic(h, B, th, tw));
    const int per = mo.on() ? mo.kx * mo.ky : 1;
    const int IH = mo.on() ? mo.ky * (TH + 1) - 1 : TH, IW = mo.on() ? mo.kx * (TW + 1) - 1 : TW;   // the plan's image: the workspace geometry
    const int NIplan = ((plan && plan->count > B ? plan->count : B) + per - 1) / per;
    int G = group_size(h, NIplan, IH, IW);
    int rc = ensure_workspace(h, G, IH, IW, mo.on() ? TH + 1 : 0, mo.on() ? TW + 1 : 0);
    while (rc == S2SR_E_CAPACITY && G > 1) {          // the card is shared: fall back to smaller launch groups rather than fail the job
        G = (G + 1) / 2;
        rc = ensure_workspace(h, G, IH, IW, mo.on() ? TH + 1 : 0, mo.on() ? TW + 1 : 0);
    }
    if (rc) return rc;
    Workspace& w = h->ws;
    const size_t opx = (size_t)16 * TH * TW;          // output pixels per tile: the x4 tail on the trunk grid
    // segments of equal image geometry: the full mosaics, then the remainder as one smaller mosaic
    struct Seg { int t0, nwin, kx, ky; };
    Seg segs[2];
    int nseg = 0;
    if (!mo.on()) segs[nseg++] = Seg{0, B, 1, 1};
    else {
        const int full = B / per, rem = B % per;
        if (full) segs[nseg++] = Seg{0, full * per, mo.kx, mo.ky};
        if (rem) { Seg r{full * per, rem, 1, 1}; mosaic_remainder(rem, mo.kx, mo.ky, &r.kx, &r.ky); segs[nseg++] = r; }
    }
    for (int si = 0; si < nseg; ++si) {
    const Seg& sg = segs[si];
    const int sper = sg.kx * sg.ky;
    const int NI = (sg.nwin + sper - 1) / sper;                                // images of this segment
    const int SH = mo.on() ? sg.ky * (TH + 1) - 1 : TH, SW = mo.on() ? sg.kx * (TW + 1) - 1 : TW;
    for (int g0 = 0; g0 < NI; g0 += G) {
        const int n = (NI - g0 < G) ? (NI - g0) : G;
        const int t0 = sg.t0 + g0 * sper;                                     // first window / tile of this group
        const int nt = (sg.t0 + sg.nwin - t0 < n * sper) ? (sg.t0 + sg.nwin - t0) : n * sper;   // windows / tiles in it
        const uint8_t* in8 = d_tiles ? d_tiles + (size_t)t0 * sh * sw * 3 : nullptr;
        const float* in32 = d_tiles ? nullptr : d_x_f32 + (size_t)t0 * 3 * th * tw;
        float* o32 = d_out_f32 ? d_out_f32 + (size_t)t0 * 3 * opx : nullptr;
        uint8_t* o8 = d_out_u8 ? d_out_u8 + (size_t)t0 * 3 * opx : nullptr;
        Mosaic mg = mo;
        mg.kx = sg.kx; mg.ky = sg.ky; mg.count = nt;
        auto enqueue = [&]() -> int {
            {
                Scope sc(h, st, F_PACK, 0.0, (double)nt * th * tw * (3.0 + 8.0));   // (scale 2: 32 B per trunk pixel = 8 per input pixel)
                if (u == 2) {      // pixel_unshuffle(x, 2) folded into the packers
                    if (in8 && mo.on()) HIPCHK(h, launch_pack_u8_unshuffle_mosaic(in8, nt, TH, TW, sg.kx, sg.ky, w.P0, w.Hp, w.Wp, st));
                    else if (in8) HIPCHK(h, launch_pack_u8_unshuffle(in8, n, sh, sw, TH, TW, w.P0, w.Hp, w.Wp, st));
                    else HIPCHK(h, launch_pack_f32_nchw_unshuffle(in32, n, TH, TW, 255.0f, w.P0, w.Hp, w.Wp, st));
                } else if (in8 && mo.on()) HIPCHK(h, launch_pack_u8_mosaic(in8, nt, th, tw, sg.kx, sg.ky, w.P0, w.Hp, w.Wp, st));
                else if (in8) HIPCHK(h, launch_pack_u8(in8, n, th, tw, w.P0, w.Hp, w.Wp, st));
                else HIPCHK(h, launch_pack_f32_nchw(in32, n, 3, th, tw, 255.0f, w.P0, 1, w.Hp, w.Wp, st));
            }
            return run_net(h, st, n, SH, SW, o32, o8, mo.on() ? mg : Mosaic());
        };
        // the legacy null stream cannot be captured; profiling wants its events between launches
        GraphEntry* ge = nullptr;
        if (h->graphs_on && h->prof <= 0 && st != nullptr) {
            for (GraphEntry& g : h->graphs)
                if (g.n == n && g.th == th && g.tw == tw && g.sh == sh && g.sw == sw && g.in_u8 == in8 && g.in_f32 == in32 && g.out_u8 == o8 &&
                    g.out_f32 == o32 && g.st == st && g.mos_kx == (mo.on() ? sg.kx : 0) && g.mos_ky == (mo.on() ? sg.ky : 0) &&
                    g.mos_count == (mo.on() ? nt : 0)) { ge = &g; break; }
            if (!ge) {   // first sighting: remember it, launch directly (also warms the per-kernel attributes)
                if (h->graphs.size() >= 24) {
                    size_t victim = 0;
                    for (size_t i = 1; i < h->graphs.size(); ++i)
                        if (h->graphs[i].last_use < h->graphs[victim].last_use) victim = i;
                    if (h->graphs[victim].exec) hipGraphExecDestroy(h->graphs[victim].exec);
                    h->graphs.erase(h->graphs.begin() + victim);
                }
                GraphEntry g;
                g.n = n; g.th = th; g.tw = tw; g.sh = sh; g.sw = sw; g.in_u8 = in8; g.in_f32 = in32; g.out_u8 = o8; g.out_f32 = o32; g.st = st;
                g.mos_kx = mo.on() ? sg.kx : 0; g.mos_ky = mo.on() ? sg.ky : 0; g.mos_count = mo.on() ? nt : 0;
                g.last_use = ++h->graph_clock;
                h->graphs.push_back(g);
                ge = nullptr;
            } else if (!ge->exec && !ge->refused) {   // second sighting: capture
                hipGraph_t graph = nullptr;
                DeviceGate gate;     // no device-wide call of any handle while this one captures (s2sr_internal.h)
                bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
                if (ok) {
                    const int erc = enqueue();
                    const hipError_t ee = hipStreamEndCapture(st, &graph);
                    ok = (erc == S2SR_OK) && ee == hipSuccess && graph != nullptr;
                }
                if (ok) ok = hipGraphInstantiate(&ge->exec, graph, nullptr, nullptr, 0) == hipSuccess;
                if (graph) hipGraphDestroy(graph);
                if (!ok) {
                    (void)hipGetLastError();
                    ge->exec = nullptr;
                    ge->refused = true;
                    ge = nullptr;
                } else {
                    ++h->graph_captures;
                }
            } else if (ge->refused) {
                ge = nullptr;
            }
        }
        if (ge && ge->exec) {
            ge->last_use = ++h->graph_clock;
            HIPCHK(h, hipGraphLaunch(ge->exec, st));
            ++h->graph_replays;
        } else {
            rc = enqueue();
            if (rc) return rc;
        }
    }
    }
    return S2SR_OK;
}

}  // namespace

// ==========================================================================================
// C ABI
// ==========================================================================================
extern "C" {

const char* s2sr_version(void) {
    return "s2sr 0.4 (gfx950, fp16-MFMA implicit-GEMM conv)";
}

int s2sr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

size_t s2sr_expected_blob_floats_scale(int32_t num_block, int32_t scale) {
    if (scale != 2 && scale != 4) return 0;
    size_t n = 0;
    for (const ConvSpec& s : conv_specs(num_block, scale)) n += (size_t)s.cin * s.cout * 9 + s.cout;
    return n;
}

size_t s2sr_expected_blob_floats(int32_t num_block) { return s2sr_expected_blob_floats_scale(num_block, 4); }

size_t s2sr_expected_blob_floats_cfg(const s2sr_config* cfg) {
    if (!cfg) return 0;
    if (cfg->arch == S2SR_ARCH_COMPACT)
        return ((cfg->num_block == 16 || cfg->num_block == 32) && cfg->num_feat == 64 && cfg->scale == 4) ? compact_blob_floats(cfg->num_block) : 0;
    if (cfg->arch != S2SR_ARCH_RRDB || cfg->num_block <= 0 || cfg->num_feat != 64 || cfg->num_grow != 32) return 0;
    return s2sr_expected_blob_floats_scale(cfg->num_block, cfg->scale);
}

const char* s2sr_last_error(const s2sr_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int s2sr_create(const s2sr_config* cfg, s2sr_handle** out) {
    if (!cfg || !out) return fail(nullptr, S2SR_E_INVALID, "null argument");
    *out = nullptr;
    if (cfg->arch != S2SR_ARCH_RRDB && cfg->arch != S2SR_ARCH_COMPACT) return fail(nullptr, S2SR_E_INVALID, "unknown arch (S2SR_ARCH_RRDB or S2SR_ARCH_COMPACT)");
    if (cfg->arch == S2SR_ARCH_COMPACT) {
        if ((cfg->num_block != 16 && cfg->num_block != 32) || cfg->num_feat != 64 || cfg->scale != 4)
            return fail(nullptr, S2SR_E_INVALID, "unsupported compact net shape (need num_conv = num_block in {16, 32}, num_feat=64, scale=4)");
        if (cfg->precision == S2SR_PREC_FP8) return fail(nullptr, S2SR_E_INVALID, "the compact arch has no fp8 mode");
    } else if (cfg->num_block <= 0 || cfg->num_feat != 64 || cfg->num_grow != 32 || (cfg->scale != 4 && cfg->scale != 2))
        return fail(nullptr, S2SR_E_INVALID, "unsupported net shape (need num_feat=64, num_grow=32, scale=4 or 2)");
    if (cfg->precision != S2SR_PREC_F16 && cfg->precision != S2SR_PREC_F16_HP && cfg->precision != S2SR_PREC_FP8)
        return fail(nullptr, S2SR_E_INVALID, "unknown precision");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, S2SR_E_NODEVICE, "no HIP device visible; libs2sr has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, S2SR_E_INVALID, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
        return fail(nullptr, S2SR_E_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, S2SR_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is gfx950-only");
    s2sr_handle* h = new s2sr_handle();
    h->cfg = *cfg;
    if (hipSetDevice(cfg->device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(nullptr, S2SR_E_HIP, "hipStreamCreate failed");
    }
    if (hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking) != hipSuccess) {
        hipStreamDestroy(h->stream);
        delete h;
        return fail(nullptr, S2SR_E_HIP, "hipStreamCreate failed");
    }
    // The ten run-time switches of the shipped library (each fixed at creation, reported by s2sr_debug_get_config, each with a
    // byte-identity or tolerance test): S2SR_GRAPH, S2SR_MOSAIC, S2SR_SMALL8, S2SR_F16_FULL, S2SR_LAST_FOLD, S2SR_D2H_STAGED,
    // S2SR_FP8_TAIL, S2SR_LO_EXP, S2SR_FP8_XEXP, S2SR_FP8_GEXP.
    if (const char* g = getenv("S2SR_GRAPH")) h->graphs_on = atoi(g) != 0;
    if (const char* g = getenv("S2SR_MOSAIC")) h->mosaic_on = atoi(g) != 0;
    if (const char* g = getenv("S2SR_SMALL8")) h->small8 = atoi(g) != 0;
    if (const char* g = getenv("S2SR_F16_FULL")) h->f16_full = atoi(g) != 0;
    if (const char* g = getenv("S2SR_LAST_FOLD")) h->last_fold = atoi(g) != 0;
    if (const char* g = getenv("S2SR_D2H_STAGED")) h->d2h_staged_on = atoi(g) != 0;
    if (const char* g = getenv("S2SR_FP8_TAIL")) h->fp8_hp_tail = strcmp(g, "hp") == 0;
    if (const char* g = getenv("S2SR_LO_EXP")) {
        const int v = atoi(g);
        if (v >= 6 && v <= 18) h->lo_exp = v;
    }
    if (const char* g = getenv("S2SR_FP8_XEXP")) h->fp8_x_exp = atoi(g);
    if (const char* g = getenv("S2SR_FP8_GEXP")) h->fp8_g_exp = atoi(g);
    h->fp8_x_exp0 = h->fp8_x_exp; h->fp8_g_exp0 = h->fp8_g_exp;
    if (dev_malloc(&h->d_trash, 8192) != hipSuccess) {
        hipStreamDestroy(h->copy_stream);
        hipStreamDestroy(h->stream);
        delete h;
        return fail(nullptr, S2SR_E_HIP, "hipMalloc failed");
    }
    for (int i = 0; i < F_COUNT; ++i) {
        memset(&h->stats[i], 0, sizeof(s2sr_kstat));
        snprintf(h->stats[i].name, sizeof h->stats[i].name, "%s", kFamName[i]);
    }
    *out = h;
    return S2SR_OK;
}

void s2sr_destroy(s2sr_handle* h) {
    if (!h) return;
    hipSetDevice(h->cfg.device);
    dev_sync();
    drop_graphs(h);
    free_weights(h);
    if (h->ws.base) dev_free(h->ws.base);
    if (h->d_trash) dev_free(h->d_trash);
    for (int i = 0; i < 6; ++i)
        if (h->d_scratch[i]) dev_free(h->d_scratch[i]);
    for (EvRec& r : h->evs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    for (hipEvent_t e : h->ev_pool) hipEventDestroy(e);
    for (hipEvent_t e : h->group_done) hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
        if (h->stage_buf[i]) host_free(h->stage_buf[i]);
        if (h->stage_ev[i]) hipEventDestroy(h->stage_ev[i]);
    }
    for (auto& m : h->stitch_sets)
        if (m.d) dev_free(m.d);
    if (h->host_arena) host_free(h->host_arena);
    if (h->host_copy_ev) hipEventDestroy(h->host_copy_ev);
    if (h->copy_stream) hipStreamDestroy(h->copy_stream);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

// Weights in, by either door.  `d_blob` is the fp32 blob ON THE DEVICE (the host entry uploads it first): the 345 RDB convs
// are repacked by device kernels straight from it (pack.hip), every bias is gathered on the device; only the six head/tail
// convs (0.9 MB of the 67 MB) come back to the host, because their split-operand / sub-pixel packers are host code.
// SRVGGNetCompact: 1.2 M parameters -- the blob comes to the host whole and every conv goes through pack_conv_weights (plain
// fp16, one segment).  The last conv's 48 output channels are placed in the rows the pixel-shuffle epilogue wants
// (compact_last_row_channel); bias and slopes stay fp32.
static int load_weights_compact(s2sr_handle* h, const float* d_blob, size_t n_floats, hipStream_t st) {
    const int nc = h->cfg.num_block;
    const size_t want = compact_blob_floats(nc);
    if (n_floats != want) {
        char b[160];
        snprintf(b, sizeof b, "weight blob has %zu floats, a compact net of %d convs needs %zu", n_floats, nc, want);
        return fail(h, S2SR_E_BADBLOB, b);
    }
    HIPCHK(h, dev_sync());
    drop_graphs(h);
    free_weights(h);
    h->has_weights = false;
    std::vector<float> blob(n_floats);
    HIPCHK(h, hipMemcpyAsync(blob.data(), d_blob, n_floats * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    const int nconv = nc + 2;
    std::vector<float> pb((size_t)nconv * 128, 0.f);     // per conv: [64 bias | 64 slopes]
    HIPCHK(h, dev_malloc(&h->pool_b, pb.size() * sizeof(float)));
    std::vector<char> tmp;
    std::vector<float> wperm((size_t)64 * 64 * 9);
    size_t off = 0;
    for (int idx = 0; idx < nconv; ++idx) {
        const int cin = idx == 0 ? 3 : 64, cout = idx == nconv - 1 ? 48 : 64;
        const float* wsrc = blob.data() + off; off += (size_t)cin * cout * 9;
        const float* bsrc = blob.data() + off; off += cout;
        float* bias = pb.data() + (size_t)idx * 128;
        ConvW cw;
        cw.cin = cin; cw.cout = cout; cw.ct = 2; cw.seg_len = (cin + 15) / 16; cw.nstage = cw.seg_len; cw.seg_lo_mask = 0;
        const float* pw = wsrc;
        if (idx == nconv - 1) {     // rows in the epilogue's order, idle rows zero
            std::fill(wperm.begin(), wperm.end(), 0.f);
            for (int row = 0; row < 64; ++row) {
                const int ch = compact_last_row_channel(row);
                if (ch < 0) continue;
                memcpy(&wperm[(size_t)row * 64 * 9], wsrc + (size_t)ch * 64 * 9, sizeof(float) * 64 * 9);
                bias[row] = bsrc[ch];
            }
            pw = wperm.data();
        } else {
            memcpy(bias, bsrc, sizeof(float) * 64);
            memcpy(bias + 64, blob.data() + off, sizeof(float) * 64);   // the PReLU behind this conv
            off += 64;
        }
        const size_t wb = conv_wpack_bytes(cin, 64);
        tmp.resize(wb);
        pack_conv_weights(pw, cin, 64, 1, tmp.data(), false);
        HIPCHK(h, dev_malloc(&cw.d_wpack, wb));
        HIPCHK(h, copy_blocking(h, cw.d_wpack, tmp.data(), wb, hipMemcpyHostToDevice));
        cw.d_bias = h->pool_b + (size_t)idx * 128;
        cw.d_slope = h->pool_b + (size_t)idx * 128 + 64;
        h->convs.push_back(cw);
    }
    HIPCHK(h, copy_blocking(h, h->pool_b, pb.data(), pb.size() * sizeof(float), hipMemcpyHostToDevice));
    h->has_weights = true;
    return S2SR_OK;
}

static int load_weights_locked(s2sr_handle* h, const float* d_blob, size_t n_floats, hipStream_t st) {
    if (h->compact()) return load_weights_compact(h, d_blob, n_floats, st);
    const std::vector<ConvSpec> specs = conv_specs(h->cfg.num_block, h->cfg.scale);
    const size_t want = s2sr_expected_blob_floats_scale(h->cfg.num_block, h->cfg.scale);
    if (n_floats != want) {
        char b[160];
        snprintf(b, sizeof b, "weight blob has %zu floats, a %d-block scale-%d net needs %zu", n_floats, h->cfg.num_block, h->cfg.scale, want);
        return fail(h, S2SR_E_BADBLOB, b);
    }
    HIPCHK(h, dev_sync());
    drop_graphs(h);
    free_weights(h);
    h->has_weights = false;
    h->fp8_x_exp = h->fp8_x_exp0; h->fp8_g_exp = h->fp8_g_exp0;     // exponents calibrated for the previous weights do not carry over
    const bool fp8 = h->cfg.precision == S2SR_PREC_FP8;
    const bool hp = h->cfg.precision == S2SR_PREC_F16_HP || (fp8 && h->fp8_hp_tail);
    const size_t nconv = specs.size();
    // ---- plan: blob offsets, pooled sizes
    std::vector<uint64_t> woff(nconv), boff(nconv), poff(nconv, 0);
    std::vector<int32_t> couts(nconv);
    size_t off = 0, pool_bytes = 0;
    for (size_t i = 0; i < nconv; ++i) {
        woff[i] = off; off += (size_t)specs[i].cin * specs[i].cout * 9;
        boff[i] = off; off += specs[i].cout;
        couts[i] = specs[i].cout;
        const bool trunk = i >= 1 && i + 5 < nconv;
        if (trunk) {
            poff[i] = pool_bytes;
            pool_bytes += align256(fp8 ? conv_wpack_bytes_f8(specs[i].cin, specs[i].cout) : conv_wpack_bytes(specs[i].cin, specs[i].cout));
        }
    }
    HIPCHK(h, dev_malloc(&h->pool_w, pool_bytes ? pool_bytes : 256));
    HIPCHK(h, dev_malloc(&h->pool_b, nconv * 64 * sizeof(float)));
    if (fp8) HIPCHK(h, dev_malloc(&h->pool_s, nconv * 64 * sizeof(int32_t)));
    {   // biases: one gather kernel
        uint64_t* d_off = nullptr;
        int32_t* d_cout = nullptr;
        HIPCHK(h, dev_malloc(&d_off, nconv * 8));
        HIPCHK(h, dev_malloc(&d_cout, nconv * 4));
        HIPCHK(h, hipMemcpyAsync(d_off, boff.data(), nconv * 8, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(d_cout, couts.data(), nconv * 4, hipMemcpyHostToDevice, st));
        HIPCHK(h, launch_gather_bias(d_blob, d_off, d_cout, (int)nconv, h->pool_b, st));
        HIPCHK(h, hipStreamSynchronize(st));
        dev_free(d_off); dev_free(d_cout);
    }
    std::vector<char> tmp;
    std::vector<float> hw;
    for (size_t idx = 0; idx < nconv; ++idx) {
        const ConvSpec& s = specs[idx];
        ConvW cw;
        const int nb = (s.cin + 15) / 16;
        // split-operand convs: the six outside the RRDB trunk (conv_first, conv_body, up1, up2, hr, last)
        const bool split = hp && (idx == 0 || idx + 5 >= nconv);
        // conv_first's inputs are exact integers: no x_lo.  conv_last has 29 idle output channels: w_lo
        // rides in couts 8..10 of both segments (x_hi, x_lo), one pass over x_hi less
        // All the others (cin 64): x_hi*w_hi on the fp16 MFMA, x_lo*w_hi + x_hi*w_lo as e4m3 planes on the
        // block-scaled fp8 MFMA (twice the rate, half the bytes; 2^-15-relative error on 2^-11-sized terms).
        const bool f8 = split && idx != 0 && s.cin == 64;
        // conv_last (3 couts of 32): w_lo rides in the idle couts 8..10 of the fp16 stages, so only the x_lo planes come in
        // as e4m3 -- 6 stages instead of 8, 192 instead of 256 B per pixel read (S2SR_LAST_FOLD=0: the 8-stage form)
        const bool last_fold = f8 && idx + 1 == nconv && s.cout <= 8 && h->last_fold;
        const bool fold = (split && !f8 && idx + 1 == nconv && s.cout <= 8) || last_fold;
        const int nseg = !split ? 1 : ((idx == 0 || fold || f8) ? 2 : 3);
        cw.cin = s.cin; cw.cout = s.cout; cw.ct = (s.cout + 31) / 32;
        cw.seg_len = nb; cw.nstage = nseg * nb; cw.seg_lo_mask = (nseg == 3 || fold || f8) ? 0x2 : 0x0;
        if (last_fold) cw.nstage = nb + 2;
        cw.f8 = f8;
        cw.fold = fold;
        cw.d_bias = h->pool_b + idx * 64;
        const bool trunk = idx >= 1 && idx + 5 < nconv;     // the 345 RDB convs
        if (trunk) {
            cw.pooled = true;
            cw.d_wpack = h->pool_w + poff[idx];
            if (fp8) {
                cw.f8trunk = true;
                cw.seg_len = (s.cin + 31) / 32;
                cw.nstage = (cw.seg_len + 1) & ~1;
                cw.seg_lo_mask = 0;
                cw.d_wscale = h->pool_s + idx * 64;
                HIPCHK(h, launch_pack_trunk_f8(d_blob + woff[idx], s.cin, s.cout, cw.d_wpack, cw.d_wscale, st));
            } else {
                HIPCHK(h, launch_pack_trunk_f16(d_blob + woff[idx], s.cin, s.cout, cw.d_wpack, st));
            }
        } else {
            // head / tail conv: its weights come to the host for the split-operand / sub-pixel packers
            hw.resize((size_t)s.cin * s.cout * 9);
            HIPCHK(h, hipMemcpyAsync(hw.data(), d_blob + woff[idx], hw.size() * sizeof(float), hipMemcpyDeviceToHost, st));
            HIPCHK(h, hipStreamSynchronize(st));
            const float* pw = hw.data();
            const size_t wb = last_fold ? (size_t)cw.nstage * 9 * cw.ct * 1024 : conv_wpack_bytes_seg(s.cin, s.cout, nseg);
            tmp.resize(wb);
            if (f8) pack_conv_weights_f8hp(pw, s.cin, s.cout, tmp.data(), last_fold);
            else pack_conv_weights(pw, s.cin, s.cout, nseg, tmp.data(), fold);
            if (s.cin == 64 && s.cout == 64 && (idx + 4 == nconv || idx + 3 == nconv)) {   // conv_up1, conv_up2: sub-pixel form
                const size_t pb = conv_wpack_bytes_phase(s.cin, s.cout);
                std::vector<char> ph(pb);
                for (int k = 0; k < 2; ++k) {
                    pack_conv_weights_phase_f8hp(pw, s.cin, s.cout, k, ph.data());
                    HIPCHK(h, dev_malloc(&cw.d_wphase[k], pb));
                    HIPCHK(h, copy_blocking(h, cw.d_wphase[k], ph.data(), pb, hipMemcpyHostToDevice));
                }
            }
            HIPCHK(h, dev_malloc(&cw.d_wpack, wb));
            HIPCHK(h, copy_blocking(h, cw.d_wpack, tmp.data(), wb, hipMemcpyHostToDevice));
        }
        h->convs.push_back(cw);
    }
    HIPCHK(h, hipStreamSynchronize(st));
    h->has_weights = true;
    return S2SR_OK;
}

int s2sr_load_weights(s2sr_handle* h, const float* blob, size_t n_floats) {
    if (!h || !blob) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n_floats != handle_blob_floats(h)) return load_weights_locked(h, nullptr, n_floats, h->stream);   // -> BADBLOB text
    float* d_blob = nullptr;
    HIPCHK(h, dev_malloc(&d_blob, n_floats * sizeof(float)));
    hipError_t e = hipMemcpyAsync(d_blob, blob, n_floats * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        dev_free(d_blob);
        return fail(h, S2SR_E_HIP, std::string("upload of the weight blob failed: ") + hipGetErrorString(e));
    }
    const int rc = load_weights_locked(h, d_blob, n_floats, h->stream);
    dev_free(d_blob);
    return rc;
}

// Device-resident blob (what an RCCL broadcast leaves on every rank): repacked on the device; only the six head/tail convs'
// weights (0.9 MB) visit the host.  `stream` = the stream the blob was produced on (NULL = default stream).
int s2sr_load_weights_dev(s2sr_handle* h, const void* d_blob, size_t n_floats, void* stream) {
    if (!h || !d_blob) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    return load_weights_locked(h, (const float*)d_blob, n_floats, h->stream);
}

int s2sr_plan_tiles(int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t scale, s2sr_window* out, int32_t cap,
                    int32_t* n) {
    if (H <= 0 || W <= 0 || tile <= 0 || pad < 0 || scale <= 0 || !n) return S2SR_E_INVALID;
    const int nx = (W + tile - 1) / tile, ny = (H + tile - 1) / tile;
    *n = nx * ny;
    if (!out) return S2SR_OK;
    if (cap < nx * ny) return S2SR_E_CAPACITY;
    const int win = tile + 2 * pad, op = pad * scale;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            s2sr_window& w = out[y * nx + x];
            // far edge first, then pull the near edge in so the window keeps its full extent
            w.x2 = (x * tile + win < W) ? x * tile + win : W;
            w.y2 = (y * tile + win < H) ? y * tile + win : H;
            w.x1 = (w.x2 - win > 0) ? w.x2 - win : 0;
            w.y1 = (w.y2 - win > 0) ? w.y2 - win : 0;
            // the halo is dropped on every side that has a neighbouring tile INDEX
            w.crop_left = x > 0 ? op : 0;
            w.crop_top = y > 0 ? op : 0;
            w.crop_right = x < nx - 1 ? op : 0;
            w.crop_bottom = y < ny - 1 ? op : 0;
            w.ox1 = w.x1 * scale + w.crop_left;
            w.oy1 = w.y1 * scale + w.crop_top;
            w.ox2 = w.x2 * scale - w.crop_right;
            w.oy2 = w.y2 * scale - w.crop_bottom;
        }
    return S2SR_OK;
}

int s2sr_forward_batch_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t B, int32_t th, int32_t tw, void* d_out,
                              void* stream) {
    if (!h || !d_tiles || !d_out) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;   // NULL = the default stream, as everywhere in HIP
    return forward_dev(h, st, (const uint8_t*)d_tiles, nullptr, B, th, tw, (uint8_t*)d_out, nullptr);
}

// A PART of a larger job of `job_windows` equal windows (a chunk of an AOI's windows on one rank, s2sr/dist.py): the window
// mosaic and the workspace are planned for the whole job, so every part runs in the same planes and replays its graphs.
int s2sr_forward_part_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t B, int32_t th, int32_t tw, int32_t job_windows, void* d_out,
                             void* stream) {
    if (!h || !d_tiles || !d_out || job_windows < B) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const Mosaic mo = pick_mosaic(h, job_windows, th, tw);
    return forward_dev(h, (hipStream_t)stream, (const uint8_t*)d_tiles, nullptr, B, th, tw, (uint8_t*)d_out, nullptr, mo.on() ? &mo : nullptr);
}

// Device -> caller's host buffer, `bytes` from `src`, ordered behind everything already on the copy stream; returns when the
// bytes are in `dst`.  The caller's buffer is ordinary pageable memory (a numpy array): handed to hipMemcpyAsync directly, the
// runtime moves it with copy KERNELS through its own staging at ~6 GB/s, and those kernels take CUs from the persistent conv
// workgroups of the chunk computing meanwhile (4096 x 4096 AOI: +20 ms of compute under 130 ms of copies).  Here: two pinned
// 32-MB slices filled by the DMA engines (pinned destination), emptied by this thread's memcpy while the next slice flies.
static constexpr size_t kStageBytes = 32u << 20;
// `exposed`: nothing computes under this copy (the last band, or the only one): below 128 MB the runtime's own path is then as
// fast or faster (50 MB: 58.1 vs 60.3 ms per 1024 x 1024 call), and there are no conv workgroups for its copy kernels to displace.
static bool is_pinned_host(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // an ordinary malloc'd pointer is "invalid value" to the runtime: not an error of ours
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

static int d2h_staged(s2sr_handle* h, uint8_t* dst, const uint8_t* src, size_t bytes, bool exposed) {
    if (is_pinned_host(dst)) {   // s2sr_host_alloc'd (or registered) destination: one DMA, nothing for this thread to copy
        HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->copy_stream));
        HIPCHK(h, hipStreamSynchronize(h->copy_stream));
        return S2SR_OK;
    }
    if (!h->d2h_staged_on || bytes < (exposed ? (128u << 20) : (24u << 20))) {
        HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->copy_stream));
        HIPCHK(h, hipStreamSynchronize(h->copy_stream));
        return S2SR_OK;
    }
    for (int i = 0; i < 2; ++i) {
        if (!h->stage_buf[i]) HIPCHK(h, host_malloc(&h->stage_buf[i], kStageBytes, hipHostMallocDefault));
        if (!h->stage_ev[i]) HIPCHK(h, hipEventCreateWithFlags(&h->stage_ev[i], hipEventDisableTiming));
    }
    const size_t nsl = (bytes + kStageBytes - 1) / kStageBytes;
    auto len = [&](size_t k) { return k + 1 < nsl ? kStageBytes : bytes - k * kStageBytes; };
    for (size_t k = 0; k < nsl + 2; ++k) {
        const int i = (int)(k & 1);
        if (k >= 2) {   // slice k-2 sits in buffer i
            HIPCHK(h, hipEventSynchronize(h->stage_ev[i]));
            memcpy(dst + (k - 2) * kStageBytes, h->stage_buf[i], len(k - 2));
        }
        if (k < nsl) {
            HIPCHK(h, hipMemcpyAsync(h->stage_buf[i], src + k * kStageBytes, len(k), hipMemcpyDeviceToHost, h->copy_stream));
            HIPCHK(h, hipEventRecord(h->stage_ev[i], h->copy_stream));
        }
    }
    return S2SR_OK;
}

int s2sr_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return S2SR_E_INVALID;
    *out = nullptr;
    if (host_malloc(out, bytes, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return S2SR_E_HIP;
    }
    return S2SR_OK;
}

int s2sr_host_free(void* p) {
    if (!p) return S2SR_OK;
    if (host_free(p) != hipSuccess) {
        (void)hipGetLastError();
        return S2SR_E_HIP;
    }
    return S2SR_OK;
}

static int forward_batch_u8_once(s2sr_handle* h, const uint8_t* tiles, int32_t B, int32_t th, int32_t tw, uint8_t* out) {
    if (!h || !tiles || !out) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int S = h->cfg.scale, u = h->unshuffle();
    const size_t ib = (size_t)B * th * tw * 3, ob = ib * S * S;
    int rc = ensure_scratch(h, 0, ib);
    if (rc) return rc;
    rc = ensure_scratch(h, 1, ob);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_scratch[0], tiles, ib, hipMemcpyHostToDevice, h->stream));
    // Groups are enqueued one by one with an event after each; the device-to-host copy of group g
    // runs on the copy stream while group g+1 computes, so only the last group's copy is exposed.
    // one mosaic plan for the whole batch (ragged tiles): every group runs in the same workspace geometry
    const Mosaic mo = pick_mosaic(h, B, th, tw);
    const int per = mo.on() ? mo.kx * mo.ky : 1;
    const int G = (mo.on() ? group_size(h, (B + per - 1) / per, mo.ky * (mo.wh + 1) - 1, mo.kx * (mo.ww + 1) - 1) : group_size(h, B, th / u, tw / u)) * per;
    const size_t tin = (size_t)th * tw * 3, tout = tin * S * S;
    const int ngroups = (B + G - 1) / G;
    while ((int)h->group_done.size() < ngroups) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->group_done.push_back(e);
    }
    for (int g = 0; g < ngroups; ++g) {
        const int g0 = g * G, n = (B - g0 < G) ? (B - g0) : G;
        rc = forward_dev(h, h->stream, (const uint8_t*)h->d_scratch[0] + g0 * tin, nullptr, n, th, tw,
                         (uint8_t*)h->d_scratch[1] + g0 * tout, nullptr, mo.on() ? &mo : nullptr);
        if (rc) return rc;
        HIPCHK(h, hipEventRecord(h->group_done[g], h->stream));
    }
    for (int g = 0; g < ngroups; ++g) {
        const int g0 = g * G, n = (B - g0 < G) ? (B - g0) : G;
        HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->group_done[g], 0));
        if ((rc = d2h_staged(h, out + g0 * tout, (const uint8_t*)h->d_scratch[1] + g0 * tout, n * tout, g + 1 == ngroups))) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return S2SR_OK;
}

int s2sr_forward_batch_u8(s2sr_handle* h, const uint8_t* tiles, int32_t B, int32_t th, int32_t tw, uint8_t* out) {
    RUN_WITH_STREAM_RECOVERY(h, forward_batch_u8_once(h, tiles, B, th, tw, out));
}

static int forward_f32_once(s2sr_handle* h, const float* x, int32_t N, int32_t H, int32_t W, float* y) {
    if (!h || !x || !y) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t ib = (size_t)N * 3 * H * W * 4, ob = ib * h->cfg.scale * h->cfg.scale;
    int rc = ensure_scratch(h, 0, ib);
    if (rc) return rc;
    rc = ensure_scratch(h, 1, ob);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_scratch[0], x, ib, hipMemcpyHostToDevice, h->stream));
    rc = forward_dev(h, h->stream, nullptr, (const float*)h->d_scratch[0], N, H, W, nullptr, (float*)h->d_scratch[1]);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(y, h->d_scratch[1], ob, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return S2SR_OK;
}

int s2sr_forward_f32(s2sr_handle* h, const float* x, int32_t N, int32_t H, int32_t W, float* y) {
    RUN_WITH_STREAM_RECOVERY(h, forward_f32_once(h, x, N, H, W, y));
}

// host-side maps of the paste rule; shared by enhance and the multi-GPU stitch
static void build_stitch_maps(const std::vector<s2sr_window>& wins, int nx, int ny, int OH, int OW,
                              std::vector<int32_t>& rm, std::vector<int32_t>& cm) {
    rm.assign(2 * (size_t)OH, -1);
    cm.assign(2 * (size_t)OW, -1);
    // last window in loop order wins (:278): ascending index, later entries overwrite the map
    for (int y = 0; y < ny; ++y) {
        const s2sr_window& w = wins[(size_t)y * nx];
        for (int oy = w.oy1; oy < w.oy2; ++oy) { rm[2 * oy] = y; rm[2 * oy + 1] = oy - w.oy1 + w.crop_top; }
    }
    for (int x = 0; x < nx; ++x) {
        const s2sr_window& w = wins[x];
        for (int ox = w.ox1; ox < w.ox2; ++ox) { cm[2 * ox] = x; cm[2 * ox + 1] = ox - w.ox1 + w.crop_left; }
    }
}

// RealESRGAN.enhance (cnn_super_resolution.py:217-234) incl. _tile_process (:236-280)
// Chunk sizes of a tiled enhance(), front to back, in row units (pure host arithmetic; s2sr_debug_plan_chunks exposes it to the
// CPU tests).  `unit_windows` windows per row unit, `per` windows per launch image (a mosaic; 1 without), `pimg` 32 x 32 patches per
// launch image, `ncu` persistent workgroups.  The tail (last, middle) is searched for the fewest trunk-conv rounds plus the
// exposed copy of the last band; what is left goes in front in pieces of at most u_max units.
static void plan_chunk_sizes(int units, int u_max, long unit_windows, int per, long pimg, int ncu, std::vector<int>& sizes) {
    sizes.clear();
    if (units <= 0) return;
    if (u_max < 1) u_max = 1;
    if (per < 1) per = 1;
    if (ncu < 1) ncu = 1;
    auto rounds = [&](int u) -> double {                                        // trunk-conv rounds of a chunk of u units
        const long imgs = ((long)u * unit_windows + per - 1) / per;
        return (double)((imgs * pimg + ncu - 1) / ncu);
    };
    const double copy_per_unit = (double)unit_windows * pimg / per / ncu / 6.0;  // exposed copy of one unit, in rounds
    int best_last = 1, best_mid = 0;
    double best = 1e300;
    for (int last = 1; last <= 3 && last <= units; ++last)
        for (int mid = 0; mid <= 12 && last + mid <= units; ++mid) {
            if (mid > u_max || last > u_max || mid > 5 * last) continue;         // a band's copy must fit under the next chunk's compute (~6x)
            const int front = units - last - mid;
            if (front > 0 && mid == 0 && front > 5 * last) continue;            // a big chunk straight in front of the last one
            if (front > 0 && mid > 0 && front > 6 * mid && front <= u_max) continue;
            double c = rounds(last) + (mid ? rounds(mid) : 0.0) + last * copy_per_unit;
            for (int left = front; left > 0;) { const int u = left < u_max ? left : u_max; c += rounds(u); left -= u; }
            if (c < best - 1e-9) { best = c; best_last = last; best_mid = mid; }
        }
    for (int left = units - best_last - best_mid; left > 0;) { const int u = left < u_max ? left : u_max; sizes.push_back(u); left -= u; }
    if (best_mid) sizes.push_back(best_mid);
    sizes.push_back(best_last);
}

int s2sr_debug_pick_mosaic(int32_t B, int32_t th, int32_t tw, int32_t* kx, int32_t* ky) {
    if (!kx || !ky || B < 0 || th <= 0 || tw <= 0) return S2SR_E_INVALID;
    const Mosaic m = pick_mosaic_cfg(true, B, th, tw);
    *kx = m.on() ? m.kx : 1; *ky = m.on() ? m.ky : 1;
    return S2SR_OK;
}

int s2sr_debug_mosaic_patches(int32_t B, int32_t th, int32_t tw, int64_t* launched, int64_t* plain) {
    if (!launched || !plain || B <= 0 || th <= 0 || tw <= 0) return S2SR_E_INVALID;
    const Mosaic m = pick_mosaic_cfg(true, B, th, tw);
    *plain = (int64_t)B * (roundup32(th) / 32) * (roundup32(tw) / 32);
    *launched = m.on() ? (int64_t)mosaic_patches(B, th, tw, m.kx, m.ky) : *plain;
    return S2SR_OK;
}

int s2sr_debug_plan_chunks(int32_t units, int32_t u_max, int32_t unit_windows, int32_t per, int32_t pimg, int32_t ncu, int32_t* sizes,
                           int32_t cap, int32_t* n) {
    if (!n || units < 0 || cap < 0 || (cap > 0 && !sizes)) return S2SR_E_INVALID;
    std::vector<int> v;
    plan_chunk_sizes(units, u_max, unit_windows, per, pimg, ncu, v);
    *n = (int32_t)v.size();
    if ((int)v.size() > cap) return cap == 0 ? S2SR_OK : S2SR_E_CAPACITY;
    for (size_t i = 0; i < v.size(); ++i) sizes[i] = v[i];
    return S2SR_OK;
}

static int postprocess_dev_locked(s2sr_handle* h, const void* d_rgb, int32_t B, int32_t H, int32_t W, const s2sr_pp_params* prm,
                                  void* d_out, hipStream_t st);
static int pp_band_begin_locked(s2sr_handle* h, int H, int W, const s2sr_pp_params* prm, int order, hipStream_t st);
static int pp_band_hist_locked(s2sr_handle* h, const void* d_img, int y0, int y1, hipStream_t st);
static int pp_band_lut_locked(s2sr_handle* h, hipStream_t st);
static int pp_band_rows_locked(s2sr_handle* h, const void* d_img, int y0, int y1, void* d_out, hipStream_t st);

// The image a tile plan is made for.  Scale 2: H x W reflect-padded by one row / column at the bottom / right to even sizes
// (RealESRGANer's mod-2 rule; the pad is read by index, see pack.hip), and an even tile, so that every window of the padded image
// has even origin and extent.
static int plan_dims(s2sr_handle* h, int H, int W, int tile, int* PH, int* PW) {
    *PH = H; *PW = W;
    if (h->unshuffle() == 1) return S2SR_OK;
    if (H < 2 || W < 2) return fail(h, S2SR_E_INVALID, "scale 2 needs an image of at least 2 x 2 (the mod-2 reflect pad)");
    if (tile % 2) return fail(h, S2SR_E_INVALID, "scale 2 needs an even tile: every window of the padded image must have even origin and size");
    *PH = H + (H & 1); *PW = W + (W & 1);
    return S2SR_OK;
}

// job_rgb: the caller's image is RGB and wants RGB back -- R and B are swapped on the device in front of and behind the net (the
// reference's cvtColor pair, wow_sr.py:85,103).  prm: the crop-visibility post-process (wow_sr.py:187-209) on the stitched RGB
// image, on the device, before the one copy out (it is image-global: no band leaves before the whole mosaic is done).
static int enhance_impl(s2sr_handle* h, const uint8_t* img, int H, int W, int tile, int pad, uint8_t* out_u8,
                        float* out_f32, bool force_tiled = false, bool job_rgb = false, const s2sr_pp_params* prm = nullptr) {
    if (!h || !img || (!out_u8 && !out_f32) || H <= 0 || W <= 0 || tile <= 0 || pad < 0) return S2SR_E_INVALID;
    if ((job_rgb || prm) && !out_u8) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    int rc, PH, PW;
    if ((rc = plan_dims(h, H, W, tile, &PH, &PW))) return rc;
    // scale 2, odd H or W: everything below runs on the padded PH x PW image; the output is cropped to OH x OW by the stitch maps
    const bool reflect = PH != H || PW != W;
    const int scale = h->cfg.scale, u = h->unshuffle(), OH = H * scale, OW = W * scale, OHp = PH * scale, OWp = PW * scale;
    const size_t ib = (size_t)H * W * 3, opx = (size_t)OH * OW * 3;
    if ((rc = ensure_scratch(h, 0, ib))) return rc;
    if ((rc = ensure_scratch(h, 1, opx * (out_f32 ? 4 : 1)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_scratch[0], img, ib, hipMemcpyHostToDevice, st));
    if (job_rgb) HIPCHK(h, launch_swap_rb_u8((const uint8_t*)h->d_scratch[0], (size_t)H * W, (uint8_t*)h->d_scratch[0], st));
    const bool whole_finish = job_rgb || prm != nullptr;      // the image leaves in one piece, behind the device-side finish
    const bool tiled = force_tiled || (long long)PH * PW > (long long)tile * tile * 4;   // strict '>' (:226)
    if (!tiled) {
        if (out_f32 || reflect) {
            // net output is NCHW (f32; enhance() returns HWC) or the padded image's (u8, odd scale-2 image) -> stitch with an
            // identity map, cropped to OH x OW
            const size_t opxp = (size_t)OHp * OWp * 3;
            if ((rc = ensure_scratch(h, 2, opxp * (out_f32 ? 4 : 1)))) return rc;
            rc = forward_dev(h, st, (const uint8_t*)h->d_scratch[0], nullptr, 1, PH, PW, out_f32 ? nullptr : (uint8_t*)h->d_scratch[2],
                             out_f32 ? (float*)h->d_scratch[2] : nullptr, nullptr, H, W);
            if (rc) return rc;
            std::vector<int32_t> rm(2 * OH), cm(2 * OW);
            for (int i = 0; i < OH; ++i) { rm[2 * i] = 0; rm[2 * i + 1] = i; }
            for (int i = 0; i < OW; ++i) { cm[2 * i] = 0; cm[2 * i + 1] = i; }
            if ((rc = ensure_scratch(h, 3, (rm.size() + cm.size()) * 4))) return rc;
            int32_t* d_rm = (int32_t*)h->d_scratch[3];
            int32_t* d_cm = d_rm + rm.size();
            HIPCHK(h, hipMemcpyAsync(d_rm, rm.data(), rm.size() * 4, hipMemcpyHostToDevice, st));
            HIPCHK(h, hipMemcpyAsync(d_cm, cm.data(), cm.size() * 4, hipMemcpyHostToDevice, st));
            HIPCHK(h, hipStreamSynchronize(st));   // rm/cm are stack-owned host buffers
            if (out_f32) HIPCHK(h, launch_stitch_f32((const float*)h->d_scratch[2], 1, OHp, OWp, d_rm, d_cm, OH, OW, (float*)h->d_scratch[1], st));
            else HIPCHK(h, launch_stitch_u8((const uint8_t*)h->d_scratch[2], 1, OHp, OWp, d_rm, d_cm, OH, OW, (uint8_t*)h->d_scratch[1], st));
        } else {
            rc = forward_dev(h, st, (const uint8_t*)h->d_scratch[0], nullptr, 1, H, W, (uint8_t*)h->d_scratch[1], nullptr);
            if (rc) return rc;
        }
    } else {
        int T = 0;
        s2sr_plan_tiles(PH, PW, tile, pad, scale, nullptr, 0, &T);
        std::vector<s2sr_window> wins(T);
        s2sr_plan_tiles(PH, PW, tile, pad, scale, wins.data(), T, &T);
        const int pnx = (PW + tile - 1) / tile, pny = (PH + tile - 1) / tile;    // the reference's plan
        const int wh = wins[0].y2 - wins[0].y1, ww = wins[0].x2 - wins[0].x1;   // all windows share one shape
        std::vector<int32_t> rm, cm;
        build_stitch_maps(wins, pnx, pny, OHp, OWp, rm, cm);                    // (the stitches read the first OH x OW of them)
        // When a dimension ends within 2*pad of a tile multiple, the last two window rows (columns)
        // of the plan are the same rectangle: the reference runs the net on both (only the paste
        // ranges differ).  Identical inputs give identical outputs, so each distinct rectangle is
        // forwarded once and the paste maps point at it.
        std::vector<int> uy(pny), ux(pnx), rows_y1, cols_x1;
        for (int y = 0; y < pny; ++y) {
            const int y1 = wins[(size_t)y * pnx].y1;
            if (rows_y1.empty() || rows_y1.back() != y1) rows_y1.push_back(y1);
            uy[y] = (int)rows_y1.size() - 1;
        }
        for (int x = 0; x < pnx; ++x) {
            const int x1 = wins[x].x1;
            if (cols_x1.empty() || cols_x1.back() != x1) cols_x1.push_back(x1);
            ux[x] = (int)cols_x1.size() - 1;
        }
        for (size_t i = 0; i < rm.size(); i += 2)
            if (rm[i] >= 0) rm[i] = uy[rm[i]];
        for (size_t i = 0; i < cm.size(); i += 2)
            if (cm[i] >= 0) cm[i] = ux[cm[i]];
        const int nx = (int)cols_x1.size(), ny = (int)rows_y1.size();
        T = nx * ny;
        std::vector<int32_t> rects(4 * (size_t)T);
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int t = y * nx + x;
                rects[4 * t] = rows_y1[y]; rects[4 * t + 1] = rows_y1[y] + wh; rects[4 * t + 2] = cols_x1[x]; rects[4 * t + 3] = cols_x1[x] + ww;
            }
        const size_t tin = (size_t)T * wh * ww * 3, tout = tin * scale * scale;
        if ((rc = ensure_scratch(h, 2, tin))) return rc;
        if ((rc = ensure_scratch(h, 4, tout * (out_f32 ? 4 : 1)))) return rc;
        if ((rc = ensure_scratch(h, 3, (rects.size() + rm.size() + cm.size()) * 4))) return rc;
        int32_t* d_rects = (int32_t*)h->d_scratch[3];
        int32_t* d_rm = d_rects + rects.size();
        int32_t* d_cm = d_rm + rm.size();
        HIPCHK(h, hipMemcpyAsync(d_rects, rects.data(), rects.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(d_rm, rm.data(), rm.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(d_cm, cm.data(), cm.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipStreamSynchronize(st));
        if (reflect) HIPCHK(h, launch_gather_windows_reflect((const uint8_t*)h->d_scratch[0], H, W, d_rects, T, wh, ww, (uint8_t*)h->d_scratch[2], st));
        else HIPCHK(h, launch_gather_windows((const uint8_t*)h->d_scratch[0], H, W, d_rects, T, wh, ww, (uint8_t*)h->d_scratch[2], st));
        // Chunks of whole window rows.  An output row is final once the last window row that pastes into it is done (the row
        // map is monotone), so each chunk is followed by the stitch of its band of final rows, and the band's device-to-host
        // copy runs on the copy stream under the next chunk's compute.  A chunk holds whole launch groups: for windows that
        // travel as mosaics (forward_dev) rows in multiples of what fills a mosaic, and as many mosaics as the workspace
        // allows -- the patch count of a launch must be large against the 256 workgroups (one 4 x 4 mosaic of 276-pixel
        // windows is 1225 patches = 4.8 per CU, five rounds for 4.8 rounds of work; five mosaics are 23.9 -> 24).
        // Chunk sizes.  The device-to-host copy of a chunk's band hides under the NEXT chunk's compute and only the last band's
        // copy is exposed, so chunks shrink towards the end (a row of 276-pixel windows computes ~6x longer than its 13 MB band
        // takes to reach pageable host memory; a chunk may be up to 5x its successor).  What a small chunk costs is the rounding
        // of its patch count to whole rounds of the persistent workgroups in the trunk convs (32 x 32 patches; a 4 x 4 mosaic
        // of 276-pixel windows = 1225 patches = 4.8 rounds of 256: 1, 2, 3, 4 mosaics lose 4.3 %, 5 or 10 lose 0.3 %).  The
        // tail (last, middle) is searched over small sizes for the fewest rounds + exposed copy; the rest goes in front in
        // workspace-sized pieces.  4096 x 4096 at 256/10: 16 rows of 16 windows -> 10 + 5 + 1.
        std::vector<int> chunk_r0;   // first window row of each chunk, plus ny at the end
        const Mosaic mo = pick_mosaic(h, T, wh, ww);   // ONE plan for the job: every chunk runs in its workspace geometry
        {
            const int per = mo.on() ? mo.kx * mo.ky : 1;
            const int gw = (mo.on() ? group_size(h, (T + per - 1) / per, mo.ky * (mo.wh + 1) - 1, mo.kx * (mo.ww + 1) - 1)
                                    : group_size(h, T, wh / u, ww / u)) * per;          // windows per launch group
            const int r_min = (per + nx - 1) / nx;                                      // rows that fill a mosaic
            const int units = (ny + r_min - 1) / r_min;                                 // ... and how many such row units the image has
            int u_max = gw / nx / r_min;                                                // units per chunk the workspace allows
            if (u_max < 1) u_max = 1;
            int ncu = 256;
            (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->cfg.device);
            const long pimg = mo.on() ? (long)((mo.ky * (mo.wh + 1) - 1 + 31) / 32) * ((mo.kx * (mo.ww + 1) - 1 + 31) / 32)
                                      : (long)((wh / u + 31) / 32) * ((ww / u + 31) / 32);   // 32 x 32 patches per launch image
            std::vector<int> sizes;                                                     // in units, front to back
            plan_chunk_sizes(units, u_max, r_min * nx, per, pimg, ncu, sizes);
            int r = 0;
            for (int u : sizes) { chunk_r0.push_back(r); r += u * r_min; }
            chunk_r0.push_back(ny);
        }
        const int nchunks = (int)chunk_r0.size() - 1;
        if (!out_f32 && nchunks > 1) {
            // A job (job_rgb / prm) takes the same route: the channel swap behind the net is applied to every band as it is stitched;
            // the post-process -- image-global through CLAHE's grid (wow_sr.py:191-192) -- counts every band into the histograms as
            // it is stitched (under the compute of the chunks still to come), builds the LUTs behind the last band and then
            // finishes the image in row bands, each followed by its copy out: what is exposed behind the last window is one band's
            // kernels plus the PCIe time of the image (the r04 form waited for the whole mosaic, swapped, post-processed and only
            // then started the one copy).
            const size_t win_in = (size_t)wh * ww * 3, win_out = win_in * scale * scale;
            const size_t row_b = (size_t)OW * 3;
            int fin_rows = 0, nfin = 0;          // finishing bands of the post-process: ~48 MB each, whole 32-row tile rows
            if (prm) {
                fin_rows = (int)(((size_t)48 << 20) / row_b) & ~31;
                if (fin_rows < 64) fin_rows = 64;
                nfin = (OH + fin_rows - 1) / fin_rows;
                if ((rc = pp_band_begin_locked(h, OH, OW, prm, job_rgb ? 3 : 0, st))) return rc;   // (allocates: before anything is enqueued)
            }
            while ((int)h->group_done.size() < nchunks + nfin) {
                hipEvent_t e;
                HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
                h->group_done.push_back(e);
            }
            uint8_t* d_img_out = (uint8_t*)h->d_scratch[1];
            int yb = 0, prev_yb = 0, prev_ye = 0;
            for (int c = 0; c < nchunks; ++c) {
                const int r0 = chunk_r0[c], r1 = chunk_r0[c + 1] < ny ? chunk_r0[c + 1] : ny;
                const int t0 = r0 * nx, n = (r1 - r0) * nx;
                rc = forward_dev(h, st, (const uint8_t*)h->d_scratch[2] + t0 * win_in, nullptr, n, wh, ww,
                                 (uint8_t*)h->d_scratch[4] + t0 * win_out, nullptr, mo.on() ? &mo : nullptr);
                if (rc) return rc;
                int ye = OH;
                if (r1 < ny)
                    for (ye = yb; ye < OH && rm[2 * ye] < r1; ++ye) {}
                if (ye > yb) {
                    HIPCHK(h, launch_stitch_u8((const uint8_t*)h->d_scratch[4], nx, wh * scale, ww * scale, d_rm + 2 * yb, d_cm, ye - yb, OW,
                                               d_img_out + (size_t)yb * row_b, st));
                    if (prm) {
                        if ((rc = pp_band_hist_locked(h, d_img_out, yb, ye, st))) return rc;
                    } else if (job_rgb) {
                        HIPCHK(h, launch_swap_rb_u8(d_img_out + (size_t)yb * row_b, (size_t)(ye - yb) * OW, d_img_out + (size_t)yb * row_b, st));
                    }
                }
                HIPCHK(h, hipEventRecord(h->group_done[c], st));
                if (!prm && c > 0 && prev_ye > prev_yb) {
                    HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->group_done[c - 1], 0));
                    if ((rc = d2h_staged(h, out_u8 + (size_t)prev_yb * row_b, d_img_out + (size_t)prev_yb * row_b,
                                         (size_t)(prev_ye - prev_yb) * row_b, false))) return rc;
                }
                prev_yb = yb; prev_ye = ye; yb = ye;
            }
            if (!prm) {
                if (prev_ye > prev_yb) {
                    HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->group_done[nchunks - 1], 0));
                    if ((rc = d2h_staged(h, out_u8 + (size_t)prev_yb * row_b, d_img_out + (size_t)prev_yb * row_b,
                                         (size_t)(prev_ye - prev_yb) * row_b, true))) return rc;
                }
            } else {
                // LUTs, then every finishing band's kernels (in place: a band's rows are rewritten only after the apply pass, which
                // runs R rows ahead, has read them), an event behind each; the copies follow band by band on the copy stream
                const bool timing = getenv("S2SR_JOB_TIMING") != nullptr;     // diagnostic: stage times of the finish on stderr
                auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
                double t_enq = now(), t_compute = 0, t_first = 0;
                if ((rc = pp_band_lut_locked(h, st))) return rc;
                for (int b = 0; b < nfin; ++b) {
                    const int y0 = b * fin_rows, y1 = y0 + fin_rows < OH ? y0 + fin_rows : OH;
                    if ((rc = pp_band_rows_locked(h, d_img_out, y0, y1, d_img_out, st))) return rc;
                    HIPCHK(h, hipEventRecord(h->group_done[nchunks + b], st));
                }
                if (timing) {
                    HIPCHK(h, hipEventSynchronize(h->group_done[nchunks - 1]));
                    t_compute = now();
                }
                for (int b = 0; b < nfin; ++b) {
                    const int y0 = b * fin_rows, y1 = y0 + fin_rows < OH ? y0 + fin_rows : OH;
                    HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->group_done[nchunks + b], 0));
                    if ((rc = d2h_staged(h, out_u8 + (size_t)y0 * row_b, d_img_out + (size_t)y0 * row_b, (size_t)(y1 - y0) * row_b,
                                         false))) return rc;
                    if (timing && b == 0) t_first = now();
                }
                if (timing)
                    fprintf(stderr, "[s2sr job] finish: %d bands of %d rows; last chunk done %.2f ms after the finish was queued, first band on the host "
                            "+%.2f ms, all bands +%.2f ms\n", nfin, fin_rows, t_compute - t_enq, t_first - t_compute, now() - t_compute);
            }
            HIPCHK(h, hipStreamSynchronize(h->copy_stream));
            HIPCHK(h, hipStreamSynchronize(st));
            return S2SR_OK;
        }
        rc = forward_dev(h, st, (const uint8_t*)h->d_scratch[2], nullptr, T, wh, ww, out_f32 ? nullptr : (uint8_t*)h->d_scratch[4],
                         out_f32 ? (float*)h->d_scratch[4] : nullptr);
        if (rc) return rc;
        if (out_f32) HIPCHK(h, launch_stitch_f32((const float*)h->d_scratch[4], nx, wh * scale, ww * scale, d_rm, d_cm, OH, OW, (float*)h->d_scratch[1], st));
        else HIPCHK(h, launch_stitch_u8((const uint8_t*)h->d_scratch[4], nx, wh * scale, ww * scale, d_rm, d_cm, OH, OW, (uint8_t*)h->d_scratch[1], st));
    }
    const uint8_t* d_final = (const uint8_t*)h->d_scratch[1];
    if (whole_finish) {
        if (job_rgb) HIPCHK(h, launch_swap_rb_u8((const uint8_t*)h->d_scratch[1], (size_t)OH * OW, (uint8_t*)h->d_scratch[1], st));
        if (prm) {
            // the windows' output buffer is free again once the stitch has read it; whole-image jobs get a buffer of their own
            if ((rc = ensure_scratch(h, 4, opx))) return rc;
            if ((rc = postprocess_dev_locked(h, h->d_scratch[1], 1, OH, OW, prm, h->d_scratch[4], st))) return rc;
            d_final = (const uint8_t*)h->d_scratch[4];
        }
    }
    if (h->group_done.empty()) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->group_done.push_back(e);
    }
    HIPCHK(h, hipEventRecord(h->group_done[0], st));
    HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->group_done[0], 0));
    if ((rc = d2h_staged(h, out_f32 ? (uint8_t*)out_f32 : out_u8, out_f32 ? (const uint8_t*)h->d_scratch[1] : d_final, opx * (out_f32 ? 4 : 1), true))) return rc;
    HIPCHK(h, hipStreamSynchronize(st));
    return S2SR_OK;
}

int s2sr_enhance_u8(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, uint8_t* out) {
    RUN_WITH_STREAM_RECOVERY(h, enhance_impl(h, img, H, W, tile, pad, out, nullptr));
}

// A whole /api/wow job's device work in one call (apply_wow_sr, wow_sr.py:85-110): RGB image in, RGB2BGR, RealESRGAN.enhance,
// BGR2RGB, _enhance_for_crops (prm != NULL), RGB image out -- one upload, one download, nothing in between on the host.
int s2sr_enhance_job_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W, int32_t tile, int32_t pad, const s2sr_pp_params* prm,
                        uint8_t* out_rgb) {
    RUN_WITH_STREAM_RECOVERY(h, enhance_impl(h, rgb, H, W, tile, pad, out_rgb, nullptr, false, true, prm));
}

int s2sr_enhance_f32(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, float* out) {
    RUN_WITH_STREAM_RECOVERY(h, enhance_impl(h, img, H, W, tile, pad, nullptr, out));
}

int s2sr_cut_windows_u8_dev(s2sr_handle* h, const void* d_img, int32_t H, int32_t W, int32_t tile, int32_t pad,
                            int32_t first, int32_t count, void* d_tiles, void* stream) {
    if (!h || !d_img || !d_tiles || H <= 0 || W <= 0 || tile <= 0 || pad < 0 || first < 0 || count <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;   // NULL = the default stream, as everywhere in HIP
    int T = 0, PH, PW;
    int rc = plan_dims(h, H, W, tile, &PH, &PW);
    if (rc) return rc;
    s2sr_plan_tiles(PH, PW, tile, pad, h->cfg.scale, nullptr, 0, &T);
    if (first + count > T) return fail(h, S2SR_E_INVALID, "window range exceeds the plan");
    std::vector<s2sr_window> wins(T);
    s2sr_plan_tiles(PH, PW, tile, pad, h->cfg.scale, wins.data(), T, &T);
    const int wh = wins[0].y2 - wins[0].y1, ww = wins[0].x2 - wins[0].x1;
    std::vector<int32_t> rects(4 * (size_t)count);
    for (int t = 0; t < count; ++t) {
        const s2sr_window& w = wins[first + t];
        rects[4 * t] = w.y1; rects[4 * t + 1] = w.y2; rects[4 * t + 2] = w.x1; rects[4 * t + 3] = w.x2;
    }
    rc = ensure_scratch(h, 3, rects.size() * 4);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_scratch[3], rects.data(), rects.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (PH != H || PW != W)
        HIPCHK(h, launch_gather_windows_reflect((const uint8_t*)d_img, H, W, (const int32_t*)h->d_scratch[3], count, wh, ww, (uint8_t*)d_tiles, st));
    else HIPCHK(h, launch_gather_windows((const uint8_t*)d_img, H, W, (const int32_t*)h->d_scratch[3], count, wh, ww, (uint8_t*)d_tiles, st));
    return S2SR_OK;
}

int s2sr_stitch_rows_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t oy0, int32_t oy1,
                            void* d_out, void* stream) {
    if (!h || !d_tiles || !d_out || H <= 0 || W <= 0 || tile <= 0 || pad < 0 || oy0 < 0 || oy1 > h->cfg.scale * H || oy0 > oy1) return S2SR_E_INVALID;
    if (oy0 == oy1) return S2SR_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;   // NULL = the default stream, as everywhere in HIP
    const int S = h->cfg.scale;
    int T = 0, PH, PW;
    int rc = plan_dims(h, H, W, tile, &PH, &PW);
    if (rc) return rc;
    s2sr_plan_tiles(PH, PW, tile, pad, S, nullptr, 0, &T);
    std::vector<s2sr_window> wins(T);
    s2sr_plan_tiles(PH, PW, tile, pad, S, wins.data(), T, &T);
    const int nx = (PW + tile - 1) / tile, ny = (PH + tile - 1) / tile;
    const int wh = wins[0].y2 - wins[0].y1, ww = wins[0].x2 - wins[0].x1;
    const size_t nrm = 2 * (size_t)(S * PH), ncm = 2 * (size_t)(S * PW);   // maps of the padded image; the stitch reads S H x S W
    // the plan's paste maps: from the handle's LRU of map sets, or built and uploaded now.  A NEW set costs an allocation and a
    // blocking upload on the handle's own stream -- nothing the caller has queued on ITS stream is waited for (r04: any key change
    // synchronised the device under the process-wide gate, so the first band's stitch drained every compute chunk already queued
    // and stalled the captures of other handles).  Only when all four sets are taken is the least recently used one recycled, and
    // only then is the device synchronised: a stitch that still reads it may be in flight on a stream this library does not know.
    const int key[4] = {H, W, tile, pad + 1};
    s2sr_handle::StitchMaps* ms = nullptr;
    for (auto& m : h->stitch_sets)
        if (m.d && m.key[0] == key[0] && m.key[1] == key[1] && m.key[2] == key[2] && m.key[3] == key[3]) ms = &m;
    if (!ms) {
        for (auto& m : h->stitch_sets)
            if (!m.d) { ms = &m; break; }
        if (!ms) {
            ms = &h->stitch_sets[0];
            for (auto& m : h->stitch_sets)
                if (m.last_use < ms->last_use) ms = &m;
            HIPCHK(h, dev_sync());
            if (ms->cap < (nrm + ncm) * 4) {
                HIPCHK(h, dev_free(ms->d));
                ms->d = nullptr; ms->cap = 0;
            }
        }
        ms->key[0] = 0;                       // (invalid until the upload is through)
        if (!ms->d) {
            HIPCHK(h, dev_malloc(&ms->d, (nrm + ncm) * 4));
            ms->cap = (nrm + ncm) * 4;
        }
        std::vector<int32_t> rm, cm;
        build_stitch_maps(wins, nx, ny, S * PH, S * PW, rm, cm);
        HIPCHK(h, copy_blocking(h, ms->d, rm.data(), nrm * 4, hipMemcpyHostToDevice));
        HIPCHK(h, copy_blocking(h, ms->d + nrm, cm.data(), ncm * 4, hipMemcpyHostToDevice));
        for (int i = 0; i < 4; ++i) ms->key[i] = key[i];
    }
    ms->last_use = ++h->stitch_clock;
    const int32_t* d_rm = ms->d;
    const int32_t* d_cm = d_rm + nrm;
    HIPCHK(h, launch_stitch_u8((const uint8_t*)d_tiles, nx, wh * S, ww * S, d_rm + 2 * (size_t)oy0, d_cm, oy1 - oy0, S * W,
                               (uint8_t*)d_out + (size_t)oy0 * S * W * 3, st));
    return S2SR_OK;
}

int s2sr_stitch_windows_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t H, int32_t W, int32_t tile, int32_t pad,
                               void* d_out, void* stream) {
    if (!h) return S2SR_E_INVALID;
    return s2sr_stitch_rows_u8_dev(h, d_tiles, H, W, tile, pad, 0, h->cfg.scale * H, d_out, stream);
}

// Device -> host for callers that hold device buffers (s2sr/dist.py's consuming rank): `bytes` from d_src into dst once
// everything enqueued on `stream` so far is done; returns when the bytes are in dst.  A destination from s2sr_host_alloc is
// filled by one DMA, a pageable one through the pinned staging slices (d2h_staged) -- never the runtime's copy kernels, which
// take CUs from the conv workgroups of whatever computes meanwhile.
int s2sr_copy_to_host(s2sr_handle* h, void* dst, const void* d_src, size_t bytes, void* stream) {
    if (!h || !dst || !d_src) return S2SR_E_INVALID;
    if (bytes == 0) return S2SR_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->host_copy_ev) HIPCHK(h, hipEventCreateWithFlags(&h->host_copy_ev, hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(h->host_copy_ev, (hipStream_t)stream));
    HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->host_copy_ev, 0));
    return d2h_staged(h, (uint8_t*)dst, (const uint8_t*)d_src, bytes, false);
}

int s2sr_tile_process_f32(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, float* out) {
    RUN_WITH_STREAM_RECOVERY(h, enhance_impl(h, img, H, W, tile, pad, nullptr, out, true));
}

// post-process on device buffers; the caller holds h->mu
static int postprocess_dev_locked(s2sr_handle* h, const void* d_rgb, int32_t B, int32_t H, int32_t W, const s2sr_pp_params* prm,
                                  void* d_out, hipStream_t st) {
    const size_t wb = postprocess_work_bytes(B, H, W, *prm);
    int rc = ensure_scratch(h, 5, wb);
    if (rc) return rc;
    Scope sc(h, st, F_POST, 0.0, (double)B * H * W * 9.0);
    HIPCHK(h, launch_postprocess((const uint8_t*)d_rgb, B, H, W, *prm, (uint8_t*)d_out, h->d_scratch[5], wb, st));
    return S2SR_OK;
}

int s2sr_postprocess_batch_u8_dev(s2sr_handle* h, const void* d_rgb, int32_t B, int32_t H, int32_t W,
                                  const s2sr_pp_params* prm, void* d_out, void* stream) {
    if (!h || !d_rgb || !d_out || !prm || B <= 0 || H <= 0 || W <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return postprocess_dev_locked(h, d_rgb, B, H, W, prm, d_out, (hipStream_t)stream);   // NULL = the default stream, as everywhere in HIP
}

// ---- the post-process over one device image in row bands (see postprocess.hip launch_pp_band_*) -------------------------------
// order: S2SR_PP_ORDER_BGR = the image's bytes are B,G,R; S2SR_PP_ORDER_SWAP_OUT = R and B exchanged in the rows written
static int pp_band_begin_locked(s2sr_handle* h, int H, int W, const s2sr_pp_params* prm, int order, hipStream_t st) {
    if (prm->clahe_grid <= 0 || prm->clahe_grid > 64) return fail(h, S2SR_E_INVALID, "clahe_grid must be 1..64");
    int rc = ensure_scratch(h, 5, postprocess_work_bytes(1, H, W, *prm));
    if (rc) return rc;
    s2sr_handle::PPBand& b = h->ppb;
    b = s2sr_handle::PPBand();
    b.H = H; b.W = W; b.prm = *prm;
    b.bgr = (order & S2SR_PP_ORDER_BGR) ? 1 : 0;
    b.swap_out = (order & S2SR_PP_ORDER_SWAP_OUT) ? 1 : 0;
    b.radius = pp_band_radius(*prm);
    HIPCHK(h, launch_pp_band_begin(H, W, *prm, h->d_scratch[5], st));
    b.open = true;
    return S2SR_OK;
}

static int pp_band_hist_locked(s2sr_handle* h, const void* d_img, int y0, int y1, hipStream_t st) {
    s2sr_handle::PPBand& b = h->ppb;
    if (!b.open || b.lut) return fail(h, S2SR_E_INVALID, "pp_band_hist: no banded post-process open, or its LUTs are already built");
    if (y0 < 0 || y1 > b.H || y0 > y1) return fail(h, S2SR_E_INVALID, "pp_band_hist: rows outside the image");
    Scope sc(h, st, F_POST, 0.0, (double)(y1 - y0) * b.W * 3.0);
    HIPCHK(h, launch_pp_band_hist((const uint8_t*)d_img, b.H, b.W, b.prm, b.bgr, y0, y1, h->d_scratch[5], st));
    return S2SR_OK;
}

static int pp_band_lut_locked(s2sr_handle* h, hipStream_t st) {
    s2sr_handle::PPBand& b = h->ppb;
    if (!b.open || b.lut) return fail(h, S2SR_E_INVALID, "pp_band_lut: no banded post-process open, or its LUTs are already built");
    HIPCHK(h, launch_pp_band_lut(b.H, b.W, b.prm, h->d_scratch[5], st));
    b.lut = true;
    return S2SR_OK;
}

static int pp_band_rows_locked(s2sr_handle* h, const void* d_img, int y0, int y1, void* d_out, hipStream_t st) {
    s2sr_handle::PPBand& b = h->ppb;
    if (!b.open || !b.lut) return fail(h, S2SR_E_INVALID, "pp_band_rows: the LUTs are not built (begin, hist over every row, lut, then rows)");
    if (y0 != b.rows_end || y1 <= y0 || y1 > b.H) return fail(h, S2SR_E_INVALID, "pp_band_rows: bands must follow each other from row 0");
    const int need = y1 + b.radius < b.H ? y1 + b.radius : b.H;     // the blur of row y1-1 reads R rows below it
    Scope sc(h, st, F_POST, 0.0, (double)(y1 - y0) * b.W * 6.0);
    if (need > b.applied_end) {
        HIPCHK(h, launch_pp_band_apply((const uint8_t*)d_img, b.H, b.W, b.prm, b.bgr, b.applied_end, need, h->d_scratch[5], st));
        b.applied_end = need;
    }
    HIPCHK(h, launch_pp_band_sharpen(b.H, b.W, b.prm, b.bgr, b.swap_out, y0, y1, h->d_scratch[5], (uint8_t*)d_out, st));
    b.rows_end = y1;
    if (y1 == b.H) b.open = false;
    return S2SR_OK;
}

int s2sr_pp_band_begin_dev(s2sr_handle* h, int32_t H, int32_t W, const s2sr_pp_params* prm, int32_t order, void* stream) {
    if (!h || !prm || H <= 0 || W <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return pp_band_begin_locked(h, H, W, prm, order, (hipStream_t)stream);
}

int s2sr_pp_band_hist_dev(s2sr_handle* h, const void* d_img, int32_t y0, int32_t y1, void* stream) {
    if (!h || !d_img) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return pp_band_hist_locked(h, d_img, y0, y1, (hipStream_t)stream);
}

int s2sr_pp_band_lut_dev(s2sr_handle* h, void* stream) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return pp_band_lut_locked(h, (hipStream_t)stream);
}

int s2sr_pp_band_rows_dev(s2sr_handle* h, const void* d_img, int32_t y0, int32_t y1, void* d_out, void* stream) {
    if (!h || !d_img || !d_out) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return pp_band_rows_locked(h, d_img, y0, y1, d_out, (hipStream_t)stream);
}

// Host image in, host image out.  ONE lock scope from the upload to the download: the staging buffers
// (d_scratch[0], [1]) belong to the handle, and the app shares one post-process handle per device between
// all jobs (app/wow_sr.py), which the reference runs from concurrent worker threads (main.py:247-368).
int s2sr_postprocess_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W, const s2sr_pp_params* prm, uint8_t* out) {
    if (!h || !rgb || !out || !prm || H <= 0 || W <= 0) return S2SR_E_INVALID;
    const size_t nb = (size_t)H * W * 3;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = ensure_scratch(h, 0, nb);
    if (rc) return rc;
    if ((rc = ensure_scratch(h, 1, nb))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_scratch[0], rgb, nb, hipMemcpyHostToDevice, h->stream));
    if ((rc = postprocess_dev_locked(h, h->d_scratch[0], 1, H, W, prm, h->d_scratch[1], h->stream))) return rc;
    HIPCHK(h, hipMemcpyAsync(out, h->d_scratch[1], nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return S2SR_OK;
}

// ---- XYZ tile pyramid (host buffers in and out; geometry tables come from the caller) ---------------
int s2sr_warp_bilinear_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W, const float* grid, int32_t gh, int32_t gw,
                          int32_t step, int32_t OH, int32_t OW, uint8_t* out_rgba) {
    if (!h || !rgb || !grid || !out_rgba || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || gh <= 0 || gw <= 0) return S2SR_E_INVALID;
    if (step <= 0 || (step & (step - 1))) return fail(h, S2SR_E_INVALID, "warp node spacing must be a power of two");
    if ((int64_t)(gh - 1) * step < OH - 1 || (int64_t)(gw - 1) * step < OW - 1)
        return fail(h, S2SR_E_INVALID, "warp node grid does not cover the output raster");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t ib = (size_t)H * W * 3, gb = (size_t)gh * gw * 8, ob = (size_t)OH * OW * 4;
    int rc;
    if ((rc = ensure_scratch(h, 0, ib))) return rc;
    if ((rc = ensure_scratch(h, 1, ob))) return rc;
    if ((rc = ensure_scratch(h, 3, gb))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_scratch[0], rgb, ib, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->d_scratch[3], grid, gb, hipMemcpyHostToDevice, st));
    {
        Scope sc(h, st, F_MISC, 0.0, (double)ob + (double)OH * OW * 12.0);
        HIPCHK(h, launch_warp_bilinear((const uint8_t*)h->d_scratch[0], H, W, (const float*)h->d_scratch[3], gh, gw, step, OH, OW,
                                       (uint8_t*)h->d_scratch[1], st));
    }
    HIPCHK(h, hipMemcpyAsync(out_rgba, h->d_scratch[1], ob, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->warp_slot = 1; h->warp_h = OH; h->warp_w = OW;      // the raster also stays on the device for the base level of its pyramid
    return S2SR_OK;
}

int s2sr_tiles_base_u8(s2sr_handle* h, const uint8_t* rgba, int32_t H, int32_t W, const int32_t* col_lo, const int32_t* col_hi,
                       const int32_t* row_lo, const int32_t* row_hi, int32_t nx, int32_t ny, uint8_t* out) {
    if (!h || !col_lo || !col_hi || !row_lo || !row_hi || H <= 0 || W <= 0 || nx <= 0 || ny <= 0) return S2SR_E_INVALID;
    for (int i = 0; i < nx * 256; ++i)
        if (col_lo[i] < 0 || col_hi[i] >= W) return fail(h, S2SR_E_INVALID, "column footprint table leaves the raster");
    for (int i = 0; i < ny * 256; ++i)
        if (row_lo[i] < 0 || row_hi[i] >= H) return fail(h, S2SR_E_INVALID, "row footprint table leaves the raster");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t ib = (size_t)H * W * 4, ob = (size_t)nx * ny * 65536 * 4, cb = (size_t)nx * 256 * 4, rb = (size_t)ny * 256 * 4;
    // rgba == NULL: the raster is the one the previous call on this handle -- s2sr_warp_bilinear_u8 -- produced, taken from its
    // device copy (a 4096 x 4096 source: 67 MB that would cross PCIe twice between the two calls)
    int in_slot = 0;
    if (!rgba) {
        if (h->warp_slot < 0 || h->warp_h != H || h->warp_w != W)
            return fail(h, S2SR_E_INVALID, "rgba == NULL, but the previous call on this handle did not leave a warped raster of this size on the device");
        in_slot = h->warp_slot;
    }
    const int out_slot = in_slot == 1 ? 0 : 1;
    int rc;
    if (rgba && (rc = ensure_scratch(h, in_slot, ib))) return rc;
    if ((rc = ensure_scratch(h, out_slot, ob))) return rc;
    if ((rc = ensure_scratch(h, 3, 2 * cb + 2 * rb))) return rc;
    int32_t* t = (int32_t*)h->d_scratch[3];
    if (rgba) HIPCHK(h, hipMemcpyAsync(h->d_scratch[in_slot], rgba, ib, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(t, col_lo, cb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(t + nx * 256, col_hi, cb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(t + 2 * nx * 256, row_lo, rb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(t + 2 * nx * 256 + ny * 256, row_hi, rb, hipMemcpyHostToDevice, st));
    {
        Scope sc(h, st, F_MISC, 0.0, (double)ib + (double)ob);
        HIPCHK(h, launch_tiles_base((const uint8_t*)h->d_scratch[in_slot], W, t, t + nx * 256, t + 2 * nx * 256, t + 2 * nx * 256 + ny * 256, nx,
                                    ny, (uint8_t*)h->d_scratch[out_slot], st));
    }
    if (out) HIPCHK(h, hipMemcpyAsync(out, h->d_scratch[out_slot], ob, hipMemcpyDeviceToHost, st));      // out == NULL: the level stays on the device
    HIPCHK(h, hipStreamSynchronize(st));
    h->tiles_slot = out_slot; h->tiles_nx = nx; h->tiles_ny = ny;
    return S2SR_OK;
}

int s2sr_tiles_overview_u8(s2sr_handle* h, const uint8_t* child, int32_t cnx, int32_t cny, int32_t ox, int32_t oy, int32_t pnx,
                           int32_t pny, uint8_t* out) {
    if (!h || cnx <= 0 || cny <= 0 || pnx <= 0 || pny <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t ib = (size_t)cnx * cny * 65536 * 4, ob = (size_t)pnx * pny * 65536 * 4;
    // child == NULL: the children are the level the previous pyramid call on this handle produced, still on the device (a
    // z18 level is 2.9 GB: sending it back costs as much as fetching it did)
    int in_slot = 0;
    if (!child) {
        if (h->tiles_slot < 0 || h->tiles_nx != cnx || h->tiles_ny != cny)
            return fail(h, S2SR_E_INVALID, "child == NULL, but the previous call on this handle did not leave a tile level of this size on the device");
        in_slot = h->tiles_slot;
    }
    const int out_slot = in_slot == 1 ? 0 : 1;
    int rc;
    if (child && (rc = ensure_scratch(h, in_slot, ib))) return rc;
    if ((rc = ensure_scratch(h, out_slot, ob))) return rc;
    if (child) HIPCHK(h, hipMemcpyAsync(h->d_scratch[in_slot], child, ib, hipMemcpyHostToDevice, st));
    {
        Scope sc(h, st, F_MISC, 0.0, (double)ib + (double)ob);
        HIPCHK(h, launch_tiles_overview((const uint8_t*)h->d_scratch[in_slot], cnx, cny, ox, oy, pnx, pny, (uint8_t*)h->d_scratch[out_slot], st));
    }
    if (out) HIPCHK(h, hipMemcpyAsync(out, h->d_scratch[out_slot], ob, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->tiles_slot = out_slot; h->tiles_nx = pnx; h->tiles_ny = pny;
    return S2SR_OK;
}

// The PNG files of the tile level the previous base / overview call left on the device: token statistics on the device, Huffman
// codes on the host, bit emission on the device, chunk framing + CRC + file writes on host threads (pngdev.hip).  Only the
// compressed streams cross PCIe.
static int tiles_write_png_locked(s2sr_handle* h, int32_t nx, int32_t ny, const char* const* paths, int32_t flags, int32_t* written);

int s2sr_tiles_write_png(s2sr_handle* h, int32_t nx, int32_t ny, const char* const* paths, int32_t flags, int32_t* written) {
    if (!h || !paths || nx <= 0 || ny <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return tiles_write_png_locked(h, nx, ny, paths, flags, written);
}

// The same with the XYZ layout spelled out instead of nx * ny path strings: tile (j, i) of the level goes to
// <dir>/<zoom>/<x0 + i>/<y_rows[j]>.png (gdal2tiles --xyz, reference tiling.py:138-186).  A z18 level is 9801 paths: built here they
// cost a millisecond, as Python strings plus a ctypes array 5-7 ms per level.
int s2sr_tiles_write_png_xyz(s2sr_handle* h, int32_t nx, int32_t ny, const char* dir, int32_t zoom, int32_t x0, const int32_t* y_rows,
                             int32_t flags, int32_t* written) {
    if (!h || !dir || !y_rows || nx <= 0 || ny <= 0 || zoom < 0) return S2SR_E_INVALID;
    const size_t dl = strlen(dir);
    if (dl == 0 || dl > 3800) return S2SR_E_INVALID;
    const size_t slot = dl + 48;                                  // "/zz/xxxxxxxxxx/yyyyyyyyyy.png" is at most 30 characters
    std::vector<char> text((size_t)nx * ny * slot);
    std::vector<const char*> paths((size_t)nx * ny);
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            char* p = text.data() + ((size_t)j * nx + i) * slot;
            snprintf(p, slot, "%s/%d/%d/%d.png", dir, zoom, x0 + i, y_rows[j]);
            paths[(size_t)j * nx + i] = p;
        }
    std::lock_guard<std::mutex> lk(h->mu);
    return tiles_write_png_locked(h, nx, ny, paths.data(), flags, written);
}

static int tiles_write_png_locked(s2sr_handle* h, int32_t nx, int32_t ny, const char* const* paths, int32_t flags, int32_t* written) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (h->tiles_slot < 0 || h->tiles_nx != nx || h->tiles_ny != ny)
        return fail(h, S2SR_E_INVALID, "the previous call on this handle did not leave a tile level of this size on the device");
    const int slot = h->tiles_slot;
    const uint8_t* d_tiles = (const uint8_t*)h->d_scratch[slot];
    const int n = nx * ny;
    hipStream_t st = h->stream;
    const bool timing = getenv("S2SR_PNG_TIMING") != nullptr;
    const bool row_threads = (flags & S2SR_PNG_ROW_THREADS) != 0;
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    double t_wait = 0, t_plan = 0, t_files = 0, t_hostenc = 0;
    // The level goes through in GROUPS of ~2048 tiles so that the device phases of one group run under the host phases of another
    // (r04 / first form of r05: one group = the level, the phases strictly one behind the other -- for z18's 9801 tiles 7 ms of
    // statistics kernel + copy and 7 ms of upload + emit kernel with idle CPUs, 5 ms of Huffman codes and 27 ms of framing / CRC /
    // file writes with an idle device).  All statistics kernels and their copies back are queued up front; then, group by group:
    // wait for the group's statistics, build its codes (host pool), queue its upload + emit kernel, and -- while that runs --
    // bring the PREVIOUS group's streams back and write its files.  Streams ping-pong between two device buffers.
    int ngroups = (flags & S2SR_PNG_SMALL_GROUPS) ? (n + 2) / 3 : (n <= 1536 ? 1 : (n + 2047) / 2048);   // (the flag: groups of 3, for the tests)
    if (const char* e = getenv("S2SR_PNG_GROUP_TILES")) {      // A/B knob (tools/tiles_ab.py): tiles per group, 0 = the whole level as one
        const int v = atoi(e);
        ngroups = v <= 0 ? 1 : (n + v - 1) / v;
    }
    const int gsz = (n + ngroups - 1) / ngroups;
    const size_t tile_stats_b = (512 + 512 + 1) * 4;                       // per tile: token histogram, row Adler pairs, any-alpha flag
    int rc;
    if ((rc = ensure_scratch(h, 2, (size_t)n * tile_stats_b))) return rc;
    if ((rc = ensure_scratch(h, 3, png_plan_bytes(n)))) return rc;
    // the statistics come back into, and the plans go up from, ONE page-locked block kept on the handle (a z18 level: 40 MB down,
    // 27 MB up; as fresh pageable vectors each crossed PCIe through the runtime's staging and was page-faulted in first)
    const size_t stats_b = ((size_t)n * tile_stats_b + 255) & ~(size_t)255, plan_b = png_plan_bytes(n);
    if (h->host_arena_bytes < stats_b + plan_b) {
        if (h->host_arena) HIPCHK(h, host_free(h->host_arena));
        h->host_arena = nullptr; h->host_arena_bytes = 0;
        const size_t want = (stats_b + plan_b + ((size_t)8 << 20)) & ~(((size_t)1 << 20) - 1);
        HIPCHK(h, host_malloc(&h->host_arena, want, hipHostMallocDefault));
        h->host_arena_bytes = want;
    }
    for (int i = 0; i < 2; ++i) {
        if (!h->stage_buf[i]) HIPCHK(h, host_malloc(&h->stage_buf[i], kStageBytes, hipHostMallocDefault));
        if (!h->stage_ev[i]) HIPCHK(h, hipEventCreateWithFlags(&h->stage_ev[i], hipEventDisableTiming));
    }
    struct Group {
        int a = 0, n = 0;                       // first tile, tiles
        uint32_t *d_stats = nullptr;            // device: [hist n x 512 | adler n x 512 | flag n]
        const uint32_t* stats = nullptr;        // ... its page-locked host copy
        uint8_t* d_tables = nullptr;            // device: the plan's upload block
        PngTilePlan plan;
        size_t out_words = 0;
        hipEvent_t ev_stats = nullptr, ev_emit = nullptr;
    };
    std::vector<Group> groups(ngroups);
    struct EventsBack {          // the groups' events go back to the handle's pool on every way out
        s2sr_handle* h; std::vector<Group>& gs;
        ~EventsBack() { for (Group& G : gs) { if (G.ev_stats) h->ev_pool.push_back(G.ev_stats); if (G.ev_emit) h->ev_pool.push_back(G.ev_emit); } }
    } events_back{h, groups};
    for (int g = 0; g < ngroups; ++g) {
        Group& G = groups[g];
        G.a = g * gsz;
        G.n = (G.a + gsz <= n ? gsz : n - G.a);
        G.d_stats = (uint32_t*)((char*)h->d_scratch[2] + (size_t)G.a * tile_stats_b);
        G.stats = (const uint32_t*)((const char*)h->host_arena + (size_t)G.a * tile_stats_b);
        G.d_tables = (uint8_t*)h->d_scratch[3] + png_plan_bytes(G.a);
        G.plan.arena = (char*)h->host_arena + stats_b + png_plan_bytes(G.a);
        G.plan.arena_bytes = png_plan_bytes(G.n);
        G.ev_stats = get_event(h);
        G.ev_emit = get_event(h);
        {
            Scope sc(h, st, F_MISC, 0.0, (double)G.n * 262144.0);      // algorithmic: every tile byte once
            HIPCHK(h, launch_png_tile_stats(d_tiles + (size_t)G.a * 262144, G.n, G.d_stats, G.d_stats + (size_t)G.n * 512,
                                            G.d_stats + (size_t)G.n * 1024, row_threads, st));
        }
        HIPCHK(h, hipMemcpyAsync((void*)G.stats, G.d_stats, (size_t)G.n * tile_stats_b, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipEventRecord(G.ev_stats, st));
    }
    std::atomic<int> failed{0};
    if (written) for (int t = 0; t < n; ++t) written[t] = 0;
    size_t total_words = 0, n_host = 0;

    // group g: its streams back in batches through the two page-locked staging buffers (while one batch is framed, checksummed and
    // written from its buffer by the host threads, the next one is on the wire), then the few tiles the host encoder takes
    auto write_group = [&](Group& G, const uint32_t* d_out) -> int {
        const PngTilePlan& plan = G.plan;
        const char* const* gpaths = paths + G.a;
        int32_t* gwritten = written ? written + G.a : nullptr;
        std::vector<int> host_tiles;
        for (int t = 0; t < G.n; ++t) if (plan.mode[t] == 2) host_tiles.push_back(t);
        std::vector<uint8_t> host_px(host_tiles.size() * (size_t)262144);
        for (size_t k = 0; k < host_tiles.size(); ++k)          // (noise: stored blocks are smaller than a Huffman block) their pixels
            HIPCHK(h, hipMemcpyAsync(host_px.data() + k * 262144, d_tiles + (size_t)(G.a + host_tiles[k]) * 262144, 262144, hipMemcpyDeviceToHost,
                                     h->copy_stream));
        struct Batch { int t0, t1; size_t w0, w1; };
        std::vector<Batch> batches;
        {
            const size_t cap_words = kStageBytes / 4;
            int t0 = 0;
            while (t0 < G.n) {
                int t1 = t0;
                const size_t w0 = plan.out_word[t0];
                auto end_of = [&](int t) { return t + 1 < G.n ? plan.out_word[t + 1] : G.out_words; };
                while (t1 < G.n && end_of(t1) - w0 <= cap_words) ++t1;
                if (t1 == t0) return fail(h, S2SR_E_CAPACITY, "a tile's stream is larger than a staging buffer");
                batches.push_back(Batch{t0, t1, w0, end_of(t1 - 1)});
                t0 = t1;
            }
        }
        for (size_t k = 0; k <= batches.size(); ++k) {
            if (k < batches.size() && batches[k].w1 > batches[k].w0)
                HIPCHK(h, hipMemcpyAsync(h->stage_buf[k & 1], d_out + batches[k].w0, (batches[k].w1 - batches[k].w0) * 4, hipMemcpyDeviceToHost,
                                         h->copy_stream));
            if (k < batches.size()) HIPCHK(h, hipEventRecord(h->stage_ev[k & 1], h->copy_stream));
            if (k > 0) {
                const Batch& bt = batches[k - 1];
                HIPCHK(h, hipEventSynchronize(h->stage_ev[(k - 1) & 1]));
                const uint32_t* words = (const uint32_t*)h->stage_buf[(k - 1) & 1];
                if (!png_parallel_for(bt.t1 - bt.t0, [&](int i) {
                    const int t = bt.t0 + i;
                    if (plan.mode[t] != 1) return;
                    static thread_local std::vector<uint8_t> buf;
                    if (!png_write_tile_file(gpaths[t], words + (plan.out_word[t] - bt.w0), plan.deflate_bytes[t], plan.eob[t], plan.eob_at[t],
                                             plan.adler[t], buf))
                        failed.store(1);
                    else if (gwritten) gwritten[t] = 1;
                })) failed.store(1);
            }
        }
        const double t0 = now();
        if (!host_tiles.empty()) {
            HIPCHK(h, hipStreamSynchronize(h->copy_stream));
            const size_t cap = s2sr_png_bound(256, 256, 4);
            if (!png_parallel_for((int)host_tiles.size(), [&](int k) {
                static thread_local std::vector<uint8_t> buf;
                buf.resize(cap);
                size_t len = 0;
                const int t = host_tiles[k];
                if (s2sr_png_encode(host_px.data() + (size_t)k * 262144, 256, 256, 4, 1024, buf.data(), cap, &len) != S2SR_OK ||
                    !png::write_file(gpaths[t], buf.data(), len))
                    failed.store(1);
                else if (gwritten) gwritten[t] = 1;
            })) failed.store(1);
            n_host += host_tiles.size();
        }
        t_hostenc += now() - t0;
        return S2SR_OK;
    };

    for (int g = 0; g <= ngroups; ++g) {
        if (g < ngroups) {
            Group& G = groups[g];
            double t0 = now();
            HIPCHK(h, hipEventSynchronize(G.ev_stats));
            double t1 = now();
            t_wait += t1 - t0;
            G.out_words = png_plan_tiles(G.n, G.stats, G.stats + (size_t)G.n * 512, G.stats + (size_t)G.n * 1024, paths + G.a,
                                         (flags & S2SR_PNG_SKIP_TRANSPARENT) != 0, (flags & S2SR_PNG_HOST_ENCODER) != 0, &G.plan);
            t_plan += now() - t1;
            if (G.plan.failed) { return fail(h, S2SR_E_IO, "planning the tile streams failed (an encoder thread ran out of memory)"); }
            total_words += G.out_words;
            const int oslot = 4 + (g & 1);                       // the group's stream buffer: scratch 4 / 5 in turn
            if ((rc = ensure_scratch(h, oslot, (G.out_words + 1) * 4))) return rc;
            uint32_t* d_out = (uint32_t*)h->d_scratch[oslot];
            HIPCHK(h, hipMemcpyAsync(G.d_tables, G.plan.tb, G.plan.upload_bytes, hipMemcpyHostToDevice, st));
            HIPCHK(h, hipMemsetAsync(d_out, 0, (G.out_words + 1) * 4, st));
            {
                Scope sc(h, st, F_MISC, 0.0, (double)G.n * 262144.0 + (double)G.out_words * 4.0);
                const size_t tb_b = (size_t)G.n * 512 * 4, hdr_b = (size_t)G.n * 160 * 4;
                HIPCHK(h, launch_png_tile_emit(d_tiles + (size_t)G.a * 262144, G.n, G.d_tables + tb_b + hdr_b, (const uint32_t*)G.d_tables,
                                               (const uint32_t*)(G.d_tables + tb_b), d_out, row_threads, st));
            }
            HIPCHK(h, hipEventRecord(G.ev_emit, st));
        }
        if (g > 0) {
            Group& P = groups[g - 1];
            double t0 = now();
            HIPCHK(h, hipEventSynchronize(P.ev_emit));           // the copy stream may read the group's streams
            double t1 = now();
            t_wait += t1 - t0;
            if ((rc = write_group(P, (const uint32_t*)h->d_scratch[4 + ((g - 1) & 1)]))) return rc;
            t_files += now() - t1;
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    if (timing)
        fprintf(stderr, "[s2sr png] %d tiles in %d group(s) (%zu on the host encoder), %.1f ms: waiting for the device %.1f, Huffman codes %.1f, "
                "streams (%.0f MB) back in batches + files %.1f (of which host-encoded tiles %.1f)\n", n, ngroups, n_host, now() - t_begin, t_wait,
                t_plan, (double)total_words * 4 / 1e6, t_files, t_hostenc);
    h->tiles_slot = slot; h->tiles_nx = nx; h->tiles_ny = ny;      // the scratch requests above dropped the marker; the level is intact
    if (failed.load()) return fail(h, S2SR_E_IO, "a tile file could not be written (or an encoder thread ran out of memory)");
    return S2SR_OK;
}

int s2sr_set_profiling(s2sr_handle* h, int32_t on) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->prof = on < 0 ? 0 : on;
    h->span_on = false; h->span_count = 0;
    for (int i = 0; i < 16; ++i) h->fam_count[i] = 0;
    return S2SR_OK;
}

int s2sr_reset_kernel_stats(s2sr_handle* h) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = collect_events(h);
    for (int i = 0; i < F_COUNT; ++i) { h->stats[i].launches = 0; h->stats[i].total_ms = 0; h->stats[i].flops = 0; h->stats[i].bytes = 0; }
    return rc;
}

int s2sr_get_kernel_stats(s2sr_handle* h, s2sr_kstat* out, int32_t cap, int32_t* n) {
    if (!h || !n) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = collect_events(h);
    if (rc) return rc;
    *n = F_COUNT;
    if (!out) return S2SR_OK;
    if (cap < F_COUNT) return S2SR_E_CAPACITY;
    for (int i = 0; i < F_COUNT; ++i) out[i] = h->stats[i];
    return S2SR_OK;
}

int s2sr_graph_stats(s2sr_handle* h, int64_t* captures, int64_t* replays) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (captures) *captures = h->graph_captures;
    if (replays) *replays = h->graph_replays;
    return S2SR_OK;
}

int s2sr_synchronize(s2sr_handle* h) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, dev_sync());
    return S2SR_OK;
}

// Per-tensor-kind activation scales of the fp8 trunk from data: one forward of the calibration tiles with wide scales
// (nothing clips), the largest |x| of the trunk and |x_k| of the growth planes over all RDBs, then the largest exponents
// that keep `headroom` x those maxima below e4m3's 448.
int s2sr_calibrate_fp8(s2sr_handle* h, const uint8_t* tiles, int32_t B, int32_t th, int32_t tw, float headroom, int32_t* x_exp,
                       int32_t* g_exp) {
    if (!h || !tiles || B <= 0 || th <= 0 || tw <= 0 || !(headroom >= 1.0f)) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cfg.precision != S2SR_PREC_FP8) return fail(h, S2SR_E_INVALID, "s2sr_calibrate_fp8 needs a handle created with S2SR_PREC_FP8");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t ib = (size_t)B * th * tw * 3, ob = ib * h->cfg.scale * h->cfg.scale;
    int rc = ensure_scratch(h, 0, ib);
    if (rc) return rc;
    if ((rc = ensure_scratch(h, 1, ob))) return rc;
    float* d_c = nullptr;
    HIPCHK(h, dev_malloc(&d_c, 2 * sizeof(float)));
    HIPCHK(h, hipMemcpyAsync(h->d_scratch[0], tiles, ib, hipMemcpyHostToDevice, h->stream));
    const int old_x = h->fp8_x_exp, old_g = h->fp8_g_exp, old_prof = h->prof;
    const bool old_graphs = h->graphs_on;
    float m[2] = {0.f, 0.f};
    hipError_t e = hipSuccess;
    // The measuring pass itself stores e4m3 planes: with scales 2^mx / 2^mg it sees values up to 448 / 2^mx (trunk) and
    // 448 / 2^mg (growth) and clips beyond.  Start wide (trunk up to 448, growth up to 112); a maximum that reaches the
    // pass's own ceiling means "at least this much": measure again 8x wider (twice at most, then report it).
    int mx = 0, mg = 2;
    bool clipped = false;
    for (int attempt = 0; attempt < 3; ++attempt) {
        hipError_t e0 = hipMemsetAsync(d_c, 0, 2 * sizeof(float), h->stream);
        if (e0 != hipSuccess) { dev_free(d_c); return fail(h, S2SR_E_HIP, "calibration memset failed"); }
        h->fp8_x_exp = mx; h->fp8_g_exp = mg;
        h->graphs_on = false; h->prof = 0;
        h->d_calib = d_c;
        rc = forward_dev(h, h->stream, (const uint8_t*)h->d_scratch[0], nullptr, B, th, tw, (uint8_t*)h->d_scratch[1], nullptr);
        h->d_calib = nullptr;
        h->graphs_on = old_graphs; h->prof = old_prof;
        e = hipMemcpyAsync(m, d_c, sizeof m, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (rc || e != hipSuccess) break;
        const bool cx = m[0] >= 0.98f * ldexpf(448.0f, -mx), cg = m[1] >= 0.98f * ldexpf(448.0f, -mg);
        clipped = cx || cg;
        if (!clipped || attempt == 2) break;
        if (cx) mx -= 3;
        if (cg) mg -= 3;
    }
    dev_free(d_c);
    if (rc || e != hipSuccess) {
        h->fp8_x_exp = old_x; h->fp8_g_exp = old_g;
        return rc ? rc : fail(h, S2SR_E_HIP, std::string("calibration read-back failed: ") + hipGetErrorString(e));
    }
    if (clipped) {
        h->fp8_x_exp = old_x; h->fp8_g_exp = old_g;
        char b[200];
        snprintf(b, sizeof b, "fp8 calibration: activations still reach the measuring pass's ceiling at scales 2^%d / 2^%d (|x| >= %g, |x_k| >= %g)",
                 mx, mg, m[0], m[1]);
        return fail(h, S2SR_E_INVALID, b);
    }
    auto pick = [&](float vmax, int fallback) {
        if (!(vmax > 0.f)) return fallback;
        int k = (int)floorf(log2f(448.0f / (vmax * headroom)));
        return k > 12 ? 12 : (k < -8 ? -8 : k);
    };
    drop_graphs(h);                            // captured launches carry the old exponents
    h->fp8_x_exp = pick(m[0], old_x);
    h->fp8_g_exp = pick(m[1], old_g);
    if (x_exp) *x_exp = h->fp8_x_exp;
    if (g_exp) *g_exp = h->fp8_g_exp;
    return S2SR_OK;
}

uint8_t s2sr_debug_f32_to_e4m3(float v) { return f32_to_e4m3(v); }

size_t s2sr_debug_pack_f8_bytes(int32_t cin, int32_t cout) {
    if (cin <= 0 || cout <= 0 || cout > 64) return 0;
    return conv_wpack_bytes_f8(cin, cout);
}

int s2sr_debug_pack_f8(const float* w, int32_t cin, int32_t cout, uint8_t* out, int32_t* wscale) {
    if (!w || !out || !wscale || cin <= 0 || cout <= 0 || cout > 64) return S2SR_E_INVALID;
    pack_conv_weights_f8(w, cin, cout, out, wscale);
    return S2SR_OK;
}

int s2sr_debug_conv(s2sr_handle* h, const float* x, int32_t N, int32_t Cin, int32_t H, int32_t W, const float* weight,
                    const float* bias, int32_t Cout, int32_t upsample, int32_t act, float* y) {
    if (!h || !x || !weight || !bias || !y || N <= 0 || Cin <= 0 || Cout <= 0 || Cout > 64 || H <= 0 || W <= 0)
        return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const int NB = (Cin + 15) / 16;
    const int OHh = upsample ? 2 * H : H, OWw = upsample ? 2 * W : W;
    const int sHp = padded(H), sWp = padded(W), Hp = padded(OHh), Wp = padded(OWw);
    const size_t sblk = (size_t)sHp * sWp * 32;
    const size_t plane_b = (size_t)N * NB * sblk, xb = (size_t)N * Cin * H * W * 4,
                 yb = (size_t)N * Cout * OHh * OWw * 4, wb = conv_wpack_bytes(Cin, Cout);
    char *d_plane = nullptr, *d_w = nullptr;
    float *d_x = nullptr, *d_y = nullptr, *d_b = nullptr;
    HIPCHK(h, dev_malloc(&d_plane, plane_b));
    HIPCHK(h, dev_malloc(&d_x, xb));
    HIPCHK(h, dev_malloc(&d_y, yb));
    HIPCHK(h, dev_malloc(&d_w, wb));
    HIPCHK(h, dev_malloc(&d_b, 64 * 4));
    std::vector<char> wp(wb);
    pack_conv_weights(weight, Cin, Cout, 1, wp.data());
    float bb[64] = {0};
    memcpy(bb, bias, Cout * sizeof(float));
    HIPCHK(h, hipMemsetAsync(d_plane, 0, plane_b, st));
    HIPCHK(h, hipMemcpyAsync(d_x, x, xb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(d_w, wp.data(), wb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(d_b, bb, sizeof bb, hipMemcpyHostToDevice, st));
    HIPCHK(h, launch_pack_f32_nchw(d_x, N, Cin, H, W, 1.0f, d_plane, NB, sHp, sWp, st));
    ConvParams p{};
    p.src = d_plane; p.src_img = (uint64_t)NB * sblk; p.nstage = NB;
    p.wpack = d_w; p.bias = d_b; p.N = N; p.H = OHh; p.W = OWw; p.Hp = Hp; p.Wp = Wp; p.sHp = sHp; p.sWp = sWp;
    p.out_f32 = d_y; p.cout = Cout; p.act = act; p.trash = h->d_trash;
    HIPCHK(h, launch_conv(p, (Cout + 31) / 32, EPI_DEBUG, upsample != 0, false, st));
    HIPCHK(h, hipMemcpyAsync(y, d_y, yb, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    dev_free(d_plane); dev_free(d_x); dev_free(d_y); dev_free(d_w); dev_free(d_b);
    return S2SR_OK;
}

// diagnostic (bench.py secondary.mfma_ceiling): `launches` back-to-back launches of one of the three loops of ceiling.hip on one
// workgroup per CU, timed with an event pair on the handle's stream behind launches / 4 + 1 untimed ones (the clock settles under load)
int s2sr_debug_mfma_ceiling(s2sr_handle* h, int32_t mode, int32_t stages, int32_t launches, double* flop_per_launch, double* dma_bytes_per_launch,
                            float* ms_total) {
    if (!h || mode < 0 || mode > 8 || stages <= 0 || launches <= 0 || !ms_total) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->cfg.device);
    const size_t src_bytes = (size_t)336 << 20;          // what a conv1-4 launch of 16 images fills its rings with; larger than L2 + MALL
    int rc = ensure_scratch(h, 2, src_bytes);
    if (rc) return rc;
    const size_t sink_bytes = (size_t)ncu * 512 * 4, store_bytes = (size_t)64 << 20;      // mode 5 streams its stores through 64 MB
    if ((rc = ensure_scratch(h, 3, sink_bytes + store_bytes))) return rc;
    char* d_store = (char*)h->d_scratch[3] + sink_bytes;
    hipStream_t st = h->stream;
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    HIPCHK(h, launch_mfma_ceiling(mode, (char*)h->d_scratch[2], src_bytes, true /* fill the operands: 0.1 ms */, (float*)h->d_scratch[3], ncu, stages, d_store,
                                  store_bytes, st));
    for (int i = 0; i < launches / 4; ++i)
        HIPCHK(h, launch_mfma_ceiling(mode, (char*)h->d_scratch[2], src_bytes, false, (float*)h->d_scratch[3], ncu, stages, d_store, store_bytes, st));
    HIPCHK(h, hipEventRecord(e0, st));
    for (int i = 0; i < launches; ++i)
        HIPCHK(h, launch_mfma_ceiling(mode, (char*)h->d_scratch[2], src_bytes, false, (float*)h->d_scratch[3], ncu, stages, d_store, store_bytes, st));
    HIPCHK(h, hipEventRecord(e1, st));
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipEventElapsedTime(ms_total, e0, e1));
    h->ev_pool.push_back(e0); h->ev_pool.push_back(e1);
    if (flop_per_launch) *flop_per_launch = mfma_ceiling_flop_per_launch(mode, ncu, stages);
    if (dma_bytes_per_launch) *dma_bytes_per_launch = mfma_ceiling_dma_bytes_per_launch(mode, ncu, stages);
    return S2SR_OK;
}

// diagnostic prototype (persist.hip): `launches` launches of the RDB-shaped loop whose workgroups stay across layers, `grid` workgroups (<= one per
// CU: they must all be resident) of `P` patches each, `rdbs` RDBs per launch; flags in uncached device memory, zeroed in front of every launch
int s2sr_debug_rdb_persistent(s2sr_handle* h, int32_t variant, int32_t grid, int32_t P, int32_t rdbs, int32_t launches, double* flop_per_launch,
                              float* ms_total, int32_t* timeouts, int32_t* mismatches) {
    if (!h || variant < 0 || variant > 5 || grid < 2 || P < 2 || P > 4 || rdbs < 1 || rdbs > 4000 || launches < 1 || !ms_total) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->compact()) return fail(h, S2SR_E_INVALID, "s2sr_debug_rdb_persistent: RRDB handles only");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->cfg.device);
    if (grid > ncu) return fail(h, S2SR_E_INVALID, "more workgroups than CUs: they would not all be resident");
    const size_t wts_bytes = (size_t)8 << 20, ws_bytes = rdb_persistent_ws_bytes(variant, grid, P), sink_bytes = (size_t)grid * 512 * 4;
    int rc = ensure_scratch(h, 2, wts_bytes);
    if (rc) return rc;
    if ((rc = ensure_scratch(h, 3, sink_bytes + 256))) return rc;
    if ((rc = ensure_scratch(h, 4, ws_bytes))) return rc;
    struct Uncached {
        void* p = nullptr;
        ~Uncached() { if (p) (void)hipFree(p); }
    } fl;
    const size_t flag_bytes = ((size_t)grid * P + 1) * 4;
    HIPCHK(h, hipExtMallocWithFlags(&fl.p, flag_bytes, hipDeviceMallocUncached));
    uint32_t* d_timeouts = (uint32_t*)((char*)h->d_scratch[3] + sink_bytes);
    hipStream_t st = h->stream;
    // operand data: the ceiling loops' generator fills the weights buffer and the working set (toggle rates as there)
    HIPCHK(h, launch_mfma_ceiling(0, (char*)h->d_scratch[2], wts_bytes, true, (float*)h->d_scratch[3], 1, 1, nullptr, 0, st));
    HIPCHK(h, launch_mfma_ceiling(0, (char*)h->d_scratch[4], ws_bytes, true, (float*)h->d_scratch[3], 1, 1, nullptr, 0, st));
    HIPCHK(h, hipMemsetAsync(d_timeouts, 0, 12, st));
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    auto one = [&]() -> int {
        HIPCHK(h, hipMemsetAsync(fl.p, 0, flag_bytes, st));
        HIPCHK(h, launch_rdb_persistent(variant, (const char*)h->d_scratch[2], wts_bytes, (char*)h->d_scratch[4], (uint32_t*)fl.p, (float*)h->d_scratch[3],
                                        grid, P, rdbs, d_timeouts, st));
        return S2SR_OK;
    };
    for (int i = 0; i < launches / 4 + 1; ++i)
        if ((rc = one())) return rc;
    HIPCHK(h, hipEventRecord(e0, st));
    for (int i = 0; i < launches; ++i)
        if ((rc = one())) return rc;
    HIPCHK(h, hipEventRecord(e1, st));
    uint32_t to[3] = {0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(to, d_timeouts, 12, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipEventElapsedTime(ms_total, e0, e1));
    h->ev_pool.push_back(e0); h->ev_pool.push_back(e1);
    if (flop_per_launch) *flop_per_launch = rdb_persistent_flop_per_launch(grid, P, rdbs);
    if (timeouts) *timeouts = (int32_t)to[0];
    if (mismatches) { mismatches[0] = (int32_t)to[1]; mismatches[1] = (int32_t)to[2]; }
    return S2SR_OK;
}

int s2sr_debug_get_config(s2sr_handle* h, s2sr_debug_config* out) {
    if (!h || !out) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    memset(out, 0, sizeof *out);
    // trunk_w4 always 1; trunk_wino, fp8_form, reserved[1] and reserved[3] always 0 (the forms they named were removed)
    out->precision = h->cfg.precision; out->group = h->cfg.group; out->trunk_w4 = 1; out->lo_exp = h->lo_exp;
    out->fp8_x_exp = h->fp8_x_exp; out->fp8_g_exp = h->fp8_g_exp; out->fp8_hp_tail = h->fp8_hp_tail ? 1 : 0;
    out->graphs_on = h->graphs_on ? 1 : 0; out->reserved[0] = h->mosaic_on ? 1 : 0; out->reserved[2] = h->last_fold ? 1 : 0; out->reserved[4] = h->f16_full ? 1 : 0; out->reserved[5] = (int32_t)h->ws_allocs;
    return S2SR_OK;
}

// One RDB-shaped conv through conv_trunk_f16 / conv_trunk_f8.  Host-side packing and decoding (a test hook: clarity over
// speed); the weights go through the production device packers (pack.hip).
int s2sr_debug_conv_trunk(s2sr_handle* h, const s2sr_debug_trunk_args* a) {
    if (!h || !a || !a->x || !a->weight || !a->bias || !a->y) return S2SR_E_INVALID;
    if (h->compact()) return S2SR_E_INVALID;     // RRDB handles only
    const int kind = a->kind, N = a->N, Cin = a->Cin, H = a->H, W = a->W;
    if (kind < 0 || kind > 5 || N <= 0 || H <= 0 || W <= 0) return S2SR_E_INVALID;
    const bool f8 = kind >= 3, c5 = (kind % 3) != 0, rr = (kind % 3) == 2;
    const int Cout = c5 ? 64 : 32;
    if (c5 ? Cin != 192 : (Cin != 64 && Cin != 96 && Cin != 128 && Cin != 160)) return fail(h, S2SR_E_INVALID, "Cin does not match the RDB form");
    if (rr && !a->skip) return fail(h, S2SR_E_INVALID, "rdb3 form needs skip");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const int Hp = padded(H), Wp = padded(W);
    const size_t ppx = (size_t)Hp * Wp, blk = ppx * 32;
    auto pix = [&](int y, int x) { return (size_t)(y + 1) * Wp + (x + 1); };
    // ---- weights through the production device packers
    DevBuf d_w32, d_wp, d_b, d_ws;
    const size_t wn = (size_t)Cout * Cin * 9;
    HIPCHK(h, dev_malloc(&d_w32.p, wn * 4));
    HIPCHK(h, hipMemcpyAsync(d_w32.p, a->weight, wn * 4, hipMemcpyHostToDevice, st));
    HIPCHK(h, dev_malloc(&d_wp.p, f8 ? conv_wpack_bytes_f8(Cin, Cout) : conv_wpack_bytes(Cin, Cout)));
    HIPCHK(h, dev_malloc(&d_b.p, 64 * 4));
    HIPCHK(h, dev_malloc(&d_ws.p, 64 * 4));
    float bb[64] = {0};
    memcpy(bb, a->bias, Cout * sizeof(float));
    HIPCHK(h, hipMemcpyAsync(d_b.p, bb, sizeof bb, hipMemcpyHostToDevice, st));
    if (f8) HIPCHK(h, launch_pack_trunk_f8((const float*)d_w32.p, Cin, Cout, d_wp.p, (int32_t*)d_ws.p, st));
    else HIPCHK(h, launch_pack_trunk_f16((const float*)d_w32.p, Cin, Cout, d_wp.p, st));
    // ---- activations: the dense tensor D (12 fp16 blocks per image, or 6 e4m3 planes), packed on the host
    const int xe = h->fp8_x_exp, ge = h->fp8_g_exp, le = h->lo_exp;
    const size_t dimg = (f8 ? 6 : 12) * blk;
    std::vector<char> D((size_t)N * dimg, 0);
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < Cin; ++c)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const float v = a->x[(((size_t)n * Cin + c) * H + y) * W + x];
                    if (f8) {
                        const float sc = ldexpf(v, c < 64 ? xe : ge);
                        ((uint8_t*)D.data())[(size_t)n * dimg + (size_t)(c >> 5) * blk + pix(y, x) * 32 + (c & 31)] = f32_to_e4m3(sc);
                    } else {
                        ((hf16*)(D.data() + (size_t)n * dimg + (size_t)(c >> 4) * blk + pix(y, x) * 32))[c & 15] = (hf16)v;
                    }
                }
    // a 64-channel NCHW tensor as (fp16 hi blocks [4], e4m3(lo * 2^le) planes [2]) or as fp16 only
    auto split64 = [&](const float* src, std::vector<char>& hi, size_t hi_img, std::vector<char>* lo8, bool hi_is_value) {
        for (int n = 0; n < N; ++n)
            for (int c = 0; c < 64; ++c)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        const float v = src ? src[(((size_t)n * 64 + c) * H + y) * W + x] : 0.f;
                        const hf16 hv = (hf16)v;
                        if (hi_is_value) ((hf16*)(hi.data() + (size_t)n * hi_img + (size_t)(c >> 4) * blk + pix(y, x) * 32))[c & 15] = hv;
                        if (lo8) {
                            const float l = hi_is_value ? v - (float)hv : v;
                            ((uint8_t*)lo8->data())[(size_t)n * 2 * blk + (size_t)(c >> 5) * blk + pix(y, x) * 32 + (c & 31)] = f32_to_e4m3(ldexpf(l, le));
                        }
                    }
    };
    DevBuf d_D, d_D2, d_Tin, d_Tout, d_Sk, d_SkLo, d_Xin, d_Xout;
    HIPCHK(h, dev_malloc(&d_D.p, D.size()));
    HIPCHK(h, hipMemcpyAsync(d_D.p, D.data(), D.size(), hipMemcpyHostToDevice, st));
    ConvParams p{};
    p.N = N; p.H = H; p.W = W; p.Hp = Hp; p.Wp = Wp; p.sHp = Hp; p.sWp = Wp;
    p.src = (const char*)d_D.p; p.src_img = dimg; p.wpack = d_wp.p; p.bias = (const float*)d_b.p; p.trash = h->d_trash;
    const int epi = !c5 ? EPI_LRELU : (rr ? EPI_RDB5_RRDB : EPI_RDB5);
    std::vector<char> tmp;
    if (!f8) {
        p.nstage = Cin / 16; p.seg_len = p.nstage; p.lo_exp = le;
        if (!c5) {
            p.dst = (char*)d_D.p + (size_t)(Cin / 16) * blk; p.dst_img = dimg;       // the next growth slot of the same dense tensor
        } else {
            HIPCHK(h, dev_malloc(&d_D2.p, D.size()));
            HIPCHK(h, hipMemsetAsync(d_D2.p, 0, D.size(), st));
            p.dst = (char*)d_D2.p; p.dst_img = dimg;
            std::vector<char> lo8((size_t)N * 2 * blk, 0), none;
            split64(a->lo, none, 0, &lo8, false);
            HIPCHK(h, dev_malloc(&d_Tin.p, lo8.size()));
            HIPCHK(h, dev_malloc(&d_Tout.p, lo8.size()));
            HIPCHK(h, hipMemcpyAsync(d_Tin.p, lo8.data(), lo8.size(), hipMemcpyHostToDevice, st));
            HIPCHK(h, hipMemsetAsync(d_Tout.p, 0, lo8.size(), st));
            HIPCHK(h, hipStreamSynchronize(st));
            p.xh_in = (const char*)d_Tin.p; p.T = (char*)d_Tout.p;
            if (rr) {
                std::vector<char> shi((size_t)N * 4 * blk, 0), slo((size_t)N * 2 * blk, 0);
                split64(a->skip, shi, 4 * blk, &slo, true);
                HIPCHK(h, dev_malloc(&d_Sk.p, shi.size()));
                HIPCHK(h, dev_malloc(&d_SkLo.p, slo.size()));
                HIPCHK(h, hipMemcpyAsync(d_Sk.p, shi.data(), shi.size(), hipMemcpyHostToDevice, st));
                HIPCHK(h, hipMemcpyAsync(d_SkLo.p, slo.data(), slo.size(), hipMemcpyHostToDevice, st));
                HIPCHK(h, hipStreamSynchronize(st));
                p.xh_skip = (const char*)d_Sk.p; p.xh_img = 4 * blk; p.lo_skip = (const char*)d_SkLo.p;
            }
        }
        const hipError_t e = launch_conv_trunk(p, Cout / 32, epi, st, a->form);
        if (e != hipSuccess) return fail(h, S2SR_E_HIP, std::string("launch_conv_trunk: ") + hipGetErrorString(e));
    } else {
        p.seg_len = Cin / 32; p.nstage = (p.seg_len + 1) & ~1; p.wscale = (const int32_t*)d_ws.p;
        p.x_exp = xe; p.g_exp = ge; p.xh_img = 4 * blk;
        if (!c5) {
            p.dst = (char*)d_D.p + (size_t)(Cin / 32) * blk; p.dst_img = dimg;
        } else {
            HIPCHK(h, dev_malloc(&d_D2.p, D.size()));
            HIPCHK(h, hipMemsetAsync(d_D2.p, 0, D.size(), st));
            p.dst = (char*)d_D2.p; p.dst_img = dimg;
            std::vector<char> xin((size_t)N * 4 * blk, 0);      // the fp16 trunk = the first 64 of the Cin input channels
            for (int n = 0; n < N; ++n)
                for (int c = 0; c < 64; ++c)
                    for (int y = 0; y < H; ++y)
                        for (int x = 0; x < W; ++x)
                            ((hf16*)(xin.data() + (size_t)n * 4 * blk + (size_t)(c >> 4) * blk + pix(y, x) * 32))[c & 15] =
                                (hf16)a->x[(((size_t)n * Cin + c) * H + y) * W + x];
            HIPCHK(h, dev_malloc(&d_Xin.p, xin.size()));
            HIPCHK(h, dev_malloc(&d_Xout.p, xin.size()));
            HIPCHK(h, hipMemcpyAsync(d_Xin.p, xin.data(), xin.size(), hipMemcpyHostToDevice, st));
            HIPCHK(h, hipMemsetAsync(d_Xout.p, 0, xin.size(), st));
            HIPCHK(h, hipStreamSynchronize(st));
            p.xh_in = (const char*)d_Xin.p; p.xh_out = (char*)d_Xout.p;
            if (rr) {
                std::vector<char> shi((size_t)N * 4 * blk, 0);
                split64(a->skip, shi, 4 * blk, nullptr, true);
                HIPCHK(h, dev_malloc(&d_Sk.p, shi.size()));
                HIPCHK(h, hipMemcpyAsync(d_Sk.p, shi.data(), shi.size(), hipMemcpyHostToDevice, st));
                HIPCHK(h, hipStreamSynchronize(st));
                p.xh_skip = (const char*)d_Sk.p;
            }
        }
        // conv1-4: the loader-wave form is the only one (the others the measurements buried are refused)
        const hipError_t e = (kind == 3 && a->form != 0) ? hipErrorNotSupported : launch_conv_trunk_f8(p, Cout / 32, epi, st);
        if (e != hipSuccess) return fail(h, S2SR_E_HIP, std::string("launch_conv_trunk_f8: ") + hipGetErrorString(e));
    }
    HIPCHK(h, hipStreamSynchronize(st));
    // ---- read back and decode
    auto get = [&](const void* d, size_t bytes) -> int {
        tmp.resize(bytes);
        HIPCHK(h, copy_blocking(h, tmp.data(), d, bytes, hipMemcpyDeviceToHost));
        return S2SR_OK;
    };
    int rc;
    auto for_out = [&](int C, auto fn) {
        for (int n = 0; n < N; ++n)
            for (int c = 0; c < C; ++c)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) fn(n, c, y, x, (((size_t)n * C + c) * H + y) * W + x);
    };
    if (!f8 && !c5) {
        if ((rc = get(d_D.p, D.size()))) return rc;
        const size_t ob = (size_t)(Cin / 16) * blk;
        for_out(32, [&](int n, int c, int y, int x, size_t o) {
            a->y[o] = (float)((const hf16*)(tmp.data() + (size_t)n * dimg + ob + (size_t)(c >> 4) * blk + pix(y, x) * 32))[c & 15];
        });
    } else if (!f8) {
        if ((rc = get(d_D2.p, D.size()))) return rc;
        std::vector<char> hi = tmp;
        if ((rc = get(d_Tout.p, (size_t)N * 2 * blk))) return rc;
        for_out(64, [&](int n, int c, int y, int x, size_t o) {
            const float hv = (float)((const hf16*)(hi.data() + (size_t)n * dimg + (size_t)(c >> 4) * blk + pix(y, x) * 32))[c & 15];
            const uint8_t lb = ((const uint8_t*)tmp.data())[(size_t)n * 2 * blk + (size_t)(c >> 5) * blk + pix(y, x) * 32 + (c & 31)];
            a->y[o] = hv + ldexpf(e4m3_to_f32(lb), -le);
        });
    } else if (!c5) {
        if ((rc = get(d_D.p, D.size()))) return rc;
        const size_t ob = (size_t)(Cin / 32) * blk;
        for_out(32, [&](int n, int c, int y, int x, size_t o) {
            a->y[o] = ldexpf(e4m3_to_f32(((const uint8_t*)tmp.data())[(size_t)n * dimg + ob + pix(y, x) * 32 + c]), -ge);
        });
    } else {
        if ((rc = get(d_Xout.p, (size_t)N * 4 * blk))) return rc;
        for_out(64, [&](int n, int c, int y, int x, size_t o) {
            a->y[o] = (float)((const hf16*)(tmp.data() + (size_t)n * 4 * blk + (size_t)(c >> 4) * blk + pix(y, x) * 32))[c & 15];
        });
        if (a->y_aux) {
            if ((rc = get(d_D2.p, D.size()))) return rc;
            for_out(64, [&](int n, int c, int y, int x, size_t o) {
                a->y_aux[o] = ldexpf(e4m3_to_f32(((const uint8_t*)tmp.data())[(size_t)n * dimg + (size_t)(c >> 5) * blk + pix(y, x) * 32 + (c & 31)]), -xe);
            });
        }
    }
    return S2SR_OK;
}

int s2sr_debug_bench_conv(s2sr_handle* h, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t iters,
                          float* avg_us, uint64_t* trace, int32_t trace_wgs) {
    if (!h || !avg_us || N <= 0 || H <= 0 || W <= 0 || iters <= 0 || cin < 16 || cin > 192 || cin % 16 ||
        (cout != 32 && cout != 64))
        return S2SR_E_INVALID;
    if (trace && trace_wgs > 0) return fail(h, S2SR_E_INVALID, "stamped kernel builds are not part of this library");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const int Hp = padded(H), Wp = padded(W);
    const size_t blk = (size_t)Hp * Wp * 32;
    const size_t wb = conv_wpack_bytes(cin, cout), db = (size_t)N * 12 * blk;
    DevBuf D0, D1, T, Rr, d_w, d_b;
    HIPCHK(h, dev_malloc(&D0.p, db));
    HIPCHK(h, dev_malloc(&D1.p, db));
    HIPCHK(h, dev_malloc(&T.p, (size_t)N * 4 * blk));
    HIPCHK(h, dev_malloc(&Rr.p, (size_t)N * 8 * blk));
    HIPCHK(h, dev_malloc(&d_w.p, wb));
    HIPCHK(h, dev_malloc(&d_b.p, 256));
    // pseudo-random fp16 bit patterns (finite, |v| < 2)
    std::vector<unsigned char> pat(db > wb ? db : wb);
    unsigned s = 12345u;
    for (size_t i = 0; i + 1 < pat.size(); i += 2) {
        s = s * 1664525u + 1013904223u;
        pat[i] = (unsigned char)(s >> 24);
        pat[i + 1] = (unsigned char)(((s >> 16) & 0x80) | 0x30 | ((s >> 8) & 0x0b));
    }
    HIPCHK(h, copy_blocking(h, D0.p, pat.data(), db, hipMemcpyHostToDevice));
    HIPCHK(h, copy_blocking(h, d_w.p, pat.data(), wb, hipMemcpyHostToDevice));
    HIPCHK(h, fill_blocking(h, D1.p, 0, db));
    HIPCHK(h, fill_blocking(h, T.p, 0, (size_t)N * 4 * blk));
    HIPCHK(h, fill_blocking(h, Rr.p, 0, (size_t)N * 8 * blk));
    HIPCHK(h, fill_blocking(h, d_b.p, 0, 256));
    ConvParams p{};
    p.src = (const char*)D0.p; p.src_img = 12 * blk; p.nstage = cin / 16;
    p.wpack = d_w.p; p.bias = (const float*)d_b.p; p.N = N; p.H = H; p.W = W; p.Hp = Hp; p.Wp = Wp; p.sHp = Hp; p.sWp = Wp;
    p.T = (char*)T.p; p.R = (float*)Rr.p; p.F = (float*)Rr.p; p.trash = h->d_trash;
    p.xh_in = (const char*)T.p; p.lo_exp = h->lo_exp;   // conv_trunk_f16: trunk lo coming in (here read and written in place: timing only)
    p.dst = (char*)D1.p; p.dst_img = 12 * blk;
    p.f16_form = (h->small8 ? 0 : 2) | (h->f16_full ? 0 : 4);
    const int epi = cout == 32 ? EPI_LRELU : EPI_RDB5, ct = cout / 32;
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return fail(h, S2SR_E_HIP, "hipEventCreate failed"); }
    hipError_t e = hipSuccess;
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = launch_conv_trunk(p, ct, epi, st);
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch_conv_trunk(p, ct, epi, st);
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    HIPCHK(h, e);
    *avg_us = ms * 1000.0f / iters;
    return S2SR_OK;
}

namespace {
// The launch plan a tap hook's batch gets from forward_dev (s2sr_forward_part_u8_dev: the job's mosaic) and the one launch group /
// mosaic segment it must be.
struct TapPlan {
    Mosaic plan;
    int NI = 0, skx = 0, sky = 0, SH = 0, SW = 0, IH = 0, IW = 0;
};
int tap_plan(s2sr_handle* h, bool u8, int32_t B, int32_t th, int32_t tw, int32_t job_windows, TapPlan* tp) {
    const int job = job_windows > B ? job_windows : B;
    const int u = h->unshuffle();
    if (th % u || tw % u) return fail(h, S2SR_E_INVALID, "a scale-2 handle (pixel_unshuffle by 2) needs even tile sizes");
    th /= u; tw /= u;                                   // the trunk grid from here on
    Mosaic plan = u8 ? pick_mosaic_cfg(h->mosaic_on, job, th, tw) : Mosaic();
    const int per = plan.on() ? plan.kx * plan.ky : 1;
    int skx = plan.kx, sky = plan.ky;
    if (plan.on()) {
        if (B / per && B % per) return fail(h, S2SR_E_INVALID, "batch spans two mosaic segments (full mosaics and a remainder)");
        if (B < per) mosaic_remainder(B, plan.kx, plan.ky, &skx, &sky);
    }
    const int sper = plan.on() ? skx * sky : 1;
    tp->plan = plan; tp->skx = skx; tp->sky = sky;
    tp->NI = (B + sper - 1) / sper;
    tp->IH = plan.on() ? plan.ky * (th + 1) - 1 : th; tp->IW = plan.on() ? plan.kx * (tw + 1) - 1 : tw;
    tp->SH = plan.on() ? sky * (th + 1) - 1 : th; tp->SW = plan.on() ? skx * (tw + 1) - 1 : tw;
    if (tp->NI > group_size(h, (job + per - 1) / per, tp->IH, tp->IW)) return fail(h, S2SR_E_INVALID, "batch needs more than one launch group");
    return S2SR_OK;
}
// ... and the run: forward_dev -> run_net eagerly (graphs off for the call) on buffers of its own, outputs copied back
int tap_forward(s2sr_handle* h, const uint8_t* tiles, const float* x, int32_t B, int32_t th, int32_t tw, const TapPlan& tp,
                uint8_t* out_u8, float* out_f32) {
    hipStream_t st = h->stream;
    const size_t ib = tiles ? (size_t)B * th * tw * 3 : (size_t)B * 3 * th * tw * 4, opx = (size_t)B * h->cfg.scale * h->cfg.scale * th * tw;
    DevBuf d_in, d_o8, d_o32;
    HIPCHK(h, dev_malloc(&d_in.p, ib));
    HIPCHK(h, dev_malloc(&d_o8.p, opx * 3));
    HIPCHK(h, dev_malloc(&d_o32.p, opx * 3 * 4));
    HIPCHK(h, hipMemcpyAsync(d_in.p, tiles ? (const void*)tiles : (const void*)x, ib, hipMemcpyHostToDevice, st));
    const bool graphs = h->graphs_on;
    h->graphs_on = false;
    Mosaic plan = tp.plan;
    int rc = forward_dev(h, st, tiles ? (const uint8_t*)d_in.p : nullptr, tiles ? nullptr : (const float*)d_in.p, B, th, tw,
                         out_u8 ? (uint8_t*)d_o8.p : nullptr, out_f32 ? (float*)d_o32.p : nullptr, plan.on() ? &plan : nullptr);
    h->graphs_on = graphs;
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(st));
    if (h->ws.G < tp.NI) return fail(h, S2SR_E_INVALID, "workspace fell back to a smaller launch group: the batch ran in two");
    if (out_u8) HIPCHK(h, copy_blocking(h, out_u8, d_o8.p, opx * 3, hipMemcpyDeviceToHost));
    if (out_f32) HIPCHK(h, copy_blocking(h, out_f32, d_o32.p, opx * 3 * 4, hipMemcpyDeviceToHost));
    return S2SR_OK;
}
}  // namespace

// The tail's per-layer parity hook: one batch through forward_dev -> run_net as production runs it (eagerly: graphs off for the
// call), then the tensors of the six head / tail convs copied out of the workspace and decoded on the host.
int s2sr_debug_forward_taps(s2sr_handle* h, const uint8_t* tiles, const float* x, int32_t B, int32_t th, int32_t tw, int32_t job_windows,
                            s2sr_debug_taps* t) {
    if (!h || !t || (!tiles == !x) || B <= 0 || th <= 0 || tw <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->compact()) return fail(h, S2SR_E_INVALID, "s2sr_debug_forward_taps: RRDB handles only (compact: s2sr_debug_compact_taps)");
    if (!h->has_weights) return fail(h, S2SR_E_NOWEIGHTS, "s2sr_load_weights has not been called");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    TapPlan tp;
    int rc = tap_plan(h, tiles != nullptr, B, th, tw, job_windows, &tp);
    if (rc) return rc;
    const int NI = tp.NI;
    const bool fp8 = h->cfg.precision == S2SR_PREC_FP8;
    const bool hp = h->cfg.precision == S2SR_PREC_F16_HP || (fp8 && h->fp8_hp_tail);
    t->n = NI;
    for (int k = 0; k < 3; ++k) {
        const int s = k == 0 ? 1 : 2 * k;
        t->H[k] = s * tp.SH; t->W[k] = s * tp.SW; t->Hp[k] = padded(s * tp.IH); t->Wp[k] = padded(s * tp.IW);
    }
    const bool mos = tp.plan.on();
    t->mos_kx = mos ? tp.skx : 0; t->mos_ky = mos ? tp.sky : 0; t->mos_wh = mos ? tp.plan.wh : 0; t->mos_ww = mos ? tp.plan.ww : 0;
    t->mos_count = mos ? B : 0;
    t->trunk_lo_exp = fp8 ? -1 : h->lo_exp;
    t->avail = 0;
    for (int k = 0; k < S2SR_TAP_COUNT; ++k)
        if (hp || (k != S2SR_TAP_T8 && k < S2SR_TAP_U0LO)) t->avail |= 1 << k;
    bool any = t->out_f32 || t->out_u8;
    for (int k = 0; k < S2SR_TAP_COUNT; ++k) any = any || t->tap[k];
    if (!any) return S2SR_OK;
    if ((rc = tap_forward(h, tiles, x, B, th, tw, tp, t->out_u8, t->out_f32))) return rc;
    const Workspace& w = h->ws;
    // ---- decoders: NI images of `nb` planes of 32 B per pixel at `img` bytes apart -> [n][channels][Hp][Wp] fp32
    std::vector<uint8_t> buf;
    auto blk_at = [&](int k) { return k == 0 ? w.blk1 : k == 1 ? w.blk2 : w.blk4; };
    auto f16_planes = [&](float* dst, const char* src, uint64_t img, int nb, int k) { return decode_f16_planes(h, dst, src, img, NI, nb, blk_at(k)); };
    auto e4m3_planes = [&](float* dst, const char* src, uint64_t img, int nb, int k, const float* scale /*[nb]*/) {   // 32 ch per plane
        return decode_e4m3_planes(h, dst, src, img, NI, nb, blk_at(k), scale);
    };
    const float s_lo4[4] = {1.0f / 2048.0f, 1.0f / 2048.0f, 1.0f, 1.0f};
    const int nb1 = 1;
    if (t->tap[S2SR_TAP_P0] && (rc = f16_planes(t->tap[S2SR_TAP_P0], w.P0, w.blk1, nb1, 0))) return rc;
    if (t->tap[S2SR_TAP_F]) {   // fp32 blocked-8: [n][8][Hp][Wp][8]
        const size_t np = w.blk1 / 32;
        if ((rc = fetch_planes(h, buf, (const char*)w.F, 8 * w.blk1, NI, 8, w.blk1))) return rc;
        const float* v = (const float*)buf.data();
        for (int i = 0; i < NI; ++i)
            for (int b = 0; b < 8; ++b)
                for (size_t q = 0; q < np; ++q)
                    for (int c = 0; c < 8; ++c) t->tap[S2SR_TAP_F][(((size_t)i * 64 + b * 8 + c) * np) + q] = v[(((size_t)i * 8 + b) * np + q) * 8 + c];
    }
    const auto& tr = h->trunk_rec;
    if (t->tap[S2SR_TAP_TRUNK_HI] && (rc = f16_planes(t->tap[S2SR_TAP_TRUNK_HI], tr.hi, tr.hi_img, 4, 0))) return rc;
    if (t->tap[S2SR_TAP_TRUNK_LO]) {
        if (tr.lo_exp >= 0) {
            const float s = ldexpf(1.0f, -tr.lo_exp), sc[2] = {s, s};
            if ((rc = e4m3_planes(t->tap[S2SR_TAP_TRUNK_LO], tr.lo, tr.lo_img, 2, 0, sc))) return rc;
        } else if ((rc = f16_planes(t->tap[S2SR_TAP_TRUNK_LO], tr.lo, tr.lo_img, 4, 0))) return rc;
    }
    if (hp && t->tap[S2SR_TAP_T8] && (rc = e4m3_planes(t->tap[S2SR_TAP_T8], w.T8, 4 * w.blk1, 4, 0, s_lo4))) return rc;
    const char* U[4] = {w.U0, w.U1, w.U2, w.U3};
    const char* UL[4] = {w.U0lo, w.U1lo, w.U2lo, w.U3lo};
    const int Uk[4] = {0, 1, 2, 2};
    const size_t Ublk[4] = {w.blk1, w.blk2, w.blk4, w.blk4};
    for (int u = 0; u < 4; ++u) {
        if (t->tap[S2SR_TAP_U0 + u] && (rc = f16_planes(t->tap[S2SR_TAP_U0 + u], U[u], 4 * Ublk[u], 4, Uk[u]))) return rc;
        if (hp && t->tap[S2SR_TAP_U0LO + u] && (rc = e4m3_planes(t->tap[S2SR_TAP_U0LO + u], UL[u], 4 * Ublk[u], 4, Uk[u], s_lo4))) return rc;
    }
    return S2SR_OK;
}

// The trunk's per-RDB parity hook: the batch of s2sr_debug_forward_taps, with run_net copying the trunk fields of the RDBs
// [first, first + count) out at every RDB boundary (trunk_tap) and the conv launches recording their kernel forms.
int s2sr_debug_trunk_taps(s2sr_handle* h, const uint8_t* tiles, const float* x, int32_t B, int32_t th, int32_t tw, int32_t job_windows,
                          s2sr_debug_trunk_fields* t) {
    if (!h || !t || (!tiles == !x) || B <= 0 || th <= 0 || tw <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->compact()) return fail(h, S2SR_E_INVALID, "s2sr_debug_trunk_taps: RRDB handles only (compact: s2sr_debug_compact_taps)");
    if (!h->has_weights) return fail(h, S2SR_E_NOWEIGHTS, "s2sr_load_weights has not been called");
    if (h->cfg.scale != 4) return fail(h, S2SR_E_INVALID, "trunk taps: scale-4 handles only (the scale-2 trunk is the same schedule on the half grid)");
    if (t->first < 0 || t->count < 1 || t->first + t->count > 3 * h->cfg.num_block)
        return fail(h, S2SR_E_INVALID, "RDB range outside [0, 3 * num_block)");
    const bool fp8 = h->cfg.precision == S2SR_PREC_FP8;
    if (h->d_calib) return fail(h, S2SR_E_INVALID, "trunk taps: the handle is calibrating");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    TapPlan tp;
    int rc = tap_plan(h, tiles != nullptr, B, th, tw, job_windows, &tp);
    if (rc) return rc;
    const bool mos = tp.plan.on();
    t->n = tp.NI; t->H = tp.SH; t->W = tp.SW; t->Hp = padded(tp.IH); t->Wp = padded(tp.IW);
    t->mos_kx = mos ? tp.skx : 0; t->mos_ky = mos ? tp.sky : 0; t->mos_wh = mos ? th : 0; t->mos_ww = mos ? tw : 0;
    t->mos_count = mos ? B : 0;
    t->fp8 = fp8 ? 1 : 0;
    t->lo_exp = fp8 ? -1 : h->lo_exp;
    t->x_exp = fp8 ? h->fp8_x_exp : -1;
    t->g_exp = fp8 ? h->fp8_g_exp : -1;
    if (!(t->x_hi || t->x_lo || t->growth || t->skip_hi || t->skip_lo || t->entry_lo || t->form || t->out_f32 || t->out_u8)) return S2SR_OK;
    if (t->form) memset(t->form, 0, sizeof(*t->form) * 5 * (size_t)t->count);
    TrunkTap tt;
    tt.first = t->first; tt.count = t->count; tt.t = t;
    h->ttap = &tt;
    rc = tap_forward(h, tiles, x, B, th, tw, tp, t->out_u8, t->out_f32);
    h->ttap = nullptr;
    return rc;
}

// SRVGGNetCompact's per-layer parity hook: the batch of s2sr_debug_forward_taps, with run_net_compact copying the chosen layers'
// fp16 activations out right behind their launches.
int s2sr_debug_compact_taps(s2sr_handle* h, const uint8_t* tiles, const float* x, int32_t B, int32_t th, int32_t tw, int32_t job_windows,
                            s2sr_debug_compact_fields* t) {
    if (!h || !t || (!tiles == !x) || B <= 0 || th <= 0 || tw <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->compact()) return fail(h, S2SR_E_INVALID, "s2sr_debug_compact_taps: compact handles only");
    if (!h->has_weights) return fail(h, S2SR_E_NOWEIGHTS, "s2sr_load_weights has not been called");
    if (t->nlayers < 0 || t->nlayers > S2SR_COMPACT_TAPS_MAX) return fail(h, S2SR_E_INVALID, "too many layers");
    for (int k = 0; k < t->nlayers; ++k)
        if (t->layers[k] < 0 || t->layers[k] > h->cfg.num_block || (k > 0 && t->layers[k] <= t->layers[k - 1]))
            return fail(h, S2SR_E_INVALID, "layers must ascend inside [0, num_conv]");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    TapPlan tp;
    int rc = tap_plan(h, tiles != nullptr, B, th, tw, job_windows, &tp);
    if (rc) return rc;
    const bool mos = tp.plan.on();
    t->n = tp.NI; t->H = tp.SH; t->W = tp.SW; t->Hp = padded(tp.IH); t->Wp = padded(tp.IW);
    t->mos_kx = mos ? tp.skx : 0; t->mos_ky = mos ? tp.sky : 0; t->mos_wh = mos ? th : 0; t->mos_ww = mos ? tw : 0;
    t->mos_count = mos ? B : 0;
    bool any = t->out_f32 || t->out_u8 || t->p0;
    for (int k = 0; k < t->nlayers; ++k) any = any || t->act[k];
    if (!any) return S2SR_OK;
    CompactTap ct;
    ct.t = t;
    h->ctap = &ct;
    rc = tap_forward(h, tiles, x, B, th, tw, tp, t->out_u8, t->out_f32);
    h->ctap = nullptr;
    if (rc) return rc;
    if (t->p0 && (rc = decode_f16_planes(h, t->p0, h->ws.P0, h->ws.blk1, tp.NI, 1, h->ws.blk1))) return rc;
    return S2SR_OK;
}

}  // extern "C"
