// libs2sr engine core: handle, weights, workspace planes, profiling events, the hipGraph cache and the layer schedule of
// RRDBNet.forward / RealESRGAN.enhance (reference server/app/cnn_super_resolution.py:140-158, 217-280) on top of the conv kernels
// in conv3x3.hip and conv_trunk.hip.  With engine_aoi.hip (whole images), engine_tiles.hip (the XYZ pyramid) and engine_debug.hip
// (test and diagnostic hooks) this is the C ABI of include/s2sr.h.  There is no CPU fallback anywhere in this library.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

std::recursive_mutex& s2sr::device_gate() {      // see s2sr_internal.h
    static std::recursive_mutex m;
    return m;
}

// ---- local to this file: weight bookkeeping, the workspace planner, event statistics and the layer schedule
namespace {

thread_local std::string g_create_error;

void free_weights(s2sr_handle* h) {
    for (ConvW& c : h->convs) {
        if (!c.pooled && c.d_wpack) dev_free(c.d_wpack);
        for (int k = 0; k < 2; ++k)
            if (c.d_wphase[k]) dev_free(c.d_wphase[k]);
    }
    if (h->first16.d_wpack) dev_free(h->first16.d_wpack);
    h->first16 = ConvW();
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

int ensure_workspace(s2sr_handle* h, int G, int H, int W, int mos_py = 0, int mos_px = 0) {
    Workspace& w = h->ws;
    const bool fp8 = h->cfg.precision == S2SR_PREC_FP8, hp = h->hp();
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
    auto alloc_zeroed = [&](size_t bytes) -> int {    // both layouts: one allocation, zeroed
        const hipError_t em = dev_malloc(&w.base, bytes);
        if (em != hipSuccess) {                       // leave a clean "no workspace" state: the caller may retry with a smaller group
            (void)hipGetLastError();
            w = Workspace();
            char b[200];
            snprintf(b, sizeof b, "workspace of %.1f GB for %d images of %dx%d: %s", (double)bytes / 1e9, G, H, W, hipGetErrorString(em));
            return fail(h, em == hipErrorOutOfMemory ? S2SR_E_CAPACITY : S2SR_E_HIP, b);
        }
        w.bytes = bytes;
        HIPCHK(h, fill_blocking(h, w.base, 0, w.bytes));   // the zero halos
        ++h->ws_allocs;
        return S2SR_OK;
    };
    // The planes are carved out of the allocation one behind the other.  Red-zone mode (s2sr_internal.h): a zone behind every
    // plane, patterned after the zeroing, so a plane that runs into its neighbour is caught like one that leaves the allocation.
    const size_t rz = g_redzone_bytes.load(std::memory_order_relaxed);
    struct Plane { size_t off, bytes; };
    std::vector<Plane> zoned;
    size_t off = 0;
    auto take = [&](size_t b) {
        size_t o = off;
        off += up256(b);
        if (rz && b) { zoned.push_back({o, b}); off += rz; }
        return o;
    };
    auto zone_planes = [&]() -> int {
        for (const Plane& p : zoned) HIPCHK(h, redzone_add_plane(w.base, w.base + p.off, p.bytes, up256(p.bytes) - p.bytes + rz));
        return S2SR_OK;
    };
    if (h->compact()) {
        // SRVGGNetCompact: the packed input (1 block) and two 64-channel fp16 tensors (D[0], D[1]: 4 blocks each) that the
        // layers ping-pong between -- 288 B per padded LR pixel; everything stays at input resolution
        w.blk1 = (size_t)w.Hp * w.Wp * 32;
        const size_t g = (size_t)G, oP0 = take(g * w.blk1), oA = take(g * 4 * w.blk1), oB = take(g * 4 * w.blk1);
        if (int rc = alloc_zeroed(off)) return rc;
        w.P0 = w.base + oP0; w.D[0] = w.base + oA; w.D[1] = w.base + oB;
        return zone_planes();
    }
    w.Hp2 = padded(2 * H); w.Wp2 = padded(2 * W);
    w.Hp4 = padded(4 * H); w.Wp4 = padded(4 * W);
    w.blk1 = (size_t)w.Hp * w.Wp * 32; w.blk2 = (size_t)w.Hp2 * w.Wp2 * 32; w.blk4 = (size_t)w.Hp4 * w.Wp4 * 32;
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
    if (int rc = alloc_zeroed(off)) return rc;
    w.P0 = w.base + oP0; w.D[0] = w.base + oD0; w.D[1] = w.base + oD1; w.D[2] = w.base + oD2; w.U0 = w.base + oU0;
    w.T = w.base + oT; w.Tr[0] = w.base + oT0; w.Tr[1] = w.base + oT1; w.Tr[2] = w.base + oT2; w.R = (float*)(w.base + oR); w.F = (float*)(w.base + oF);
    w.U1 = w.base + oU1; w.U2 = w.base + oU2; w.U3 = w.base + oU3;
    if (hp) { w.U0lo = w.base + oU0l; w.U1lo = w.base + oU1l; w.U2lo = w.base + oU2l; w.U3lo = w.base + oU3l; w.T8 = w.base + oT8; }
    if (fp8) {
        for (int i = 0; i < 2; ++i) w.D8[i] = w.base + oD8[i];
        for (int i = 0; i < 3; ++i) w.Xh[i] = w.base + oXh[i];
        w.Tz = w.base + oTz;
    }
    return zone_planes();
}

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

// window mosaic: every launch gets the separator geometry at the scale of the coordinates its epilogue works in
void mosaic_at(ConvParams& q, const Mosaic& mo, int scale) {
    if (!mo.on()) return;
    q.mos_py = (mo.wh + 1) * scale; q.mos_ry = mo.wh * scale; q.mos_px = (mo.ww + 1) * scale; q.mos_rx = mo.ww * scale;
    q.mos_my = (uint32_t)(0x100000000ull / (uint32_t)q.mos_py) + 1u; q.mos_mx = (uint32_t)(0x100000000ull / (uint32_t)q.mos_px) + 1u;
    q.mos_kx = mo.kx; q.mos_ky = mo.ky; q.mos_count = mo.count;
}

// The statistics of one launch of a layer: its family, and the nominal FLOPs and algorithmic bytes (every input and output element
// once) over the launch's p.N x p.H x p.W pixels -- output pixels; the up-convs: source pixels of one row-parity launch.
Scope layer_scope(s2sr_handle* h, hipStream_t st, const ConvW& cw, const ConvParams& p) {
    const bool fp8 = h->cfg.precision == S2SR_PREC_FP8;  // the RDB convs on e4m3 planes of 32 channels
    const double px = (double)p.N * p.H * p.W;
    const double out_b = (p.out_u8 ? 1.0 : 0.0) + (p.out_f32 ? 4.0 : 0.0);   // bytes per output sample the caller asked for
    const double io = cw.cin * 2.0 + cw.cout * 2.0;      // fp16 in and out
    const double planes = cw.split ? 128.0 : 0.0;        // hp: the four e4m3 correction planes of a 64-channel tensor (32 B per pixel each)
    const double f8in = 32.0 * cw.seg_len;
    double flops = 2.0 * 9.0 * cw.cin * cw.cout * px, b = 0.0;
    switch (cw.role) {
    case L_FIRST: b = io + 64 * 10.0; break;                                      // + trunk lo, R, F
    case L_RDB14: b = fp8 ? f8in + 32.0 : io; break;
    case L_RDB5: b = fp8 ? f8in + 64.0 + 128.0 + 128.0 : io + 64 * 2.0; break;    // fp8: e4m3 x out, fp16 trunk in + out; fp16: lo read + write
    case L_RDB5_RRDB: b = fp8 ? f8in + 64.0 + 3 * 128.0 : io + 64 * 5.0; break;   // + the RRDB skip: fp16 x; (fp16 hi, e4m3 lo) pair
    case L_BODY: b = io + 2 * planes + 64 * 4.0; break;                           // planes in and out, F
    case L_HR: b = io + planes + (cw.form == CF_HR_SPLIT_NOHI ? 64.0 : planes); break;   // a folded conv_last wants the two x_lo planes only
    case L_LAST: b = cw.cin * 2.0 + 3.0 * out_b + (cw.form == CF_LAST_FOLD ? 64.0 : planes); break;
    // sub-pixel up-convs: the nominal work of the 3x3 form (2*9*cin*cout per OUTPUT pixel; one row parity = half of the four); the
    // source block once (fp16 128 B, + 128 B of planes), two output pixels (both column parities) of 128 B (+ 128 B of planes) each
    case L_UP1: case L_UP2: flops *= 2.0; b = cw.split ? 768.0 : 384.0; break;
    case L_CFIRST: b = 32.0 + 128.0; break;
    case L_CBODY: b = 256.0; break;                                               // 128 B read + 128 B written per pixel
    case L_CLAST: b = 128.0 + 32.0 + 48.0 * out_b; break;
    }
    return Scope(h, st, kRoleFam[cw.role], flops, px * b);
}
int epi_of(Role r) { return r == L_RDB5 ? EPI_RDB5 : r == L_RDB5_RRDB ? EPI_RDB5_RRDB : EPI_LRELU; }   // the trunk launchers' epilogues

// one conv launch of the RRDB nets outside the fp8 trunk and the up-convs
int run_conv(s2sr_handle* h, hipStream_t st, const ConvW& cw, ConvParams p, s2sr_debug_trunk_form* form = nullptr) {   // form: where the RDB convs record their kernel form
    p.wpack = cw.d_wpack; p.bias = cw.d_bias; p.nstage = cw.nstage; p.seg_len = cw.seg_len; p.seg_lo_mask = cw.seg_lo_mask;
    p.fold_lo = cw.form == CF_LAST_FOLD ? 1 : 0;
    p.trash = h->d_trash;
    Scope sc = layer_scope(h, st, cw, p);
    if (form) *form = s2sr_debug_trunk_form{};
    if (cw.form == CF_NONE) {   // the RRDB trunk: conv_trunk.hip
        HIPCHK(h, launch_conv_trunk(p, cw.ct, epi_of(cw.role), st, h->form_switches(), 0, form));
        return S2SR_OK;
    }
    HIPCHK(h, launch_conv(p, cw.form, st, h->form_switches()));
    return S2SR_OK;
}

// conv_up1 / conv_up2: "nearest-2x, then 3x3" as four 2x2-tap convs of the source image, one
// launch per output ROW parity (conv3x3.hip, PH template parameter): 4 MACs per output pixel instead of 9.
// `p` arrives with the tensors (src / src_lo / dst / T and their image strides) and the mosaic; the geometry is set here:
// n images of Hs x Ws SOURCE pixels in planes of sHp x sWp, written to planes of oHp x oWp.
// walk[k]: the patch order of row-parity launch k (ConvParams::dbg).
int run_up_subpixel(s2sr_handle* h, hipStream_t st, const ConvW& cw, ConvParams p, int n, int Hs, int Ws, int sHp, int sWp,
                    int oHp, int oWp, const int (&walk)[2]) {
    p.N = n; p.H = Hs; p.W = Ws; p.sHp = sHp; p.sWp = sWp; p.Hp = oHp; p.Wp = oWp;
    p.bias = cw.d_bias; p.nstage = cw.nstage; p.seg_len = cw.seg_len; p.seg_lo_mask = cw.seg_lo_mask; p.fold_lo = 0;
    p.trash = h->d_trash;
    for (int k = 0; k < 2; ++k) {
        p.wpack = cw.d_wphase[k]; p.dbg = walk[k];
        Scope sc = layer_scope(h, st, cw, p);
        HIPCHK(h, launch_conv_phase(p, k, st, cw.split, h->form_switches()));
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

// SRVGGNetCompact: first conv, num_conv PReLU convs ping-ponging between D[0] and D[1], the last conv with the pixel-shuffle
// tail.  Every launch works at input resolution (the x4 happens in the last conv's stores), on the 8-wave form of conv3x3.hip.
int run_net_compact(s2sr_handle* h, hipStream_t st, int n, int H, int W, float* d_out_f32, uint8_t* d_out_u8, const Mosaic& mo) {
    Workspace& w = h->ws;
    const int nc = h->cfg.num_block;
    if (h->convs.empty()) return fail(h, S2SR_E_NOWEIGHTS, "compact weights are not loaded");
    ConvParams b{};
    b.N = n; b.H = H; b.W = W; b.Hp = w.Hp; b.Wp = w.Wp; b.sHp = w.Hp; b.sWp = w.Wp;
    b.trash = h->d_trash; b.in_scale = 1.0f / 255.0f;
    mosaic_at(b, mo, 1);
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
    int dir = 0;                                              // launch order: see serp_bit (engine_internal.h)
    auto launch = [&](const ConvW& cw, ConvParams p) -> int {
        if ((h->serpentine >> serp_bit(cw.role)) & 1) dir ^= 1;
        p.dbg = dir;
        p.wpack = cw.d_wpack; p.bias = cw.d_bias; p.slope = cw.d_slope; p.nstage = cw.nstage; p.seg_len = cw.seg_len; p.seg_lo_mask = 0;
        Scope sc = layer_scope(h, st, cw, p);
        HIPCHK(h, launch_conv(p, cw.form, st, h->form_switches()));
        return S2SR_OK;
    };
    int rc, cur = 0;
    {   // first conv 3 -> 64 on the exact 0..255 input, x 1/255 in the epilogue
        ConvParams p = b;
        p.src = w.P0; p.src_img = w.blk1; p.dst = w.D[0]; p.dst_img = 4 * w.blk1;
        if ((rc = launch(h->conv(L_CFIRST), p))) return rc;
        if ((rc = tap(0, w.D[0]))) return rc;
    }
    for (int k = 1; k <= nc; ++k) {
        ConvParams p = b;
        p.src = w.D[cur]; p.src_img = 4 * w.blk1; p.dst = w.D[cur ^ 1]; p.dst_img = 4 * w.blk1;
        if ((rc = launch(h->conv(L_CBODY, k - 1), p))) return rc;
        cur ^= 1;
        if ((rc = tap(k, w.D[cur]))) return rc;
    }
    {   // last conv 64 -> 48, pixel_shuffle(4) + nearest-x4 of the input in its stores
        ConvParams p = b;
        p.src = w.D[cur]; p.src_img = 4 * w.blk1;
        p.src_lo = w.P0; p.lo_img = w.blk1;               // the base: this LR pixel's own colour (ConvParams::slope's note)
        p.out_f32 = d_out_f32; p.out_u8 = d_out_u8; p.cout = 3;
        if ((rc = launch(h->conv(L_CLAST), p))) return rc;
    }
    return S2SR_OK;
}

// The layer schedule for `n` images already packed into ws.P0.  Exactly the op order of
// RRDBNet.forward (cnn_super_resolution.py:140-158) with ResidualDenseBlock / RRDB inlined
// (:85-91, :103-107).  The torch.cat of the dense block is "the first k blocks of D[cur]",
// never a copy; conv5 writes the next x into the other dense tensor because neighbouring
// workgroups still read this one's x as halo.
// in: what was packed.  For 16-bit input (TILE_U16) conv_first takes the cin-6 weight set and the range's in_scale.
int run_net(s2sr_handle* h, hipStream_t st, int n, int H, int W, float* d_out_f32, uint8_t* d_out_u8, const Mosaic& mo, const TileIn& in) {
    const bool in16 = in.kind == TILE_U16;
    if (h->compact()) return run_net_compact(h, st, n, H, W, d_out_f32, d_out_u8, mo);
    Workspace& w = h->ws;
    const int nb = h->cfg.num_block;
    ConvParams b{};
    b.N = n; b.H = H; b.W = W; b.Hp = w.Hp; b.Wp = w.Wp; b.sHp = w.Hp; b.sWp = w.Wp;
    b.T = w.T; b.R = w.R; b.F = w.F;
    mosaic_at(b, mo, 1);
    auto rdb_conv = [&](int g, int k) -> const ConvW& { return h->conv(L_RDB14, 5 * g + (k - 1)); };   // conv k (1..5) of global RDB g
    int rc;
    const bool fp8 = w.fp8;
    int dir = 0;                                                  // launch order: the walk of the launch in front, turned where the rule says
    auto walk = [&](int bit) { if ((h->serpentine >> bit) & 1) dir ^= 1; return dir; };
    {   // conv_first: 3 -> 64 (input = one 16-channel block)
        ConvParams p = b;
        p.dbg = walk(serp_bit(L_FIRST));
        p.src = w.P0; p.src_img = w.blk1; p.in_scale = in16 ? 1.0f / (float)(in.hi - in.lo) : 1.0f / 255.0f;
        if (fp8) { p.dst = w.Xh[0]; p.dst_img = 4 * w.blk1; }
        else { p.dst = w.D[0]; p.dst_img = 12 * w.blk1; }
        if ((rc = run_conv(h, st, in16 ? h->first16 : h->conv(L_FIRST), p))) return rc;
    }
    int cur = 0;
    const char* trunk_hi = nullptr;   // fp16 x of the trunk after the body (conv_body's main operand)
    uint64_t trunk_hi_img = 0;
    const char* trunk_lo = nullptr;   // its lo half: fp16 (4 blocks), or e4m3(lo * 2^trunk_lo_exp) planes when trunk_lo_exp >= 0
    int trunk_lo_exp = -1;
    if (fp8) {
        // the trunk on e4m3 operands (conv_trunk.hip, conv_trunk_f8): D8[cur] planes [x(2) | x1 | x2 | x3 | x4]
        const int xe = h->fp8_x_exp, ge = h->fp8_g_exp;
        {
            Scope sc(h, st, F_MISC, 0.0, (double)n * w.Hp * w.Wp * (128.0 + 64.0));
            HIPCHK(h, launch_xh_to_fp8(w.Xh[0], 4 * w.blk1, n, w.Hp, w.Wp, xe, w.D8[0], 6 * w.blk1, st));
        }
        if (h->d_calib)   // s2sr_calibrate_fp8: the trunk behind conv_first is stored at 2^x_exp too (the conversion above)
            HIPCHK(h, launch_absmax_f16(w.Xh[0], (size_t)n * 4 * w.blk1 / 2, h->d_calib, st));
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
                    const ConvW& cw = rdb_conv(3 * blk + r, k);
                    ConvParams p = b;
                    p.src = w.D8[cur]; p.src_img = 6 * w.blk1;
                    p.wpack = cw.d_wpack; p.bias = cw.d_bias; p.wscale = cw.d_wscale;
                    p.nstage = cw.nstage; p.seg_len = cw.seg_len; p.trash = h->d_trash;
                    p.x_exp = xe; p.g_exp = ge; p.xh_img = 4 * w.blk1;
                    p.dbg = walk(serp_bit(cw.role, k));
                    if (k < 5) {
                        p.dst = w.D8[cur] + (size_t)(2 + (k - 1)) * w.blk1; p.dst_img = 6 * w.blk1;
                    } else {
                        p.dst = w.D8[cur ^ 1]; p.dst_img = 6 * w.blk1;
                        p.xh_in = w.Xh[r]; p.xh_out = w.Xh[(r + 1) % 3];
                        if (cw.role == L_RDB5_RRDB) p.xh_skip = w.Xh[0];
                    }
                    Scope sc = layer_scope(h, st, cw, p);
                    HIPCHK(h, launch_conv_trunk_f8(p, cw.ct, epi_of(cw.role), st, 0, fo ? fo + (k - 1) : nullptr));
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
                    p.dbg = walk(serp_bit(L_RDB14, k));
                    p.src = w.D[r]; p.src_img = 12 * w.blk1;
                    p.dst = w.D[r] + (size_t)(4 + 2 * (k - 1)) * w.blk1; p.dst_img = 12 * w.blk1;
                    if ((rc = run_conv(h, st, rdb_conv(3 * blk + r, k), p, fo ? fo + (k - 1) : nullptr))) { span_end(h, st); return rc; }
                }
                span_end(h, st);
                ConvParams p = b;
                p.src = w.D[r]; p.src_img = 12 * w.blk1;
                p.dst = w.D[nx]; p.dst_img = 12 * w.blk1;
                p.xh_in = w.Tr[r]; p.T = w.Tr[nx]; p.lo_exp = h->lo_exp;
                const ConvW& c5 = rdb_conv(3 * blk + r, 5);
                p.dbg = walk(serp_bit(c5.role));
                if (c5.role == L_RDB5_RRDB) { p.xh_skip = w.D[0]; p.xh_img = 12 * w.blk1; p.lo_skip = w.Tr[0]; }
                if ((rc = run_conv(h, st, c5, p, fo ? fo + 4 : nullptr))) return rc;
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
        p.dbg = walk(serp_bit(L_BODY));
        if ((rc = run_conv(h, st, h->conv(L_BODY), p))) return rc;
    }
    {   // conv_up1 on nearest-2x
        ConvParams p{};
        p.N = n; p.H = 2 * H; p.W = 2 * W; p.Hp = w.Hp2; p.Wp = w.Wp2; p.sHp = w.Hp; p.sWp = w.Wp;
        p.src = w.U0; p.src_img = 4 * w.blk1; p.dst = w.U1; p.dst_img = 4 * w.blk2;
        if (hp) { p.src_lo = w.U0lo; p.lo_img = 4 * w.blk1; p.T = w.U1lo; }
        mosaic_at(p, mo, 1);                                         // sub-pixel form: the epilogue walks SOURCE pixels
        const int wk[2] = {walk(serp_bit(L_UP1)), walk(kSerpUpSecond)};
        if ((rc = run_up_subpixel(h, st, h->conv(L_UP1), p, n, H, W, w.Hp, w.Wp, w.Hp2, w.Wp2, wk))) return rc;
    }
    {   // conv_up2 on nearest-2x
        ConvParams p{};
        p.N = n; p.H = 4 * H; p.W = 4 * W; p.Hp = w.Hp4; p.Wp = w.Wp4; p.sHp = w.Hp2; p.sWp = w.Wp2;
        p.src = w.U1; p.src_img = 4 * w.blk2; p.dst = w.U2; p.dst_img = 4 * w.blk4;
        if (hp) { p.src_lo = w.U1lo; p.lo_img = 4 * w.blk2; p.T = w.U2lo; }
        mosaic_at(p, mo, 2);
        const int wk[2] = {walk(serp_bit(L_UP2)), walk(kSerpUpSecond)};
        if ((rc = run_up_subpixel(h, st, h->conv(L_UP2), p, n, 2 * H, 2 * W, w.Hp2, w.Wp2, w.Hp4, w.Wp4, wk))) return rc;
    }
    ConvParams hr{};
    hr.N = n; hr.H = 4 * H; hr.W = 4 * W; hr.Hp = w.Hp4; hr.Wp = w.Wp4; hr.sHp = w.Hp4; hr.sWp = w.Wp4;
    mosaic_at(hr, mo, 4);
    {
        ConvParams p = hr;
        p.src = w.U2; p.src_img = 4 * w.blk4; p.dst = w.U3; p.dst_img = 4 * w.blk4;
        if (hp) { p.src_lo = w.U2lo; p.lo_img = 4 * w.blk4; p.T = w.U3lo; }
        p.dbg = walk(serp_bit(L_HR));
        if ((rc = run_conv(h, st, h->conv(L_HR), p))) return rc;
    }
    {
        ConvParams p = hr;
        p.src = w.U3; p.src_img = 4 * w.blk4; p.out_f32 = d_out_f32; p.out_u8 = d_out_u8; p.cout = 3;
        if (hp) { p.src_lo = w.U3lo; p.lo_img = 4 * w.blk4; }
        p.dbg = walk(serp_bit(L_LAST));
        if ((rc = run_conv(h, st, h->conv(L_LAST), p))) return rc;
    }
    return S2SR_OK;
}

}  // namespace

// ---- what the other engine files use too (declared in engine_internal.h)
namespace s2sr::engine {

// RRDBNet(num_block) at scale 4 or 2 and SRVGGNetCompact(num_feat 64, num_conv = num_block, upscale 4), as their state dicts
// list them (s2sr/weights.py).  No validity rule lives here: s2sr_create and s2sr_expected_blob_floats_cfg say what is supported.
std::vector<Layer> layer_table(int arch, int num_block, int scale) {
    std::vector<Layer> v;
    if (arch == S2SR_ARCH_COMPACT) {
        v.push_back({L_CFIRST, 3, 64, 64});
        for (int k = 0; k < num_block; ++k) v.push_back({L_CBODY, 64, 64, 64});
        v.push_back({L_CLAST, 64, 48, 0});       // 3 colours x 4 x 4 sub-pixels
        return v;
    }
    v.push_back({L_FIRST, scale == 2 ? 12 : 3, 64, 0});   // scale 2 reads the 12 channels of pixel_unshuffle(x, 2)
    for (int b = 0; b < num_block; ++b)
        for (int r = 0; r < 3; ++r) {
            for (int k = 1; k <= 4; ++k) v.push_back({L_RDB14, 64 + (k - 1) * 32, 32, 0});
            v.push_back({r == 2 ? L_RDB5_RRDB : L_RDB5, 64 + 4 * 32, 64, 0});
        }
    for (Role r : {L_BODY, L_UP1, L_UP2, L_HR}) v.push_back({r, 64, 64, 0});
    v.push_back({L_LAST, 64, 3, 0});
    return v;
}
size_t table_floats(const std::vector<Layer>& table) { size_t n = 0; for (const Layer& l : table) n += l.floats(); return n; }

int fail(s2sr_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    else g_create_error = msg;
    return code;
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

// The HIP side of slots::Book::request.  A slot that has to move: the handle's stream drains, the graphs that hold its address go.
static int scratch_alloc(void* ctx, void** p, size_t bytes) {
    s2sr_handle* h = (s2sr_handle*)ctx;
    HIPCHK(h, dev_malloc(p, bytes));
    return S2SR_OK;
}
static int scratch_release(void* ctx, void* p) {
    s2sr_handle* h = (s2sr_handle*)ctx;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_graphs(h);
    HIPCHK(h, dev_free(p));
    return S2SR_OK;
}
int ensure_scratch(s2sr_handle* h, std::initializer_list<Want> wants) {
    const slots::DeviceMem mem{scratch_alloc, scratch_release, h};
    for (const Want& w : wants) {
        if (!w.on) continue;
        const int rc = h->scratch.request(mem, w.slot, w.bytes);
        if (rc == slots::kTakenRegrow) return fail(h, S2SR_E_INVALID, "a scratch request would move the slot this call reads the previous call's result from");
        if (rc) return rc;
    }
    return S2SR_OK;
}

// Blocking copies / fills go through one of the handle's own (non-blocking) streams, never the legacy stream: the runtime refuses
// any legacy-stream operation (hipMemcpy, hipMemset) while ANY stream of the process captures a graph, and it also invalidates
// that capture -- two handles on two threads (the x4 and the anime engine under Starlette's pool) hit exactly that in the r04 soak.
hipError_t copy_blocking(s2sr_handle* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, h->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}
hipError_t copy_rows(s2sr_handle*, void* dst, const void* src, size_t H, size_t row_bytes, size_t rows, hipMemcpyKind kind, hipStream_t st) {
    for (const RowBand b : row_bands(H, rows)) {
        const hipError_t e = hipMemcpyAsync((char*)dst + b.y0 * row_bytes, (const char*)src + b.y0 * row_bytes, b.rows() * row_bytes, kind, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
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

int ensure_group_events(s2sr_handle* h, int n) {   // h->group_done holds at least n events
    while ((int)h->group_done.size() < n) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->group_done.push_back(e);
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
void mosaic_remainder(int rem, int kx, int ky, int* rkx, int* rky) {
    *rky = (rem + kx - 1) / kx;
    if (*rky > ky) *rky = ky;
    *rkx = (*rky == 1) ? rem : kx;
}
static long mosaic_area(int th, int tw, int kx, int ky) {   // 32 x 32 patches of one kx x ky mosaic image
    return (long)(roundup32(mosaic_extent(ky, th)) / 32) * (roundup32(mosaic_extent(kx, tw)) / 32);
}
long mosaic_patches(int B, int th, int tw, int kx, int ky) {   // patches launched for B windows
    const int per = kx * ky, full = B / per, rem = B % per;
    long a = (long)full * mosaic_area(th, tw, kx, ky);
    if (rem) { int rkx, rky; mosaic_remainder(rem, kx, ky, &rkx, &rky); a += mosaic_area(th, tw, rkx, rky); }
    return a;
}
// pure host arithmetic (s2sr_debug_pick_mosaic exposes it to the CPU tests)
Mosaic pick_mosaic_cfg(bool mosaic_on, int B, int th, int tw) {
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
// th x tw: input windows; the mosaic is laid out on the trunk grid (its wh x ww are trunk sizes)
Mosaic pick_mosaic(const s2sr_handle* h, int B, int th, int tw) { return pick_mosaic_cfg(h->mosaic_on, B, th / h->unshuffle(), tw / h->unshuffle()); }
// Windows per launch group of a job of T windows of th x tw (input sizes) that travels under `mo`: what the workspace allows,
// in whole launch images.
int group_windows(const s2sr_handle* h, const Mosaic& mo, int T, int th, int tw) {
    const int u = h->unshuffle(), per = mo.per();
    return group_size(h, (T + per - 1) / per, mo.image_h(th / u), mo.image_w(tw / u)) * per;
}

// Segments of equal image geometry that B windows travel as: the full mosaics, then the remainder as one smaller mosaic (plain
// images: one segment of B one-window images).  Returns how many.
struct Seg { int t0, nwin, kx, ky; };
static int split_segments(const Mosaic& mo, int B, Seg (&segs)[2]) {
    int nseg = 0;
    if (!mo.on()) segs[nseg++] = Seg{0, B, 1, 1};
    else {
        const int per = mo.per(), full = B / per, rem = B % per;
        if (full) segs[nseg++] = Seg{0, full * per, mo.kx, mo.ky};
        if (rem) { Seg r{full * per, rem, 1, 1}; mosaic_remainder(rem, mo.kx, mo.ky, &r.kx, &r.ky); segs[nseg++] = r; }
    }
    return nseg;
}

// The only place a packer is chosen: nt tiles of th x tw of `in` into ws.P0, as the windows of the mosaic mg or (mg off) one per image.
static int pack_group(s2sr_handle* h, hipStream_t st, const TileIn& in, int nt, int th, int tw, const Mosaic& mg) {
    const Workspace& w = h->ws;
    const int u = h->unshuffle();      // 2: pixel_unshuffle(x, 2) folded into the packers
    Scope sc(h, st, F_PACK, 0.0, (double)nt * th * tw * (3.0 + 8.0));   // (scale 2: 32 B per trunk pixel = 8 per input pixel)
    HIPCHK(h, launch_pack_tiles(in, u, 255.0f, nt, th / u, tw / u, mg.on() ? mg.kx : 0, mg.on() ? mg.ky : 0, w.P0, w.Hp, w.Wp, st));
    return S2SR_OK;
}

// One captured group (GraphKey) runs `enqueue` or replays its graph: a first sighting launches directly (and warms the per-kernel
// attributes), a second one captures, a failed capture leaves the entry on direct launches for good; 24 entries, least recently used out.
template <class Enqueue>
static int run_or_replay(s2sr_handle* h, hipStream_t st, const GraphKey& key, Enqueue enqueue) {
    GraphEntry* ge = nullptr;
    // the legacy null stream cannot be captured; profiling wants its events between launches
    if (h->graphs_on && h->prof <= 0 && st != nullptr) {
        for (GraphEntry& g : h->graphs)
            if (g.key == key) { ge = &g; break; }
        if (!ge) {   // first sighting: remember it
            if (h->graphs.size() >= 24) {
                size_t victim = 0;
                for (size_t i = 1; i < h->graphs.size(); ++i)
                    if (h->graphs[i].last_use < h->graphs[victim].last_use) victim = i;
                if (h->graphs[victim].exec) hipGraphExecDestroy(h->graphs[victim].exec);
                h->graphs.erase(h->graphs.begin() + victim);
            }
            GraphEntry g;
            g.key = key;
            g.last_use = ++h->graph_clock;
            h->graphs.push_back(g);
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
            } else {
                ++h->graph_captures;
            }
        }
    }
    if (!ge || !ge->exec) return enqueue();
    ge->last_use = ++h->graph_clock;
    HIPCHK(h, hipGraphLaunch(ge->exec, st));
    ++h->graph_replays;
    return S2SR_OK;
}

// B tiles of th x tw (`in`, device) -> `out`, S = cfg.scale.  At scale 2 th and tw are even and the net runs on the th/2 x tw/2
// trunk grid.
// `plan`: the mosaic chosen for the whole job this call is a part of (a chunk of an AOI, a group of a batch) -- its geometry
// sizes the workspace, so every part of the job runs in the same planes (r03 ADVICE: re-picking the mosaic from each chunk's own
// window count gave a short last chunk another image height, and with it a workspace reallocation, a device synchronise and
// dropped graphs inside the chunk loop, on every call).  nullptr: choose from B.
int forward_dev(s2sr_handle* h, hipStream_t st, TileIn in, int B, int th, int tw, const TileOut& out, const Mosaic* plan) {
    if (!h->has_weights) return fail(h, S2SR_E_NOWEIGHTS, "s2sr_load_weights has not been called");
    if (in.kind == TILE_U16 && (!in.p || !h->first16.d_wpack || in.lo < 0 || in.hi > 65535 || in.lo >= in.hi))
        return fail(h, S2SR_E_INVALID, "16-bit input: an x4 RRDB handle, tiles, and a range 0 <= lo < hi <= 65535");
    if (B <= 0 || th <= 0 || tw <= 0) return fail(h, S2SR_E_INVALID, "bad batch/tile dims");
    const int u = h->unshuffle();
    if (th % u || tw % u) {
        char b[200];
        snprintf(b, sizeof b, "tiles of %d x %d: a scale-2 handle (pixel_unshuffle by 2) needs even tile sizes", th, tw);
        return fail(h, S2SR_E_INVALID, b);
    }
    if (!in.src_h) in.src_h = th;                                  // the rows / columns as stored
    if (!in.src_w) in.src_w = tw;
    const int TH = th / u, TW = tw / u;                            // the trunk grid: what the schedule, workspace and graphs see
    // u8 and u16 tiles may travel as window mosaics; "images" below are then mosaics of per = kx*ky windows
    const Mosaic mo = in.kind == TILE_F32 ? Mosaic() : (plan ? *plan : pick_mosaic(h, B, th, tw));
    const int per = mo.per();
    const int IH = mo.image_h(TH), IW = mo.image_w(TW);            // the plan's image: the workspace geometry
    int G = group_windows(h, mo, plan && plan->count > B ? plan->count : B, th, tw) / per;   // in images
    int rc = ensure_workspace(h, G, IH, IW, mo.on() ? TH + 1 : 0, mo.on() ? TW + 1 : 0);
    while (rc == S2SR_E_CAPACITY && G > 1) {          // the card is shared: fall back to smaller launch groups rather than fail the job
        G = (G + 1) / 2;
        rc = ensure_workspace(h, G, IH, IW, mo.on() ? TH + 1 : 0, mo.on() ? TW + 1 : 0);
    }
    if (rc) return rc;
    const size_t opx = (size_t)16 * TH * TW;          // output pixels per tile: the x4 tail on the trunk grid
    Seg segs[2];
    const int nseg = split_segments(mo, B, segs);
    for (int si = 0; si < nseg; ++si) {
        const Seg& sg = segs[si];
        const int sper = sg.kx * sg.ky;
        const int NI = (sg.nwin + sper - 1) / sper;                                // images of this segment
        const int SH = mo.on() ? mosaic_extent(sg.ky, TH) : TH, SW = mo.on() ? mosaic_extent(sg.kx, TW) : TW;
        for (int g0 = 0; g0 < NI; g0 += G) {
            const int n = (NI - g0 < G) ? (NI - g0) : G;
            const int t0 = sg.t0 + g0 * sper;                                     // first window / tile of this group
            const int nt = (sg.t0 + sg.nwin - t0 < n * sper) ? (sg.t0 + sg.nwin - t0) : n * sper;   // windows / tiles in it
            const TileIn gin = in.from(t0);
            const TileOut gout = out.from((size_t)t0 * 3 * opx);
            Mosaic mg;                                                            // the group's mosaic (off: plain images)
            if (mo.on()) { mg = mo; mg.kx = sg.kx; mg.ky = sg.ky; mg.count = nt; }
            const GraphKey key{n, th, tw, mg.on() ? mg.kx : 0, mg.on() ? mg.ky : 0, mg.on() ? nt : 0, gin, gout, st};
            rc = run_or_replay(h, st, key, [&]() -> int {
                const int prc = pack_group(h, st, gin, nt, th, tw, mg);
                return prc ? prc : run_net(h, st, n, SH, SW, gout.f32, gout.u8, mg, gin);
            });
            if (rc) return rc;
        }
    }
    return S2SR_OK;
}

// what every 16-bit entry refuses before it touches the device: a net it is not built for, or a bad value range
int check_u16(s2sr_handle* h, int lo, int hi) {
    if (h->compact()) return fail(h, S2SR_E_INVALID, "16-bit input is not available on an S2SR_ARCH_COMPACT handle (its tail reads the 8-bit base image from the input plane)");
    if (h->cfg.scale != 4) return fail(h, S2SR_E_INVALID, "16-bit input is not available on a scale-2 handle (24 unshuffled channels need a second input block)");
    if (lo < 0 || hi > 65535 || lo >= hi) {
        char b[160];
        snprintf(b, sizeof b, "16-bit value range [%d, %d]: need 0 <= lo < hi <= 65535", lo, hi);
        return fail(h, S2SR_E_INVALID, b);
    }
    if (!h->has_weights) return fail(h, S2SR_E_NOWEIGHTS, "s2sr_load_weights has not been called");
    return S2SR_OK;
}

}  // namespace s2sr::engine

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
    return table_floats(layer_table(S2SR_ARCH_RRDB, num_block, scale));
}

size_t s2sr_expected_blob_floats(int32_t num_block) { return s2sr_expected_blob_floats_scale(num_block, 4); }

size_t s2sr_expected_blob_floats_cfg(const s2sr_config* cfg) {
    if (!cfg) return 0;
    if (cfg->arch == S2SR_ARCH_COMPACT) {
        if ((cfg->num_block != 16 && cfg->num_block != 32) || cfg->num_feat != 64 || cfg->scale != 4) return 0;
    } else if (cfg->arch != S2SR_ARCH_RRDB || cfg->num_block <= 0 || cfg->num_feat != 64 || cfg->num_grow != 32 || (cfg->scale != 2 && cfg->scale != 4))
        return 0;
    return table_floats(layer_table(cfg->arch, cfg->num_block, cfg->scale));
}

const char* s2sr_last_error(const s2sr_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// S2SR_SERPENTINE: the launch order of a handle (engine_internal.h serp_bit), fixed at creation like the kernel-form switches read in
// s2sr_create.  0: every launch walks front to back; any other number: that turn mask; unset: kSerpentineDefault.  Unlike those
// switches it selects no kernel and changes no byte of any result.
static int launch_order_from_env() {
    const char* g = getenv("S2SR_SERPENTINE");
    return g ? (int)strtol(g, nullptr, 0) : s2sr::engine::kSerpentineDefault;
}

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
    h->serpentine = launch_order_from_env();                 // S2SR_SERPENTINE, read here with the others
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
    if (dev_malloc(&h->d_trash, kTrashBytes) != hipSuccess) {
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
    for_each_device_buffer(h, [](void* p) { if (p) dev_free(p); });
    for (EvRec& r : h->evs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    for (hipEvent_t e : h->ev_pool) hipEventDestroy(e);
    for (hipEvent_t e : h->group_done) hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
        if (h->stage_buf[i]) host_free(h->stage_buf[i]);
        if (h->stage_ev[i]) hipEventDestroy(h->stage_ev[i]);
    }
    if (h->host_arena) host_free(h->host_arena);
    if (h->host_copy_ev) hipEventDestroy(h->host_copy_ev);
    if (h->order_ev) hipEventDestroy(h->order_ev);
    if (h->copy_stream) hipStreamDestroy(h->copy_stream);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

// Weights in, by either door.  `d_blob` is the fp32 blob ON THE DEVICE (the host entry uploads it first).  One walk over the
// layer table, one case per role: the 345 RDB convs are repacked by device kernels straight from the blob (pack.hip) and the RRDB
// nets' biases are gathered on the device; only the six head/tail convs (0.9 MB of the 67 MB) come back to the host, because their
// split-operand / sub-pixel packers are host code.  SRVGGNetCompact (1.2 M parameters) comes to the host layer by layer; its bias
// and slopes stay fp32.  Each case also decides the conv's kernel form (ConvW::form).
static int load_weights_locked(s2sr_handle* h, const float* d_blob, size_t n_floats, hipStream_t st) {
    const std::vector<Layer> table = layer_table(h->cfg.arch, h->cfg.num_block, h->cfg.scale);
    const size_t want = table_floats(table), nconv = table.size();
    const bool compact = h->compact();
    if (n_floats != want) {
        char b[160];
        if (compact) snprintf(b, sizeof b, "weight blob has %zu floats, a compact net of %d convs needs %zu", n_floats, h->cfg.num_block, want);
        else snprintf(b, sizeof b, "weight blob has %zu floats, a %d-block scale-%d net needs %zu", n_floats, h->cfg.num_block, h->cfg.scale, want);
        return fail(h, S2SR_E_BADBLOB, b);
    }
    HIPCHK(h, dev_sync());
    drop_graphs(h);
    free_weights(h);
    h->has_weights = false;
    h->fp8_x_exp = h->fp8_x_exp0; h->fp8_g_exp = h->fp8_g_exp0;     // exponents calibrated for the previous weights do not carry over
    const bool fp8 = h->cfg.precision == S2SR_PREC_FP8, hp = h->hp();
    // ---- plan: blob offsets, pooled sizes, where the schedules find each layer
    std::vector<uint64_t> woff(nconv), boff(nconv), poff(nconv, 0);
    std::vector<int32_t> couts(nconv);
    size_t off = 0, pool_bytes = 0;
    std::fill(h->at, h->at + kRoles, -1);
    for (size_t i = 0; i < nconv; ++i) {
        const Layer& l = table[i];
        woff[i] = off; boff[i] = off + (size_t)l.cin * l.cout * 9; off += l.floats();
        couts[i] = l.cout;
        if (h->at[l.role] < 0) h->at[l.role] = (int)i;
        if (is_rdb(l.role)) {
            poff[i] = pool_bytes;
            pool_bytes += up256(fp8 ? conv_wpack_bytes_f8(l.cin, l.cout) : conv_wpack_bytes(l.cin, l.cout));
        }
    }
    // pool_b, per conv: [64 bias], compact: [64 bias | 64 slopes], built on the host (the last conv's rows are permuted)
    const size_t brow = compact ? 128 : 64;
    std::vector<float> pb(compact ? nconv * brow : 0, 0.f);
    if (pool_bytes) HIPCHK(h, dev_malloc(&h->pool_w, pool_bytes));
    HIPCHK(h, dev_malloc(&h->pool_b, nconv * brow * sizeof(float)));
    if (fp8) HIPCHK(h, dev_malloc(&h->pool_s, nconv * 64 * sizeof(int32_t)));
    if (!compact) {   // biases: one gather kernel
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
    std::vector<float> hl, w2;
    auto upload = [&](void** d) -> int {   // the packed weights in tmp to a device buffer of their own
        HIPCHK(h, dev_malloc(d, tmp.size()));
        HIPCHK(h, copy_blocking(h, *d, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
        return S2SR_OK;
    };
    int rc;
    for (size_t idx = 0; idx < nconv; ++idx) {
        const Layer& l = table[idx];
        ConvW cw;
        cw.role = l.role; cw.cin = l.cin; cw.cout = l.cout; cw.ct = (l.cout + 31) / 32;
        cw.seg_len = (l.cin + 15) / 16; cw.nstage = cw.seg_len; cw.seg_lo_mask = 0;   // plain fp16: one segment
        cw.d_bias = h->pool_b + idx * brow;
        if (!is_rdb(l.role)) {   // a host-packed conv: its layer (weights, bias, slopes) comes to the host
            hl.resize(l.floats());
            HIPCHK(h, hipMemcpyAsync(hl.data(), d_blob + woff[idx], hl.size() * sizeof(float), hipMemcpyDeviceToHost, st));
            HIPCHK(h, hipStreamSynchronize(st));
        }
        switch (l.role) {
        case L_RDB14: case L_RDB5: case L_RDB5_RRDB:   // the trunk: packed on the device, launched by conv_trunk.hip
            cw.pooled = true;
            cw.d_wpack = h->pool_w + poff[idx];
            if (fp8) {
                cw.seg_len = (l.cin + 31) / 32;
                cw.nstage = (cw.seg_len + 1) & ~1;
                cw.d_wscale = h->pool_s + idx * 64;
                HIPCHK(h, launch_pack_trunk_f8(d_blob + woff[idx], l.cin, l.cout, cw.d_wpack, cw.d_wscale, st));
            } else {
                HIPCHK(h, launch_pack_trunk_f16(d_blob + woff[idx], l.cin, l.cout, cw.d_wpack, st));
            }
            break;
        case L_FIRST: {   // its inputs are exact integers: no x_lo; hp: two fp16 segments [w_hi][w_lo] on the same x
            const int nseg = hp ? 2 : 1;
            cw.form = CF_FIRST; cw.nstage = nseg * cw.seg_len;
            tmp.resize(conv_wpack_bytes_seg(l.cin, l.cout, nseg));
            pack_conv_weights(hl.data(), l.cin, l.cout, nseg, tmp.data());
            if ((rc = upload(&cw.d_wpack))) return rc;
            if (l.cin == 3) {
                // the 16-bit door's conv_first: input channels c and c + 3 (d & 255 and d & 0xff00, pack.hip) both meet w[:, c] --
                // same packer, same segments, still one 16-channel stage per segment, the same bias
                w2.resize((size_t)l.cout * 6 * 9);
                for (int co = 0; co < l.cout; ++co)
                    for (int c = 0; c < 6; ++c) memcpy(&w2[((size_t)co * 6 + c) * 9], &hl[((size_t)co * 3 + c % 3) * 9], 9 * sizeof(float));
                ConvW c6 = cw;
                c6.cin = 6; c6.d_wpack = nullptr;
                tmp.resize(conv_wpack_bytes_seg(6, l.cout, nseg));
                pack_conv_weights(w2.data(), 6, l.cout, nseg, tmp.data());
                if ((rc = upload(&c6.d_wpack))) return rc;
                h->first16 = c6;
            }
            break;
        }
        case L_BODY: case L_HR: case L_LAST: {
            // hp, cin 64: x_hi*w_hi on the fp16 MFMA, x_lo*w_hi + x_hi*w_lo as e4m3 planes on the block-scaled fp8 MFMA (twice
            // the rate, half the bytes; 2^-15-relative error on 2^-11-sized terms); body and hr write such planes for their consumer.
            // conv_last has 3 couts of 32, so w_lo rides in the idle couts 8..10 of the fp16 stages and only the x_lo planes come in as
            // e4m3 -- 6 stages instead of 8, 192 instead of 256 B per pixel read, and conv_hr need not write the x_hi planes
            // (S2SR_LAST_FOLD=0: the 8-stage form)
            const bool fold = hp && h->last_fold;
            cw.split = hp;
            if (l.role == L_BODY) cw.form = hp ? CF_BODY_SPLIT : CF_BODY;
            else if (l.role == L_HR) cw.form = !hp ? CF_HR : fold ? CF_HR_SPLIT_NOHI : CF_HR_SPLIT;
            else cw.form = !hp ? CF_LAST : fold ? CF_LAST_FOLD : CF_LAST_SPLIT8;
            if (hp) {
                cw.nstage = cw.form == CF_LAST_FOLD ? cw.seg_len + 2 : 2 * cw.seg_len; cw.seg_lo_mask = 0x2;
                tmp.resize((size_t)cw.nstage * 9 * cw.ct * 1024);
                pack_conv_weights_f8hp(hl.data(), l.cin, l.cout, tmp.data(), cw.form == CF_LAST_FOLD);
            } else {
                tmp.resize(conv_wpack_bytes(l.cin, l.cout));
                pack_conv_weights(hl.data(), l.cin, l.cout, 1, tmp.data());
            }
            if ((rc = upload(&cw.d_wpack))) return rc;
            break;
        }
        case L_UP1: case L_UP2:   // sub-pixel form in every precision: four fp16 stages of 2x2 taps, hp: + their four e4m3 planes
            cw.split = hp;
            cw.seg_len = 4; cw.nstage = hp ? 8 : 4; cw.seg_lo_mask = hp ? 0x2 : 0x0;
            tmp.resize(conv_wpack_bytes_phase(l.cin, l.cout));
            for (int k = 0; k < 2; ++k) {
                pack_conv_weights_phase_f8hp(hl.data(), l.cin, l.cout, k, tmp.data());
                if ((rc = upload(&cw.d_wphase[k]))) return rc;
            }
            break;
        case L_CFIRST: case L_CBODY: case L_CLAST: {   // plain fp16, 64 rows; bias and the PReLU slopes behind it to pool_b
            const float *wsrc = hl.data(), *bsrc = wsrc + (size_t)l.cin * l.cout * 9;
            float* bias = pb.data() + idx * brow;
            cw.form = l.role == L_CFIRST ? CF_CFIRST : l.role == L_CBODY ? CF_PRELU : CF_CLAST;
            cw.d_slope = cw.d_bias + 64;
            if (l.role == L_CLAST) {   // its 48 output channels in the rows the pixel-shuffle epilogue wants, idle rows zero
                w2.assign((size_t)64 * l.cin * 9, 0.f);
                for (int row = 0; row < 64; ++row) {
                    const int ch = compact_last_row_channel(row);
                    if (ch < 0) continue;
                    memcpy(&w2[(size_t)row * l.cin * 9], wsrc + (size_t)ch * l.cin * 9, sizeof(float) * l.cin * 9);
                    bias[row] = bsrc[ch];
                }
                wsrc = w2.data();
            } else {
                memcpy(bias, bsrc, sizeof(float) * (64 + l.extra));   // the slopes follow the bias in the blob as in the pool
            }
            tmp.resize(conv_wpack_bytes(l.cin, 64));
            pack_conv_weights(wsrc, l.cin, 64, 1, tmp.data());
            if ((rc = upload(&cw.d_wpack))) return rc;
            break;
        }
        }
        h->convs.push_back(cw);
    }
    if (compact) HIPCHK(h, copy_blocking(h, h->pool_b, pb.data(), pb.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipStreamSynchronize(st));
    h->has_weights = true;
    return S2SR_OK;
}

int s2sr_load_weights(s2sr_handle* h, const float* blob, size_t n_floats) {
    if (!h || !blob) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n_floats != s2sr_expected_blob_floats_cfg(&h->cfg)) return load_weights_locked(h, nullptr, n_floats, h->stream);   // -> BADBLOB text
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

int s2sr_forward_batch_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t B, int32_t th, int32_t tw, void* d_out,
                              void* stream) {
    if (!h || !d_tiles || !d_out) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;   // NULL = the default stream, as everywhere in HIP
    DOOR_ENTER(h, st);
    return door_leave(h, st, forward_dev(h, st, TileIn::u8(d_tiles), B, th, tw, TileOut{(uint8_t*)d_out}));
}

// A PART of a larger job of `job_windows` equal windows (a chunk of an AOI's windows on one rank, s2sr/dist.py): the window
// mosaic and the workspace are planned for the whole job, so every part runs in the same planes and replays its graphs.
int s2sr_forward_part_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t B, int32_t th, int32_t tw, int32_t job_windows, void* d_out,
                             void* stream) {
    if (!h || !d_tiles || !d_out || job_windows < B) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const Mosaic mo = pick_mosaic(h, job_windows, th, tw);
    hipStream_t st = (hipStream_t)stream;
    DOOR_ENTER(h, st);
    return door_leave(h, st, forward_dev(h, st, TileIn::u8(d_tiles), B, th, tw, TileOut{(uint8_t*)d_out}, mo.on() ? &mo : nullptr));
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
    DOOR_ENTER(h, h->stream);
    const int S = h->cfg.scale;
    const size_t ib = (size_t)B * th * tw * 3, ob = ib * S * S;
    int rc = ensure_scratch(h, {{SL_SRC, ib}, {SL_DST, ob}});
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_SRC), tiles, ib, hipMemcpyHostToDevice, h->stream));
    // Groups are enqueued one by one with an event after each; the device-to-host copy of group g
    // runs on the copy stream while group g+1 computes, so only the last group's copy is exposed.
    // one mosaic plan for the whole batch (ragged tiles): every group runs in the same workspace geometry
    const Mosaic mo = pick_mosaic(h, B, th, tw);
    const int G = group_windows(h, mo, B, th, tw);
    const size_t tin = (size_t)th * tw * 3, tout = tin * S * S;
    const int ngroups = (B + G - 1) / G;
    if ((rc = ensure_group_events(h, ngroups))) return rc;
    for (int g = 0; g < ngroups; ++g) {
        const int g0 = g * G, n = (B - g0 < G) ? (B - g0) : G;
        rc = forward_dev(h, h->stream, TileIn::u8(scratch<const uint8_t>(h, SL_SRC) + g0 * tin), n, th, tw,
                         TileOut{scratch<uint8_t>(h, SL_DST) + g0 * tout}, mo.on() ? &mo : nullptr);
        if (rc) return rc;
        HIPCHK(h, ev_record(h, h->group_done[g], h->stream, SITE_BATCH_GROUP_D2H));
    }
    for (int g = 0; g < ngroups; ++g) {
        const int g0 = g * G, n = (B - g0 < G) ? (B - g0) : G;
        HIPCHK(h, ev_stream_wait(h, h->copy_stream, h->group_done[g], SITE_BATCH_GROUP_D2H));
        if ((rc = d2h_staged(h, out + g0 * tout, scratch<const uint8_t>(h, SL_DST) + g0 * tout, n * tout, g + 1 == ngroups))) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return S2SR_OK;
}

int s2sr_forward_batch_u8(s2sr_handle* h, const uint8_t* tiles, int32_t B, int32_t th, int32_t tw, uint8_t* out) {
    RUN_WITH_STREAM_RECOVERY(h, forward_batch_u8_once(h, tiles, B, th, tw, out));
}

// The 16-bit door on a batch of tiles: the net's fp32 tile output [B,3,4th,4tw] goes to a scratch buffer, the quantiser
// (launch_stitch_quant_u16 in its plain-batch form) turns it into [B,4th,4tw,3] u16.  The caller holds h->mu.
static int forward_u16_locked(s2sr_handle* h, hipStream_t st, const uint16_t* d_tiles, int B, int th, int tw, int lo, int hi,
                              uint16_t* d_out_u16, float* d_f32) {
    int rc = forward_dev(h, st, TileIn::u16(d_tiles, lo, hi), B, th, tw, TileOut{nullptr, d_f32});
    if (rc || !d_out_u16) return rc;
    Scope sc(h, st, F_MISC, 0.0, (double)B * 16.0 * th * tw * 3.0 * (4.0 + 2.0));
    HIPCHK(h, launch_stitch_quant_u16(d_f32, 1, 0, 4 * th, 4 * tw, nullptr, nullptr, B * 4 * th, 4 * tw, lo, hi, d_out_u16, st));
    return S2SR_OK;
}

int s2sr_forward_batch_u16_dev(s2sr_handle* h, const void* d_tiles, int32_t B, int32_t th, int32_t tw, int32_t lo, int32_t hi,
                               void* d_out_u16, void* stream) {
    if (!h || !d_tiles || !d_out_u16 || B <= 0 || th <= 0 || tw <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = check_u16(h, lo, hi);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // the fp32 tiles between the net and the quantiser live in the handle's scratch (SL_DST); work already queued on the caller's
    // stream that reads an earlier call's tiles is ordered before this call's on the same stream, work on another stream by door_enter
    hipStream_t st = (hipStream_t)stream;
    DOOR_ENTER(h, st);
    if ((rc = ensure_scratch(h, SL_DST, (size_t)B * 3 * 16 * th * tw * sizeof(float)))) return rc;
    return door_leave(h, st, forward_u16_locked(h, st, (const uint16_t*)d_tiles, B, th, tw, lo, hi, (uint16_t*)d_out_u16, scratch<float>(h, SL_DST)));
}

static int forward_batch_u16_once(s2sr_handle* h, const uint16_t* tiles, int32_t B, int32_t th, int32_t tw, int32_t lo, int32_t hi,
                                  uint16_t* out_u16, float* out_f32) {
    if (!h || !tiles || (!out_u16 && !out_f32) || B <= 0 || th <= 0 || tw <= 0) {
        if (h) fail(h, S2SR_E_INVALID, "s2sr_forward_batch_u16: tiles, positive sizes and at least one output are required");
        return S2SR_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = check_u16(h, lo, hi);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    const size_t npx = (size_t)B * th * tw * 3, ib = npx * 2, fb = npx * 16 * sizeof(float), qb = npx * 16 * 2;
    if ((rc = ensure_scratch(h, {{SL_SRC, ib}, {SL_DST, fb}, {SL_MID, qb, out_u16 != nullptr}}))) return rc;
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_SRC), tiles, ib, hipMemcpyHostToDevice, h->stream));
    if ((rc = forward_u16_locked(h, h->stream, scratch<const uint16_t>(h, SL_SRC), B, th, tw, lo, hi, out_u16 ? scratch<uint16_t>(h, SL_MID) : nullptr,
                                 scratch<float>(h, SL_DST)))) return rc;
    if ((rc = ensure_group_events(h, 1))) return rc;
    HIPCHK(h, ev_record(h, h->group_done[0], h->stream, SITE_BATCH_U16_D2H));
    HIPCHK(h, ev_stream_wait(h, h->copy_stream, h->group_done[0], SITE_BATCH_U16_D2H));
    if (out_u16 && (rc = d2h_staged(h, (uint8_t*)out_u16, scratch<const uint8_t>(h, SL_MID), qb, true))) return rc;
    if (out_f32 && (rc = d2h_staged(h, (uint8_t*)out_f32, scratch<const uint8_t>(h, SL_DST), fb, true))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return S2SR_OK;
}

int s2sr_forward_batch_u16(s2sr_handle* h, const uint16_t* tiles, int32_t B, int32_t th, int32_t tw, int32_t lo, int32_t hi,
                           uint16_t* out_u16, float* out_f32) {
    RUN_WITH_STREAM_RECOVERY(h, forward_batch_u16_once(h, tiles, B, th, tw, lo, hi, out_u16, out_f32));
}

static int forward_f32_once(s2sr_handle* h, const float* x, int32_t N, int32_t H, int32_t W, float* y) {
    if (!h || !x || !y) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    const size_t ib = (size_t)N * 3 * H * W * 4, ob = ib * h->cfg.scale * h->cfg.scale;
    int rc = ensure_scratch(h, {{SL_SRC, ib}, {SL_DST, ob}});
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_SRC), x, ib, hipMemcpyHostToDevice, h->stream));
    rc = forward_dev(h, h->stream, TileIn::f32(scratch(h, SL_SRC)), N, H, W, TileOut{nullptr, scratch<float>(h, SL_DST)});
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(y, scratch(h, SL_DST), ob, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return S2SR_OK;
}

int s2sr_forward_f32(s2sr_handle* h, const float* x, int32_t N, int32_t H, int32_t W, float* y) {
    RUN_WITH_STREAM_RECOVERY(h, forward_f32_once(h, x, N, H, W, y));
}

int s2sr_set_profiling(s2sr_handle* h, int32_t on) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->prof = on < 0 ? 0 : on;
    h->span_on = false; h->span_count = 0;
    for (int i = 0; i < F_COUNT; ++i) h->fam_count[i] = 0;
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
    DOOR_ENTER(h, h->stream);
    const size_t ib = (size_t)B * th * tw * 3, ob = ib * h->cfg.scale * h->cfg.scale;
    int rc = ensure_scratch(h, {{SL_SRC, ib}, {SL_DST, ob}});
    if (rc) return rc;
    float* d_c = nullptr;
    HIPCHK(h, dev_malloc(&d_c, 2 * sizeof(float)));
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_SRC), tiles, ib, hipMemcpyHostToDevice, h->stream));
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
        rc = forward_dev(h, h->stream, TileIn::u8(scratch(h, SL_SRC)), B, th, tw, TileOut{scratch<uint8_t>(h, SL_DST)});
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

}  // extern "C"
