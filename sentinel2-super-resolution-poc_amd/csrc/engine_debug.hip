// libs2sr engine, the test and diagnostic hooks: every s2sr_debug_* entry of include/s2sr.h -- the planners' arithmetic for the
// CPU tests, single convs, the in-situ taps of the schedule, and the drivers of ceiling.hip and persist.hip.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "band_plan.h"
#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

namespace {

struct DevBuf {   // frees on scope exit: the hooks have many early returns
    void* p = nullptr;
    ~DevBuf() { if (p) dev_free(p); }
};

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
    const int TH = th / u, TW = tw / u;                 // the trunk grid
    Mosaic plan = u8 ? pick_mosaic_cfg(h->mosaic_on, job, TH, TW) : Mosaic();
    const int per = plan.per();
    int skx = plan.kx, sky = plan.ky;
    if (plan.on()) {
        if (B / per && B % per) return fail(h, S2SR_E_INVALID, "batch spans two mosaic segments (full mosaics and a remainder)");
        if (B < per) mosaic_remainder(B, plan.kx, plan.ky, &skx, &sky);
    }
    const int sper = plan.on() ? skx * sky : 1;
    tp->plan = plan; tp->skx = skx; tp->sky = sky;
    tp->NI = (B + sper - 1) / sper;
    tp->IH = plan.image_h(TH); tp->IW = plan.image_w(TW);
    tp->SH = plan.on() ? mosaic_extent(sky, TH) : TH; tp->SW = plan.on() ? mosaic_extent(skx, TW) : TW;
    if (tp->NI > group_windows(h, plan, job, th, tw) / per) return fail(h, S2SR_E_INVALID, "batch needs more than one launch group");
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
    int rc = forward_dev(h, st, tiles ? TileIn::u8(d_in.p) : TileIn::f32(d_in.p), B, th, tw,
                         TileOut{out_u8 ? (uint8_t*)d_o8.p : nullptr, out_f32 ? (float*)d_o32.p : nullptr}, plan.on() ? &plan : nullptr);
    h->graphs_on = graphs;
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(st));
    if (h->ws.G < tp.NI) return fail(h, S2SR_E_INVALID, "workspace fell back to a smaller launch group: the batch ran in two");
    if (out_u8) HIPCHK(h, copy_blocking(h, out_u8, d_o8.p, opx * 3, hipMemcpyDeviceToHost));
    if (out_f32) HIPCHK(h, copy_blocking(h, out_f32, d_o32.p, opx * 3 * 4, hipMemcpyDeviceToHost));
    return S2SR_OK;
}

}  // namespace

extern "C" {

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

int s2sr_debug_plan_windows(int32_t PH, int32_t PW, int32_t tile, int32_t pad, int32_t scale, int32_t tiled, int32_t* dims,
                            int32_t* rects, int32_t cap, int32_t* rm, int32_t* cm) {
    if (!dims || !rects || !rm || !cm || PH <= 0 || PW <= 0 || tile <= 0 || pad < 0 || scale <= 0 || cap < 0) return S2SR_E_INVALID;
    WindowJob job;
    if (int rc = plan_window_job(PH, PW, tile, pad, scale, tiled != 0, job)) return rc;
    dims[0] = job.nx; dims[1] = job.ny; dims[2] = job.wh; dims[3] = job.ww;
    if (job.rects.size() > 4 * (size_t)cap) return S2SR_E_CAPACITY;
    memcpy(rects, job.rects.data(), job.rects.size() * 4);
    memcpy(rm, job.rm.data(), job.rm.size() * 4);
    memcpy(cm, job.cm.data(), job.cm.size() * 4);
    return S2SR_OK;
}

int s2sr_debug_plan_bands(const int32_t* chunk_r0, int32_t nchunks, int32_t ny, int32_t OH, const int32_t* last_row, int32_t* bands) {
    if (!chunk_r0 || !last_row || !bands || nchunks <= 0 || ny <= 0 || OH <= 0 || chunk_r0[0] != 0 || chunk_r0[nchunks] != ny) return S2SR_E_INVALID;
    for (int k = 0; k < nchunks; ++k)
        if (chunk_r0[k] >= chunk_r0[k + 1]) return S2SR_E_INVALID;
    std::vector<int> end(nchunks);
    plan_bands(chunk_r0, nchunks, ny, OH, last_row, 1, end.data());
    for (int k = 0; k < nchunks; ++k) { bands[2 * k] = k ? end[k - 1] : 0; bands[2 * k + 1] = end[k]; }
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
    p.out_f32 = d_y; p.cout = Cout; p.act = act & 0xff; p.trash = h->d_trash;
    p.dbg = (act >> 8) & 1;                                   // bit 8 of `act`: the patches back to front
    const ConvForm form = Cout <= 32 ? (upsample ? CF_DEBUG1_UP : CF_DEBUG1) : (upsample ? CF_DEBUG2_UP : CF_DEBUG2);
    HIPCHK(h, launch_conv(p, form, st, FormSwitches{}));
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
    const size_t sink_bytes = (size_t)ncu * 512 * 4, store_bytes = (size_t)64 << 20;      // mode 5 streams its stores through 64 MB
    int rc = ensure_scratch(h, {{SL_MID, src_bytes}, {SL_TABLES, sink_bytes + store_bytes}});
    if (rc) return rc;
    char* d_store = scratch<char>(h, SL_TABLES) + sink_bytes;
    hipStream_t st = h->stream;
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    HIPCHK(h, launch_mfma_ceiling(mode, scratch<char>(h, SL_MID), src_bytes, true /* fill the operands: 0.1 ms */, scratch<float>(h, SL_TABLES), ncu, stages, d_store,
                                  store_bytes, st));
    for (int i = 0; i < launches / 4; ++i)
        HIPCHK(h, launch_mfma_ceiling(mode, scratch<char>(h, SL_MID), src_bytes, false, scratch<float>(h, SL_TABLES), ncu, stages, d_store, store_bytes, st));
    HIPCHK(h, hipEventRecord(e0, st));
    for (int i = 0; i < launches; ++i)
        HIPCHK(h, launch_mfma_ceiling(mode, scratch<char>(h, SL_MID), src_bytes, false, scratch<float>(h, SL_TABLES), ncu, stages, d_store, store_bytes, st));
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
    int rc = ensure_scratch(h, {{SL_MID, wts_bytes}, {SL_TABLES, sink_bytes + 256}, {SL_CHUNK, ws_bytes}});
    if (rc) return rc;
    struct Uncached {
        void* p = nullptr;
        ~Uncached() { if (p) (void)hipFree(p); }
    } fl;
    const size_t flag_bytes = ((size_t)grid * P + 1) * 4;
    HIPCHK(h, hipExtMallocWithFlags(&fl.p, flag_bytes, hipDeviceMallocUncached));
    uint32_t* d_timeouts = (uint32_t*)(scratch<char>(h, SL_TABLES) + sink_bytes);
    hipStream_t st = h->stream;
    // operand data: the ceiling loops' generator fills the weights buffer and the working set (toggle rates as there)
    HIPCHK(h, launch_mfma_ceiling(0, scratch<char>(h, SL_MID), wts_bytes, true, scratch<float>(h, SL_TABLES), 1, 1, nullptr, 0, st));
    HIPCHK(h, launch_mfma_ceiling(0, scratch<char>(h, SL_CHUNK), ws_bytes, true, scratch<float>(h, SL_TABLES), 1, 1, nullptr, 0, st));
    HIPCHK(h, hipMemsetAsync(d_timeouts, 0, 12, st));
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    auto one = [&]() -> int {
        HIPCHK(h, hipMemsetAsync(fl.p, 0, flag_bytes, st));
        HIPCHK(h, launch_rdb_persistent(variant, scratch<const char>(h, SL_MID), wts_bytes, scratch<char>(h, SL_CHUNK), (uint32_t*)fl.p, scratch<float>(h, SL_TABLES),
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
    // trunk_w4 always 1; trunk_wino, reserved[1] and reserved[3] always 0 (the forms they named were removed); fp8_form's slot: the launch-order mask
    out->precision = h->cfg.precision; out->group = h->cfg.group; out->trunk_w4 = 1; out->lo_exp = h->lo_exp;
    out->fp8_x_exp = h->fp8_x_exp; out->fp8_g_exp = h->fp8_g_exp; out->fp8_hp_tail = h->fp8_hp_tail ? 1 : 0; out->fp8_form = h->serpentine;
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
    const int form = a->form & 0xff;                          // bit 8 of `form`: the patches back to front
    p.dbg = (a->form >> 8) & 1;
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
        const hipError_t e = launch_conv_trunk(p, Cout / 32, epi, st, FormSwitches{}, form);   // the hook names forms; form 0 picks with the default switches
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
        const hipError_t e = launch_conv_trunk_f8(p, Cout / 32, epi, st, form);   // conv1-4: no row answers to a hook number; conv5: one form
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
    const int epi = cout == 32 ? EPI_LRELU : EPI_RDB5, ct = cout / 32;
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return fail(h, S2SR_E_HIP, "hipEventCreate failed"); }
    hipError_t e = hipSuccess;
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = launch_conv_trunk(p, ct, epi, st, h->form_switches());
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch_conv_trunk(p, ct, epi, st, h->form_switches());
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    HIPCHK(h, e);
    *avg_us = ms * 1000.0f / iters;
    return S2SR_OK;
}

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
    const bool hp = h->hp();
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
