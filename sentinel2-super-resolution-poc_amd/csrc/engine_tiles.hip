// libs2sr engine, the XYZ tile pyramid: the reprojection warp, the base and overview levels (averaged, or resampled through tap
// tables) and the driver of the device PNG writer (pngdev.hip).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "png_internal.h"
#include "resample_tables.h"

using namespace s2sr;
using namespace s2sr::engine;

extern "C" {

// ---- XYZ tile pyramid (host buffers in and out; geometry tables come from the caller) ---------------
int s2sr_warp_bilinear_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W, const float* grid, int32_t gh, int32_t gw,
                          int32_t step, int32_t OH, int32_t OW, uint8_t* out_rgba) {
    if (!h || !rgb || !grid || !out_rgba || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || gh <= 0 || gw <= 0) return S2SR_E_INVALID;
    if (step <= 0 || (step & (step - 1))) return fail(h, S2SR_E_INVALID, "warp node spacing must be a power of two");
    if ((int64_t)(gh - 1) * step < OH - 1 || (int64_t)(gw - 1) * step < OW - 1)
        return fail(h, S2SR_E_INVALID, "warp node grid does not cover the output raster");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    const size_t ib = (size_t)H * W * 3, gb = (size_t)gh * gw * 8, ob = (size_t)OH * OW * 4;
    int rc;
    if ((rc = ensure_scratch(h, {{SL_SRC, ib}, {SL_DST, ob}, {SL_TABLES, gb}}))) return rc;
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_SRC), rgb, ib, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_TABLES), grid, gb, hipMemcpyHostToDevice, st));
    {
        Scope sc(h, st, F_MISC, 0.0, (double)ob + (double)OH * OW * 12.0);
        HIPCHK(h, launch_warp_bilinear(scratch<const uint8_t>(h, SL_SRC), H, W, scratch<const float>(h, SL_TABLES), gh, gw, step, OH, OW,
                                       scratch<uint8_t>(h, SL_DST), st));
    }
    HIPCHK(h, hipMemcpyAsync(out_rgba, scratch(h, SL_DST), ob, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->scratch.keep(KEPT_RASTER, SL_DST, OH, OW);          // the raster also stays on the device for the base level of its pyramid
    return S2SR_OK;
}

// The warp with a validity mask: the same call, the mask [ceil(H / vs)][ceil(W / vs)] uploaded whole into SL_VALID.
int s2sr_warp_bilinear_masked_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* valid, int32_t valid_scale,
                                 const float* grid, int32_t gh, int32_t gw, int32_t step, int32_t OH, int32_t OW, uint8_t* out_rgba) {
    if (!h || !rgb || !grid || !out_rgba || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || gh <= 0 || gw <= 0) return S2SR_E_INVALID;
    if (!valid) return fail(h, S2SR_E_INVALID, "masked warp: valid is NULL (s2sr_warp_bilinear_u8 is the call without a mask)");
    if (valid_scale < 1) return fail(h, S2SR_E_INVALID, "masked warp: valid_scale must be at least 1");
    if (step <= 0 || (step & (step - 1))) return fail(h, S2SR_E_INVALID, "warp node spacing must be a power of two");
    if ((int64_t)(gh - 1) * step < OH - 1 || (int64_t)(gw - 1) * step < OW - 1)
        return fail(h, S2SR_E_INVALID, "warp node grid does not cover the output raster");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    const int vs = valid_scale;
    const size_t ib = (size_t)H * W * 3, gb = (size_t)gh * gw * 8, ob = (size_t)OH * OW * 4;
    const size_t vb = (size_t)((H + vs - 1) / vs) * (size_t)((W + vs - 1) / vs);
    int rc;
    if ((rc = ensure_scratch(h, {{SL_SRC, ib}, {SL_DST, ob}, {SL_TABLES, gb}, {SL_VALID, vb}}))) return rc;
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_SRC), rgb, ib, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_TABLES), grid, gb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_VALID), valid, vb, hipMemcpyHostToDevice, st));
    {
        Scope sc(h, st, F_MISC, 0.0, (double)ob + (double)OH * OW * 12.0);
        HIPCHK(h, launch_warp_bilinear_masked(scratch<const uint8_t>(h, SL_SRC), H, W, scratch<const uint8_t>(h, SL_VALID), vs,
                                              scratch<const float>(h, SL_TABLES), gh, gw, step, OH, OW, scratch<uint8_t>(h, SL_DST), st));
    }
    HIPCHK(h, hipMemcpyAsync(out_rgba, scratch(h, SL_DST), ob, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->scratch.keep(KEPT_RASTER, SL_DST, OH, OW);          // as the plain call: the raster stays for the base level of its pyramid
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
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    const size_t ib = (size_t)H * W * 4, ob = (size_t)nx * ny * 65536 * 4, cb = (size_t)nx * 256 * 4, rb = (size_t)ny * 256 * 4;
    // rgba == NULL: the raster is the one the previous call on this handle -- s2sr_warp_bilinear_u8 -- produced, taken from its
    // device copy (a 4096 x 4096 source: 67 MB that would cross PCIe twice between the two calls)
    KeptInput in(h);
    if (!rgba && !in.take(KEPT_RASTER, H, W))
        return fail(h, S2SR_E_INVALID, "rgba == NULL, but the previous call on this handle did not leave a warped raster of this size on the device");
    const Slot out_slot = other(in.slot);
    int rc;
    if ((rc = ensure_scratch(h, {{in.slot, ib, rgba != nullptr}, {out_slot, ob}, {SL_TABLES, 2 * cb + 2 * rb}}))) return rc;
    int32_t* t = scratch<int32_t>(h, SL_TABLES);
    if (rgba) HIPCHK(h, hipMemcpyAsync(scratch(h, in.slot), rgba, ib, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(t, col_lo, cb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(t + nx * 256, col_hi, cb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(t + 2 * nx * 256, row_lo, rb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(t + 2 * nx * 256 + ny * 256, row_hi, rb, hipMemcpyHostToDevice, st));
    {
        Scope sc(h, st, F_MISC, 0.0, (double)ib + (double)ob);
        HIPCHK(h, launch_tiles_base(scratch<const uint8_t>(h, in.slot), W, t, t + nx * 256, t + 2 * nx * 256, t + 2 * nx * 256 + ny * 256, nx,
                                    ny, scratch<uint8_t>(h, out_slot), st));
    }
    if (out) HIPCHK(h, hipMemcpyAsync(out, scratch(h, out_slot), ob, hipMemcpyDeviceToHost, st));      // out == NULL: the level stays on the device
    HIPCHK(h, hipStreamSynchronize(st));
    h->scratch.keep(KEPT_LEVEL, out_slot, nx, ny);
    return S2SR_OK;
}

int s2sr_tiles_overview_u8(s2sr_handle* h, const uint8_t* child, int32_t cnx, int32_t cny, int32_t ox, int32_t oy, int32_t pnx,
                           int32_t pny, uint8_t* out) {
    if (!h || cnx <= 0 || cny <= 0 || pnx <= 0 || pny <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    const size_t ib = (size_t)cnx * cny * 65536 * 4, ob = (size_t)pnx * pny * 65536 * 4;
    // child == NULL: the children are the level the previous pyramid call on this handle produced, still on the device (a
    // z18 level is 2.9 GB: sending it back costs as much as fetching it did)
    KeptInput in(h);
    if (!child && !in.take(KEPT_LEVEL, cnx, cny))
        return fail(h, S2SR_E_INVALID, "child == NULL, but the previous call on this handle did not leave a tile level of this size on the device");
    const Slot out_slot = other(in.slot);
    int rc;
    if ((rc = ensure_scratch(h, {{in.slot, ib, child != nullptr}, {out_slot, ob}}))) return rc;
    if (child) HIPCHK(h, hipMemcpyAsync(scratch(h, in.slot), child, ib, hipMemcpyHostToDevice, st));
    {
        Scope sc(h, st, F_MISC, 0.0, (double)ib + (double)ob);
        HIPCHK(h, launch_tiles_overview(scratch<const uint8_t>(h, in.slot), cnx, cny, ox, oy, pnx, pny, scratch<uint8_t>(h, out_slot), st));
    }
    if (out) HIPCHK(h, hipMemcpyAsync(out, scratch(h, out_slot), ob, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->scratch.keep(KEPT_LEVEL, out_slot, pnx, pny);
    return S2SR_OK;
}

// A level resampled through tap tables (resample.hip): the deepest one from a raster, a shallower one from the level below it.
// Same protocol as the two calls above (enum Slot); the 8-bit intermediate between the passes lives in SL_MID.
int s2sr_tiles_resample_u8(s2sr_handle* h, const uint8_t* src, int32_t src_kind, int32_t sa, int32_t sb, const int32_t* col_first,
                           const int32_t* col_count, const int32_t* col_coef, int32_t Kx, const int32_t* row_first,
                           const int32_t* row_count, const int32_t* row_coef, int32_t Ky, int32_t nx, int32_t ny, uint8_t* out) {
    if (!h) return S2SR_E_INVALID;
    if (!col_first || !col_count || !col_coef || !row_first || !row_count || !row_coef || sa <= 0 || sb <= 0 || nx <= 0 || ny <= 0 ||
        nx > (1 << 15) || ny > (1 << 15))
        return fail(h, S2SR_E_INVALID, "resample: a table is missing or a size is not positive");
    if (src_kind != S2SR_TILES_SRC_RASTER && src_kind != S2SR_TILES_SRC_LEVEL)
        return fail(h, S2SR_E_INVALID, "resample: src_kind is neither S2SR_TILES_SRC_RASTER nor S2SR_TILES_SRC_LEVEL");
    const bool level = src_kind == S2SR_TILES_SRC_LEVEL;
    if (level && (sa > (1 << 15) || sb > (1 << 15))) return fail(h, S2SR_E_INVALID, "resample: the source level is too large");
    const int64_t MW = (int64_t)nx * 256, MH = (int64_t)ny * 256;
    const int64_t src_w = level ? (int64_t)sb * 256 : sb, src_h = level ? (int64_t)sa * 256 : sa;
    int32_t c_lo, c_hi, r_lo, r_hi;
    if (const char* why = resample_check_axis(col_first, col_count, col_coef, MW, Kx, src_w, &c_lo, &c_hi)) {
        std::string m = std::string("resample, column tables: ") + why;
        return fail(h, S2SR_E_INVALID, m.c_str());
    }
    if (const char* why = resample_check_axis(row_first, row_count, row_coef, MH, Ky, src_h, &r_lo, &r_hi)) {
        std::string m = std::string("resample, row tables: ") + why;
        return fail(h, S2SR_E_INVALID, m.c_str());
    }
    std::lock_guard<std::mutex> lk(h->mu);
    // src == NULL: the source is what the previous call on this handle left on the device -- the raster of s2sr_warp_bilinear_u8,
    // or the level of a base / overview / resample call
    KeptInput in(h);
    if (!src && !level && !in.take(KEPT_RASTER, sa, sb))
        return fail(h, S2SR_E_INVALID, "src == NULL, but the previous call on this handle did not leave a warped raster of this size on the device");
    if (!src && level && !in.take(KEPT_LEVEL, sb, sa))
        return fail(h, S2SR_E_INVALID, "src == NULL, but the previous call on this handle did not leave a tile level of this size on the device");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    const Slot out_slot = other(in.slot);
    const int nrows = r_hi - r_lo;                                  // the source rows some output row reads
    const size_t ib = (size_t)src_h * src_w * 4, ob = (size_t)MW * MH * 4, mb = (size_t)MW * (nrows > 0 ? nrows : 1) * 4;
    const size_t cw = (size_t)MW * (2 + Kx), rw = (size_t)MH * (2 + Ky);
    std::vector<int32_t> tables(cw + rw);                           // [col first | count | coef Kx x MW][row first | count | coef Ky x MH]
    resample_pack_axis(col_first, col_count, col_coef, MW, Kx, tables.data());
    resample_pack_axis(row_first, row_count, row_coef, MH, Ky, tables.data() + cw);
    int rc;
    if ((rc = ensure_scratch(h, {{in.slot, ib, src != nullptr}, {out_slot, ob}, {SL_MID, mb}, {SL_TABLES, (cw + rw) * 4}}))) return rc;
    const int32_t* tc = scratch<const int32_t>(h, SL_TABLES);
    const int32_t* tr = tc + cw;
    if (src) HIPCHK(h, hipMemcpyAsync(scratch(h, in.slot), src, ib, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_TABLES), tables.data(), (cw + rw) * 4, hipMemcpyHostToDevice, st));
    {
        Scope sc(h, st, F_MISC, 0.0, (double)nrows * (double)(c_hi - c_lo) * 4.0 + (double)mb);      // algorithmic: each byte once
        HIPCHK(h, launch_resample_h(scratch<const uint8_t>(h, in.slot), level, sb, tc, tc + MW, tc + 2 * MW, nx, r_lo, nrows,
                                    scratch<uint8_t>(h, SL_MID), st));
    }
    {
        Scope sc(h, st, F_MISC, 0.0, (double)mb + (double)ob);
        HIPCHK(h, launch_resample_v(scratch<const uint8_t>(h, SL_MID), r_lo, tr, tr + MH, tr + 2 * MH, nx, ny, scratch<uint8_t>(h, out_slot), st));
    }
    if (out) HIPCHK(h, hipMemcpyAsync(out, scratch(h, out_slot), ob, hipMemcpyDeviceToHost, st));      // out == NULL: the level stays on the device
    HIPCHK(h, hipStreamSynchronize(st));
    h->scratch.keep(KEPT_LEVEL, out_slot, nx, ny);
    return S2SR_OK;
}

// The PNG files of the tile level the previous base / overview call left on the device: token statistics on the device, Huffman
// codes on the host, bit emission on the device, chunk framing + CRC + file writes on host threads (pngdev.hip).  Only the
// compressed streams cross PCIe.
static int tiles_write_png_locked(s2sr_handle* h, int32_t nx, int32_t ny, const char* const* paths, int32_t flags, int32_t* written) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    KeptInput in(h);
    if (!in.take(KEPT_LEVEL, nx, ny))
        return fail(h, S2SR_E_INVALID, "the previous call on this handle did not leave a tile level of this size on the device");
    const uint8_t* d_tiles = scratch<const uint8_t>(h, in.slot);
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
    if ((rc = ensure_scratch(h, {{SL_MID, (size_t)n * tile_stats_b}, {SL_TABLES, png_plan_bytes(n)}}))) return rc;
    // the statistics come back into, and the plans go up from, ONE page-locked block kept on the handle (a z18 level: 40 MB down,
    // 27 MB up; as fresh pageable vectors each crossed PCIe through the runtime's staging and was page-faulted in first)
    const size_t stats_b = up256((size_t)n * tile_stats_b), plan_b = png_plan_bytes(n);
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
        G.d_stats = (uint32_t*)(scratch<char>(h, SL_MID) + (size_t)G.a * tile_stats_b);
        G.stats = (const uint32_t*)((const char*)h->host_arena + (size_t)G.a * tile_stats_b);
        G.d_tables = scratch<uint8_t>(h, SL_TABLES) + png_plan_bytes(G.a);
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
        HIPCHK(h, ev_record(h, G.ev_stats, st, SITE_PNG_STATS));
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
            if (k < batches.size()) HIPCHK(h, ev_record(h, h->stage_ev[k & 1], h->copy_stream, SITE_PNG_BATCH));
            if (k > 0) {
                const Batch& bt = batches[k - 1];
                HIPCHK(h, ev_host_wait(h, h->stage_ev[(k - 1) & 1], SITE_PNG_BATCH));
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
            HIPCHK(h, ev_host_wait(h, G.ev_stats, SITE_PNG_STATS));
            double t1 = now();
            t_wait += t1 - t0;
            G.out_words = png_plan_tiles(G.n, G.stats, G.stats + (size_t)G.n * 512, G.stats + (size_t)G.n * 1024, paths + G.a,
                                         (flags & S2SR_PNG_SKIP_TRANSPARENT) != 0, (flags & S2SR_PNG_HOST_ENCODER) != 0, &G.plan);
            t_plan += now() - t1;
            if (G.plan.failed) { return fail(h, S2SR_E_IO, "planning the tile streams failed (an encoder thread ran out of memory)"); }
            total_words += G.out_words;
            const Slot oslot = png_stream_slot(g);               // the group's stream buffer
            if ((rc = ensure_scratch(h, oslot, (G.out_words + 1) * 4))) return rc;
            uint32_t* d_out = scratch<uint32_t>(h, oslot);
            HIPCHK(h, hipMemcpyAsync(G.d_tables, G.plan.tb, G.plan.upload_bytes, hipMemcpyHostToDevice, st));
            HIPCHK(h, hipMemsetAsync(d_out, 0, (G.out_words + 1) * 4, st));
            {
                Scope sc(h, st, F_MISC, 0.0, (double)G.n * 262144.0 + (double)G.out_words * 4.0);
                const size_t tb_b = (size_t)G.n * 512 * 4, hdr_b = (size_t)G.n * 160 * 4;
                HIPCHK(h, launch_png_tile_emit(d_tiles + (size_t)G.a * 262144, G.n, G.d_tables + tb_b + hdr_b, (const uint32_t*)G.d_tables,
                                               (const uint32_t*)(G.d_tables + tb_b), d_out, row_threads, st));
            }
            HIPCHK(h, ev_record(h, G.ev_emit, st, SITE_PNG_EMIT));
        }
        if (g > 0) {
            Group& P = groups[g - 1];
            double t0 = now();
            HIPCHK(h, ev_host_wait(h, P.ev_emit, SITE_PNG_EMIT));           // the copy stream may read the group's streams
            double t1 = now();
            t_wait += t1 - t0;
            if ((rc = write_group(P, scratch<const uint32_t>(h, png_stream_slot(g - 1))))) return rc;
            t_files += now() - t1;
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    if (timing)
        fprintf(stderr, "[s2sr png] %d tiles in %d group(s) (%zu on the host encoder), %.1f ms: waiting for the device %.1f, Huffman codes %.1f, "
                "streams (%.0f MB) back in batches + files %.1f (of which host-encoded tiles %.1f)\n", n, ngroups, n_host, now() - t_begin, t_wait,
                t_plan, (double)total_words * 4 / 1e6, t_files, t_hostenc);
    h->scratch.keep(KEPT_LEVEL, in.slot, nx, ny);                  // the level is intact
    if (failed.load()) return fail(h, S2SR_E_IO, "a tile file could not be written (or an encoder thread ran out of memory)");
    return S2SR_OK;
}

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

}  // extern "C"
