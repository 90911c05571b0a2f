// libs2sr engine, touching fields split (kernels: fields_split.hip, and fields.hip for the mask, the components and the
// numbering): a caller's int16 index raster -> uint16 zone labels in which blobs of several parcels are cut apart, the fields table,
// their number and, on request, the distance and core planes.
#include <stdio.h>

#include <mutex>

#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

namespace {

constexpr size_t kBandBytes = (size_t)64 << 20;                  // the rasters come and go in row bands of about this size

int split_impl(s2sr_handle* h, const int16_t* idx, int H, int W, int lo, int hi, int r_open, int r_close, int conn, int64_t min_pixels, int Z,
               const s2sr_fields_split* sp, uint16_t* labels, int64_t* fields, uint64_t* found, uint16_t* dist2, uint8_t* cores) {
    std::lock_guard<std::mutex> lk(h->mu);
    const char* what = "s2sr_fields_split_i16: ";
    if (!idx || !labels) return fail(h, S2SR_E_INVALID, std::string(what) + "idx and labels are required");
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return fail(h, S2SR_E_INVALID, std::string(what) + "H and W must be positive and H W < 2^31");
    if (lo < -32767 || hi > 32767 || lo > hi) return fail(h, S2SR_E_INVALID, std::string(what) + "lo <= hi, both in -32767..32767");
    if (r_open < 0 || r_open > 8 || r_close < 0 || r_close > 8) return fail(h, S2SR_E_INVALID, std::string(what) + "r_open and r_close must be in 0..8");
    if (conn != 4 && conn != 8) return fail(h, S2SR_E_INVALID, std::string(what) + "conn must be 4 or 8");
    if (min_pixels < 1) return fail(h, S2SR_E_INVALID, std::string(what) + "min_pixels must be >= 1");
    if (Z < 1 || Z > 65535) return fail(h, S2SR_E_INVALID, std::string(what) + "Z must be in 1..65535");
    if (sp->core_q < 1 || sp->core_q > 1000) return fail(h, S2SR_E_INVALID, std::string(what) + "core_q must be in 1..1000");
    if (sp->core_px < 0 || sp->core_px > 255) return fail(h, S2SR_E_INVALID, std::string(what) + "core_px must be in 0..255");
    if (sp->edge < 0 || sp->edge > 32767) return fail(h, S2SR_E_INVALID, std::string(what) + "edge must be in 0..32767");
    if (sp->edge_r < 0 || sp->edge_r > 4) return fail(h, S2SR_E_INVALID, std::string(what) + "edge_r must be in 0..4");
    const size_t N = (size_t)H * W, row_i = (size_t)W * 2;
    const uint32_t minpx = min_pixels > 0x80000000LL ? 0x80000000u : (uint32_t)min_pixels;       // beyond H W nothing is a field
    // SL_TABLES: the chunk sums, found, the growth's changed counter and its two planes of tile marks, fields
    const size_t tiles_b = up256(fsplit_tiles(H, W));
    const size_t o_found = up256(fields_chunks(H, W) * 4), o_changed = o_found + 256, o_dirty = o_changed + 256, o_fields = o_dirty + 2 * tiles_b,
                 fields_b = ((size_t)Z + 1) * 6 * 8;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    // 23 bytes per pixel (fields_segment_i16: 14): the distance plane lives where the labels go later, the vertical distances where
    // the cores go later; the growth words are 8 bytes of their own, parents and sizes share SL_CONS
    int rc = ensure_scratch(h, {{SL_SRC, up256(N * 2)}, {SL_DST, up256(N * 2)}, {SL_MID, up256(N)}, {SL_CHUNK, up256(N)}, {SL_VALID, up256(N)},
                                {SL_PP, up256(N * 8)}, {SL_CONS, up256(N * 4) + up256(N * 4)}, {SL_TABLES, o_fields + up256(fields_b)}});
    if (rc) return rc;
    int16_t* d_idx = scratch<int16_t>(h, SL_SRC);
    uint16_t* d_labels = scratch<uint16_t>(h, SL_DST);
    uint16_t* d_d2 = d_labels;                                   // dead before the labels are written
    uint8_t* d_m[2] = {scratch<uint8_t>(h, SL_MID), scratch<uint8_t>(h, SL_CHUNK)};
    uint8_t* d_g = scratch<uint8_t>(h, SL_VALID);
    uint8_t* d_cores = d_g;                                      // g is dead behind the row pass
    unsigned long long* d_word = scratch<unsigned long long>(h, SL_PP);
    int* d_parent = scratch<int>(h, SL_CONS);
    uint32_t* d_size = (uint32_t*)(scratch<char>(h, SL_CONS) + up256(N * 4));
    char* tab = scratch<char>(h, SL_TABLES);
    uint32_t* d_sums = (uint32_t*)tab;
    unsigned long long* d_found = (unsigned long long*)(tab + o_found);
    uint32_t* d_changed = (uint32_t*)(tab + o_changed);
    uint8_t* d_dirty[2] = {(uint8_t*)(tab + o_dirty), (uint8_t*)(tab + o_dirty + tiles_b)};
    unsigned long long* d_fields = (unsigned long long*)(tab + o_fields);
    const size_t rows = band_of(0, H, row_i, kBandBytes);
    for (size_t y0 = 0; y0 < (size_t)H; y0 += rows) {
        const size_t y1 = y0 + rows < (size_t)H ? y0 + rows : H;
        HIPCHK(h, hipMemcpyAsync(d_idx + y0 * W, idx + y0 * W, (y1 - y0) * row_i, hipMemcpyHostToDevice, st));
    }
    HIPCHK(h, hipMemsetAsync(d_fields, 0, fields_b, st));
    const double px = (double)N, chunks = (double)fields_chunks(H, W);
    size_t mark[S2SR_FSPLIT_STAGES + 1];
    int stage = 0;
    mark[0] = h->evs.size();
    int32_t rounds[2] = {0, 0};
    // ---- the mask (as fields_impl makes it) and the interior
    int cur = 0;
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 3);
        HIPCHK(h, launch_fields_mask(d_idx, H, W, lo, hi, 0, d_m[cur], st));
    }
    const int steps[4][2] = {{r_open, 1}, {r_open, 0}, {r_close, 0}, {r_close, 1}};                // radius, erode
    for (const auto& s : steps) {
        if (!s[0]) continue;
        for (int column = 0; column < 2; ++column) {
            Scope sc(h, st, F_INDEX, 0.0, px * 2);
            HIPCHK(h, launch_fields_morph(d_m[cur], d_m[cur ^ 1], H, W, s[0], s[1], column, st));
            cur ^= 1;
        }
    }
    if (r_open || r_close) {
        Scope sc(h, st, F_INDEX, 0.0, px * 4);
        HIPCHK(h, launch_fields_mask(d_idx, H, W, -32767, 32767, 1, d_m[cur], st));
    }
    const uint8_t* d_mask = d_m[cur];
    const uint8_t* d_int = d_mask;                               // I = m without an edge test
    if (sp->edge) {
        Scope sc(h, st, F_INDEX, 0.0, px * 4);                   // the index and the mask in, the interior out
        HIPCHK(h, launch_fsplit_edge(d_idx, d_mask, d_m[cur ^ 1], H, W, sp->edge, sp->edge_r, st));
        d_int = d_m[cur ^ 1];
    }
    mark[++stage] = h->evs.size();                               // S2SR_FSPLIT_EDGE ends
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 7);                   // the interior in twice, g out and in, D2 out
        HIPCHK(h, launch_fsplit_distance(d_int, d_g, d_d2, H, W, st));
    }
    if (dist2) {
        for (size_t y0 = 0; y0 < (size_t)H; y0 += rows) {
            const size_t y1 = y0 + rows < (size_t)H ? y0 + rows : H;
            HIPCHK(h, hipMemcpyAsync(dist2 + y0 * W, d_d2 + y0 * W, (y1 - y0) * row_i, hipMemcpyDeviceToHost, st));
        }
    }
    mark[++stage] = h->evs.size();                               // S2SR_FSPLIT_DISTANCE ends
    auto components = [&](const uint8_t* plane) -> int {         // parent = the root, as in fields_impl
        {
            Scope sc(h, st, F_INDEX, 0.0, px * 9);
            HIPCHK(h, launch_fields_local(plane, d_parent, d_size, H, W, conn, st));
        }
        {
            const double lines = (double)((H + 63) / 64 - 1) * W + (double)((W + 63) / 64 - 1) * H;
            Scope sc(h, st, F_INDEX, 0.0, lines * 8);
            HIPCHK(h, launch_fields_border(d_parent, H, W, conn, st));
        }
        {
            Scope sc(h, st, F_INDEX, 0.0, px * 12);
            HIPCHK(h, launch_fields_flatten(d_parent, d_size, H, W, st));
        }
        return S2SR_OK;
    };
    if ((rc = components(d_int))) return rc;
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 17);                  // the maxima cleared; parents and D2 in twice, the cores out
        HIPCHK(h, launch_fsplit_cores(d_parent, d_d2, d_size, d_cores, H, W, sp->core_q, sp->core_px, st));
    }
    if (cores) HIPCHK(h, hipMemcpyAsync(cores, d_cores, N, hipMemcpyDeviceToHost, st));
    if ((rc = components(d_cores))) return rc;                   // the markers
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 12);
        HIPCHK(h, launch_fsplit_seed(d_parent, d_word, H, W, st));
    }
    mark[++stage] = h->evs.size();                               // S2SR_FSPLIT_CORES ends
    // A growth: rounds until one changes nothing.  Each round moves every path at least one tile on, so H W bounds them.
    auto grow = [&](const uint8_t* a, const uint8_t* b, int32_t* count) -> int {
        for (;;) {
            uint32_t changed = 0;
            const int k = *count & 1;                            // this round marks plane k and reads the other, the first round reads none
            HIPCHK(h, hipMemsetAsync(d_changed, 0, 4, st));
            HIPCHK(h, hipMemsetAsync(d_dirty[k], 0, tiles_b, st));
            {
                Scope sc(h, st, F_INDEX, 0.0, px * 10);          // the planes and the words in; what is stored depends on the round
                HIPCHK(h, launch_fsplit_grow(a, b, d_word, H, W, conn, d_changed, *count ? d_dirty[k ^ 1] : nullptr, d_dirty[k], st));
            }
            HIPCHK(h, hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(h, hipStreamSynchronize(st));
            ++*count;
            if (!changed) return S2SR_OK;
            if ((size_t)*count > N) return fail(h, S2SR_E_HIP, std::string(what) + "the growth did not settle within H W rounds");
        }
    };
    if ((rc = grow(d_int, nullptr, &rounds[0]))) return rc;
    mark[++stage] = h->evs.size();                               // S2SR_FSPLIT_GROW_INTERIOR ends
    if (sp->edge) {
        {
            Scope sc(h, st, F_INDEX, 0.0, px * 8);
            HIPCHK(h, launch_fsplit_restart(d_word, H, W, st));
        }
        if ((rc = grow(d_mask, d_int, &rounds[1]))) return rc;
    }
    mark[++stage] = h->evs.size();                               // S2SR_FSPLIT_GROW_EDGES ends
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 36);                  // keys set, words in twice, keys in, parents out and in, sizes cleared
        HIPCHK(h, launch_fsplit_remap(d_word, d_parent, d_size, H, W, st));
    }
    mark[++stage] = h->evs.size();                               // S2SR_FSPLIT_REMAP ends
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 4 + chunks * 4);
        HIPCHK(h, launch_fields_count(d_parent, d_size, H, W, minpx, d_sums, st));
    }
    {
        Scope sc(h, st, F_INDEX, 0.0, chunks * 8);
        HIPCHK(h, launch_fields_scan(d_sums, H, W, d_found, st));
    }
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 4 + chunks * 4);
        HIPCHK(h, launch_fields_apply(d_parent, d_size, H, W, minpx, (uint32_t)Z, d_sums, d_fields, st));
    }
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 6);
        HIPCHK(h, launch_fields_labels(d_parent, d_size, H, W, (uint32_t)Z, d_labels, d_fields, st));
    }
    mark[++stage] = h->evs.size();                               // S2SR_FSPLIT_NUMBERING ends
    for (size_t y0 = 0; y0 < (size_t)H; y0 += rows) {
        const size_t y1 = y0 + rows < (size_t)H ? y0 + rows : H;
        HIPCHK(h, hipMemcpyAsync(labels + y0 * W, d_labels + y0 * W, (y1 - y0) * row_i, hipMemcpyDeviceToHost, st));
    }
    if (fields) HIPCHK(h, hipMemcpyAsync(fields, d_fields, fields_b, hipMemcpyDeviceToHost, st));
    if (found) HIPCHK(h, hipMemcpyAsync(found, d_found, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    for (int k = 0; k < S2SR_FSPLIT_STAGES; ++k) {
        h->fsplit_stage_ms[k] = 0.0;
        h->fsplit_stage_launches[k] = 0;
        for (size_t i = mark[k]; i < mark[k + 1] && i < h->evs.size(); ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, h->evs[i].e0, h->evs[i].e1) != hipSuccess) continue;
            h->fsplit_stage_ms[k] += ms;
            h->fsplit_stage_launches[k] += h->evs[i].n;
        }
    }
    h->fsplit_rounds[0] = rounds[0];
    h->fsplit_rounds[1] = rounds[1];
    return S2SR_OK;
}

}  // namespace

extern "C" {

int s2sr_fields_split_i16(s2sr_handle* h, const int16_t* idx, int32_t H, int32_t W, int32_t lo, int32_t hi, int32_t r_open, int32_t r_close,
                          int32_t conn, int64_t min_pixels, int32_t Z, const s2sr_fields_split* split, uint16_t* labels, int64_t* fields,
                          uint64_t* found, uint16_t* dist2, uint8_t* cores) {
    if (!h) return S2SR_E_INVALID;
    if (!split) return s2sr_fields_segment_i16(h, idx, H, W, lo, hi, r_open, r_close, conn, min_pixels, Z, labels, fields, found);
    RUN_WITH_STREAM_RECOVERY(h, split_impl(h, idx, H, W, lo, hi, r_open, r_close, conn, min_pixels, Z, split, labels, fields, found, dist2, cores));
}

int s2sr_debug_fields_split_stage_ms(s2sr_handle* h, double* ms, int32_t* launches, int32_t* rounds) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!ms || !launches || !rounds) return fail(h, S2SR_E_INVALID, "s2sr_debug_fields_split_stage_ms: ms, launches and rounds are required");
    for (int k = 0; k < S2SR_FSPLIT_STAGES; ++k) {
        ms[k] = h->fsplit_stage_ms[k];
        launches[k] = h->fsplit_stage_launches[k];
    }
    rounds[0] = h->fsplit_rounds[0];
    rounds[1] = h->fsplit_rounds[1];
    return S2SR_OK;
}

}  // extern "C"
