// libs2sr engine, touching fields split (kernels: fields_split.hip, and fields.hip for the mask, the components and the
// numbering): a caller's int16 index raster -> uint16 zone labels in which blobs of several parcels are cut apart, the fields table,
// their number and, on request, the distance and core planes.
#include <stdio.h>

#include <mutex>

#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

namespace {

int split_impl(s2sr_handle* h, const int16_t* idx, int H, int W, int lo, int hi, int r_open, int r_close, int conn, int64_t min_pixels, int Z,
               const s2sr_fields_split* sp, uint16_t* labels, int64_t* fields, uint64_t* found, uint16_t* dist2, uint8_t* cores) {
    std::lock_guard<std::mutex> lk(h->mu);
    const char* what = "s2sr_fields_split_i16: ";
    int rc = fields_check_args(h, what, idx, labels, H, W, lo, hi, r_open, r_close, conn, min_pixels, Z);
    if (rc) return rc;
    if (sp->core_q < 1 || sp->core_q > 1000) return fail(h, S2SR_E_INVALID, std::string(what) + "core_q must be in 1..1000");
    if (sp->core_px < 0 || sp->core_px > 255) return fail(h, S2SR_E_INVALID, std::string(what) + "core_px must be in 0..255");
    if (sp->edge < 0 || sp->edge > 32767) return fail(h, S2SR_E_INVALID, std::string(what) + "edge must be in 0..32767");
    if (sp->edge_r < 0 || sp->edge_r > 4) return fail(h, S2SR_E_INVALID, std::string(what) + "edge_r must be in 0..4");
    const size_t N = (size_t)H * W, row_i = (size_t)W * 2;
    // SL_TABLES: a segmentation's, with the growth's changed counter and its two planes of tile marks between found and fields
    const size_t tiles_b = up256(fsplit_tiles(H, W));
    const FieldsPlan p = fields_plan(H, W, min_pixels, Z, 256 + 2 * tiles_b);
    const size_t o_changed = p.o_between, o_dirty = o_changed + 256;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    // 23 bytes per pixel (fields_segment_i16: 14): the distance plane lives where the labels go later, the vertical distances where
    // the cores go later; the growth words are 8 bytes of their own, parents and sizes share SL_CONS
    rc = ensure_scratch(h, {{SL_SRC, up256(N * 2)}, {SL_DST, up256(N * 2)}, {SL_MID, up256(N)}, {SL_CHUNK, up256(N)}, {SL_VALID, up256(N)},
                            {SL_PP, up256(N * 8)}, {SL_CONS, up256(N * 4) + up256(N * 4)}, {SL_TABLES, p.bytes}});
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
    unsigned long long* d_found = (unsigned long long*)(tab + p.o_found);
    uint32_t* d_changed = (uint32_t*)(tab + o_changed);
    uint8_t* d_dirty[2] = {(uint8_t*)(tab + o_dirty), (uint8_t*)(tab + o_dirty + tiles_b)};
    unsigned long long* d_fields = (unsigned long long*)(tab + p.o_fields);
    const size_t rows = band_of(0, H, row_i, kRasterBandBytes);
    HIPCHK(h, copy_rows(h, d_idx, idx, H, row_i, rows, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemsetAsync(d_fields, 0, p.fields_b, st));
    const double px = (double)N;
    StageMarks book(h);                                          // the launches are booked in groups (s2sr_debug_fields_split_stage_ms)
    int32_t rounds[2] = {0, 0};
    // ---- the mask and the interior
    int cur = 0;
    if ((rc = fields_mask(h, st, d_idx, d_m, H, W, lo, hi, r_open, r_close, &cur))) return rc;
    const uint8_t* d_mask = d_m[cur];
    const uint8_t* d_int = d_mask;                               // I = m without an edge test
    if (sp->edge) {
        Scope sc(h, st, F_INDEX, 0.0, px * 4);                   // the index and the mask in, the interior out
        HIPCHK(h, launch_fsplit_edge(d_idx, d_mask, d_m[cur ^ 1], H, W, sp->edge, sp->edge_r, st));
        d_int = d_m[cur ^ 1];
    }
    book.next();                                                 // S2SR_FSPLIT_EDGE ends
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 7);                   // the interior in twice, g out and in, D2 out
        HIPCHK(h, launch_fsplit_distance(d_int, d_g, d_d2, H, W, st));
    }
    if (dist2) HIPCHK(h, copy_rows(h, dist2, d_d2, H, row_i, rows, hipMemcpyDeviceToHost, st));
    book.next();                                                 // S2SR_FSPLIT_DISTANCE ends
    if ((rc = fields_components(h, st, d_int, d_parent, d_size, H, W, conn, nullptr))) return rc;
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 17);                  // the maxima cleared; parents and D2 in twice, the cores out
        HIPCHK(h, launch_fsplit_cores(d_parent, d_d2, d_size, d_cores, H, W, sp->core_q, sp->core_px, st));
    }
    if (cores) HIPCHK(h, hipMemcpyAsync(cores, d_cores, N, hipMemcpyDeviceToHost, st));
    if ((rc = fields_components(h, st, d_cores, d_parent, d_size, H, W, conn, nullptr))) return rc;   // the markers
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 12);
        HIPCHK(h, launch_fsplit_seed(d_parent, d_word, H, W, st));
    }
    book.next();                                                 // S2SR_FSPLIT_CORES ends
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
    book.next();                                                 // S2SR_FSPLIT_GROW_INTERIOR ends
    if (sp->edge) {
        {
            Scope sc(h, st, F_INDEX, 0.0, px * 8);
            HIPCHK(h, launch_fsplit_restart(d_word, H, W, st));
        }
        if ((rc = grow(d_mask, d_int, &rounds[1]))) return rc;
    }
    book.next();                                                 // S2SR_FSPLIT_GROW_EDGES ends
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 36);                  // keys set, words in twice, keys in, parents out and in, sizes cleared
        HIPCHK(h, launch_fsplit_remap(d_word, d_parent, d_size, H, W, st));
    }
    book.next();                                                 // S2SR_FSPLIT_REMAP ends
    if ((rc = fields_numbering(h, st, d_parent, d_size, H, W, p.minpx, Z, d_sums, d_found, d_fields, d_labels, nullptr))) return rc;
    book.next();                                                 // S2SR_FSPLIT_NUMBERING ends
    HIPCHK(h, copy_rows(h, labels, d_labels, H, row_i, rows, hipMemcpyDeviceToHost, st));
    if (fields) HIPCHK(h, hipMemcpyAsync(fields, d_fields, p.fields_b, hipMemcpyDeviceToHost, st));
    if (found) HIPCHK(h, hipMemcpyAsync(found, d_found, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if ((rc = book.close(h->fsplit_stages))) return rc;
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
    return stage_times_out(h, &s2sr_handle::fsplit_stages, ms && launches && rounds,
                           "s2sr_debug_fields_split_stage_ms: ms, launches and rounds are required", ms, launches, rounds);
}

}  // extern "C"
