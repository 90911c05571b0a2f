// libs2sr engine, fields from the image (kernels and definition: fields.hip; rings: ring_trace.h): a caller's int16
// index raster -> uint16 zone labels, the fields table and their number; and a label raster -> the rings around its labels (host).
#include <stdio.h>

#include <mutex>

#include "engine_internal.h"
#include "ring_trace.h"

using namespace s2sr;
using namespace s2sr::engine;

// ---- the stages shared with the split (engine_internal.h).  A Scope's bytes: what the launch must move, not what its atomics and gathers add.
namespace s2sr::engine {

int fields_check_args(s2sr_handle* h, const char* what, const void* idx, const void* labels, int H, int W, int lo, int hi, int r_open, int r_close,
                      int conn, int64_t min_pixels, int Z) {
    if (!idx || !labels) return fail(h, S2SR_E_INVALID, std::string(what) + "idx and labels are required");
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return fail(h, S2SR_E_INVALID, std::string(what) + "H and W must be positive and H W < 2^31");
    if (lo < -32767 || hi > 32767 || lo > hi) return fail(h, S2SR_E_INVALID, std::string(what) + "lo <= hi, both in -32767..32767");
    if (r_open < 0 || r_open > 8 || r_close < 0 || r_close > 8) return fail(h, S2SR_E_INVALID, std::string(what) + "r_open and r_close must be in 0..8");
    if (conn != 4 && conn != 8) return fail(h, S2SR_E_INVALID, std::string(what) + "conn must be 4 or 8");
    if (min_pixels < 1) return fail(h, S2SR_E_INVALID, std::string(what) + "min_pixels must be >= 1");
    if (Z < 1 || Z > 65535) return fail(h, S2SR_E_INVALID, std::string(what) + "Z must be in 1..65535");
    return S2SR_OK;
}

FieldsPlan fields_plan(int H, int W, int64_t min_pixels, int Z, size_t between) {
    FieldsPlan p;
    p.minpx = min_pixels > 0x80000000LL ? 0x80000000u : (uint32_t)min_pixels;       // beyond H W nothing is a field
    p.o_found = up256(fields_chunks(H, W) * 4), p.o_between = p.o_found + 256, p.o_fields = p.o_between + between;
    p.fields_b = ((size_t)Z + 1) * 6 * 8, p.bytes = p.o_fields + up256(p.fields_b);
    return p;
}

int fields_mask(s2sr_handle* h, hipStream_t st, const int16_t* d_idx, uint8_t* const d_m[2], int H, int W, int lo, int hi, int r_open, int r_close,
                int* cur) {
    const double px = (double)H * W;
    int c = 0;                                                   // the plane that holds the mask so far
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 3);                   // the index in, a plane out
        HIPCHK(h, launch_fields_mask(d_idx, H, W, lo, hi, 0, d_m[c], st));
    }
    // open = dilate(erode), close = erode(dilate): each a row pass and a column pass
    const int steps[4][2] = {{r_open, 1}, {r_open, 0}, {r_close, 0}, {r_close, 1}};                // radius, erode
    for (const auto& s : steps) {
        if (!s[0]) continue;
        for (int column = 0; column < 2; ++column) {
            Scope sc(h, st, F_INDEX, 0.0, px * 2);               // a plane in, a plane out (a column pass reads its rows from cache)
            HIPCHK(h, launch_fields_morph(d_m[c], d_m[c ^ 1], H, W, s[0], s[1], column, st));
            c ^= 1;
        }
    }
    if (r_open || r_close) {                                     // a close may have bridged nodata
        Scope sc(h, st, F_INDEX, 0.0, px * 4);                   // the index and the plane in, the plane out
        HIPCHK(h, launch_fields_mask(d_idx, H, W, -32767, 32767, 1, d_m[c], st));
    }
    *cur = c;
    return S2SR_OK;
}

int fields_components(s2sr_handle* h, hipStream_t st, const uint8_t* plane, int* d_parent, uint32_t* d_size, int H, int W, int conn, StageMarks* book) {
    const double px = (double)H * W;
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 9);                   // a plane in, parents and sizes out
        HIPCHK(h, launch_fields_local(plane, d_parent, d_size, H, W, conn, st));
    }
    if (book) book->next();
    {
        const double lines = (double)((H + 63) / 64 - 1) * W + (double)((W + 63) / 64 - 1) * H;
        Scope sc(h, st, F_INDEX, 0.0, lines * 8);                // a border pixel's parent and its neighbour's; the walks come on top
        HIPCHK(h, launch_fields_border(d_parent, H, W, conn, st));
    }
    if (book) book->next();
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 12);                  // parents in and out, sizes in
        HIPCHK(h, launch_fields_flatten(d_parent, d_size, H, W, st));
    }
    if (book) book->next();
    return S2SR_OK;
}

int fields_numbering(s2sr_handle* h, hipStream_t st, int* d_parent, uint32_t* d_size, int H, int W, uint32_t minpx, int Z, uint32_t* d_sums,
                     unsigned long long* d_found, unsigned long long* d_fields, uint16_t* d_labels, StageMarks* book) {
    const double px = (double)H * W, chunks = (double)fields_chunks(H, W);
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 4 + chunks * 4);      // parents in (sizes at the roots only), the sums out
        HIPCHK(h, launch_fields_count(d_parent, d_size, H, W, minpx, d_sums, st));
    }
    if (book) book->next();
    {
        Scope sc(h, st, F_INDEX, 0.0, chunks * 8);
        HIPCHK(h, launch_fields_scan(d_sums, H, W, d_found, st));
    }
    if (book) book->next();
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 4 + chunks * 4);
        HIPCHK(h, launch_fields_apply(d_parent, d_size, H, W, minpx, (uint32_t)Z, d_sums, d_fields, st));
    }
    if (book) book->next();
    {
        Scope sc(h, st, F_INDEX, 0.0, px * 6);                   // parents in, labels out (ranks at the roots only)
        HIPCHK(h, launch_fields_labels(d_parent, d_size, H, W, (uint32_t)Z, d_labels, d_fields, st));
    }
    if (book) book->next();
    return S2SR_OK;
}

}  // namespace s2sr::engine

namespace {

int fields_impl(s2sr_handle* h, const int16_t* idx, int H, int W, int lo, int hi, int r_open, int r_close, int conn, int64_t min_pixels, int Z,
                uint16_t* labels, int64_t* fields, uint64_t* found) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = fields_check_args(h, "s2sr_fields_segment_i16: ", idx, labels, H, W, lo, hi, r_open, r_close, conn, min_pixels, Z);
    if (rc) return rc;
    const size_t N = (size_t)H * W, row_i = (size_t)W * 2;
    const FieldsPlan p = fields_plan(H, W, min_pixels, Z);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    rc = ensure_scratch(h, {{SL_SRC, up256(N * 2)}, {SL_DST, up256(N * 2)}, {SL_MID, up256(N)}, {SL_CHUNK, up256(N)}, {SL_PP, up256(N * 4)},
                            {SL_CONS, up256(N * 4)}, {SL_TABLES, p.bytes}});
    if (rc) return rc;
    int16_t* d_idx = scratch<int16_t>(h, SL_SRC);
    uint16_t* d_labels = scratch<uint16_t>(h, SL_DST);
    uint8_t* d_m[2] = {scratch<uint8_t>(h, SL_MID), scratch<uint8_t>(h, SL_CHUNK)};
    int* d_parent = scratch<int>(h, SL_PP);
    uint32_t* d_size = scratch<uint32_t>(h, SL_CONS);
    char* tab = scratch<char>(h, SL_TABLES);
    uint32_t* d_sums = (uint32_t*)tab;
    unsigned long long* d_found = (unsigned long long*)(tab + p.o_found);
    unsigned long long* d_fields = (unsigned long long*)(tab + p.o_fields);
    const size_t rows = band_of(0, H, row_i, kRasterBandBytes);
    HIPCHK(h, copy_rows(h, d_idx, idx, H, row_i, rows, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemsetAsync(d_fields, 0, p.fields_b, st));
    StageMarks book(h);                                          // every launch is booked to its stage (s2sr_debug_fields_stage_ms)
    int cur = 0;
    if ((rc = fields_mask(h, st, d_idx, d_m, H, W, lo, hi, r_open, r_close, &cur))) return rc;
    book.next();                                                 // S2SR_FIELDS_STAGE_MASK ends
    if ((rc = fields_components(h, st, d_m[cur], d_parent, d_size, H, W, conn, &book))) return rc;
    if ((rc = fields_numbering(h, st, d_parent, d_size, H, W, p.minpx, Z, d_sums, d_found, d_fields, d_labels, &book))) return rc;
    HIPCHK(h, copy_rows(h, labels, d_labels, H, row_i, rows, hipMemcpyDeviceToHost, st));
    if (fields) HIPCHK(h, hipMemcpyAsync(fields, d_fields, p.fields_b, hipMemcpyDeviceToHost, st));
    if (found) HIPCHK(h, hipMemcpyAsync(found, d_found, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return book.close(h->fields_stages);
}

int trace_impl(s2sr_handle* h, const uint16_t* labels, int H, int W, int Z, uint64_t xy_cap, uint64_t ring_cap, int32_t* xy, int32_t* ring_start,
               uint16_t* ring_label, uint64_t* counts) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!counts) return fail(h, S2SR_E_INVALID, "s2sr_labels_trace_u16: counts is required");
    counts[0] = counts[1] = 0;
    RingTrace t;
    if (const char* why = ring_trace(labels, H, W, Z, &t)) return fail(h, S2SR_E_INVALID, std::string("s2sr_labels_trace_u16: ") + why);
    ring_trace_copy(t, xy_cap, ring_cap, xy, ring_start, ring_label, counts);
    return S2SR_OK;
}

}  // namespace

extern "C" {

int s2sr_fields_segment_i16(s2sr_handle* h, const int16_t* idx, int32_t H, int32_t W, int32_t lo, int32_t hi, int32_t r_open, int32_t r_close,
                            int32_t conn, int64_t min_pixels, int32_t Z, uint16_t* labels, int64_t* fields, uint64_t* found) {
    RUN_WITH_STREAM_RECOVERY(h, fields_impl(h, idx, H, W, lo, hi, r_open, r_close, conn, min_pixels, Z, labels, fields, found));
}

int s2sr_debug_fields_stage_ms(s2sr_handle* h, double* ms, int32_t* launches) {
    return stage_times_out(h, &s2sr_handle::fields_stages, ms && launches, "s2sr_debug_fields_stage_ms: ms and launches are required", ms, launches);
}

int s2sr_labels_trace_u16(s2sr_handle* h, const uint16_t* labels, int32_t H, int32_t W, int32_t Z, uint64_t xy_cap, uint64_t ring_cap, int32_t* xy,
                          int32_t* ring_start, uint16_t* ring_label, uint64_t* counts) {
    return trace_impl(h, labels, H, W, Z, xy_cap, ring_cap, xy, ring_start, ring_label, counts);
}

}  // extern "C"
