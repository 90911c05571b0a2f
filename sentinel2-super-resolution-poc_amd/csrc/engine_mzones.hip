// libs2sr engine, management zones (kernels and definition: mzones.hip): a caller's int16 index rasters and uint16
// labels -> the uint8 zone raster, the per-zone table, the centres, the status per field and the number of iterations.
#include <stdio.h>

#include <mutex>

#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

namespace {

int mzones_impl(s2sr_handle* h, const int16_t* feat, int D, int H, int W, const uint16_t* labels, int Z, int k, int iters, int64_t min_per_zone,
                int smooth, int band_rows, uint8_t* zone, int64_t* table, int32_t* centres, uint8_t* status, uint32_t* iterations) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const char* what = "s2sr_zones_kmeans_i16: ";
    if (!feat || !labels || !zone) return fail(h, S2SR_E_INVALID, std::string(what) + "feat, labels and zone are required");
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return fail(h, S2SR_E_INVALID, std::string(what) + "H and W must be positive and H W < 2^31");
    if (D < 1 || D > 4) return fail(h, S2SR_E_INVALID, std::string(what) + "D must be in 1..4");
    if (k < 2 || k > 8) return fail(h, S2SR_E_INVALID, std::string(what) + "k must be in 2..8");
    if (iters < 1 || iters > 64) return fail(h, S2SR_E_INVALID, std::string(what) + "iters must be in 1..64");
    if (smooth < 0 || smooth > 4) return fail(h, S2SR_E_INVALID, std::string(what) + "smooth must be in 0..4");
    if (Z < 1 || Z > 65535) return fail(h, S2SR_E_INVALID, std::string(what) + "Z must be in 1..65535");
    if (min_per_zone < 1) return fail(h, S2SR_E_INVALID, std::string(what) + "min_per_zone must be >= 1");
    if (band_rows < 0) return fail(h, S2SR_E_INVALID, std::string(what) + "band_rows must be >= 0");
    const size_t N = (size_t)H * W, F = (size_t)Z + 1;
    const long long least = (long long)k * (min_per_zone > 0x80000000LL ? 0x80000000LL : min_per_zone);   // beyond H W every field is skipped
    // SL_TABLES: cnt, lo, hi, status, zone_of, centres, ranked, changed, acc (the iterations' sums, then the table)
    const size_t o_lo = up256(F * 4), o_hi = o_lo + up256(F * D * 4), o_status = o_hi + up256(F * D * 4), o_zone_of = o_status + up256(F);
    const size_t o_centres = o_zone_of + up256(F * k), o_ranked = o_centres + up256(F * k * D * 4), o_changed = o_ranked + up256(F * k * D * 4);
    const size_t o_acc = o_changed + 256, acc_b = F * k * (1 + D) * 8, table_b = F * k * (1 + 2 * D) * 8;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    int rc = ensure_scratch(h, {{SL_SRC, up256(N * 2 * D)}, {SL_DST, up256(N * 2)}, {SL_MID, up256(N)}, {SL_CHUNK, up256(N)}, {SL_TABLES, o_acc + up256(table_b)}});
    if (rc) return rc;
    int16_t* d_feat = scratch<int16_t>(h, SL_SRC);
    uint16_t* d_labels = scratch<uint16_t>(h, SL_DST);
    uint8_t* d_z[2] = {scratch<uint8_t>(h, SL_MID), scratch<uint8_t>(h, SL_CHUNK)};
    char* tab = scratch<char>(h, SL_TABLES);
    uint32_t* d_cnt = (uint32_t*)tab;
    int* d_lo = (int*)(tab + o_lo);
    int* d_hi = (int*)(tab + o_hi);
    uint8_t* d_status = (uint8_t*)(tab + o_status);
    uint8_t* d_zone_of = (uint8_t*)(tab + o_zone_of);
    int* d_centres = (int*)(tab + o_centres);
    int* d_ranked = (int*)(tab + o_ranked);
    uint32_t* d_changed = (uint32_t*)(tab + o_changed);
    unsigned long long* d_acc = (unsigned long long*)(tab + o_acc);
    // the bands the rasters travel in, the statistics pass behind each; and the bands of the passes that run on the whole raster,
    // which are the caller's or one
    const size_t rows = band_of(band_rows, H, (size_t)W * (2 * D + 2), kRasterBandBytes);
    const size_t prows = band_rows > 0 ? band_of(band_rows, H, 1, 1) : (size_t)H;
    const double cells = (double)(F * k);
    StageMarks book(h);                                          // every launch is booked to its stage (s2sr_debug_mzones_stage_ms)
    HIPCHK(h, hipMemsetAsync(d_acc, 0, acc_b, st));
    {
        Scope sc(h, st, F_INDEX, 0.0, (double)F * (4 + 8 * D));
        HIPCHK(h, launch_mzones_clear(d_cnt, d_lo, d_hi, Z, D, st));
    }
    for (const RowBand b : row_bands(H, rows)) {
        HIPCHK(h, hipMemcpyAsync(d_labels + b.y0 * W, labels + b.y0 * W, b.rows() * W * 2, hipMemcpyHostToDevice, st));
        for (int d = 0; d < D; ++d)
            HIPCHK(h, hipMemcpyAsync(d_feat + d * N + b.y0 * W, feat + d * N + b.y0 * W, b.rows() * W * 2, hipMemcpyHostToDevice, st));
        Scope sc(h, st, F_INDEX, 0.0, (double)b.rows() * W * (2 * D + 2));
        HIPCHK(h, launch_mzones_stats(d_feat, D, H, W, (int)b.y0, (int)b.y1, d_labels, Z, d_cnt, d_lo, d_hi, st));
    }
    {
        Scope sc(h, st, F_INDEX, 0.0, cells * (1 + 4 * D));
        HIPCHK(h, launch_mzones_start(d_cnt, d_lo, d_hi, Z, k, D, least, d_status, d_centres, st));
    }
    book.next();                                                 // S2SR_MZONES_STATISTICS ends
    uint32_t ran = (uint32_t)iters;
    for (int t = 1; t <= iters; ++t) {
        HIPCHK(h, hipMemsetAsync(d_changed, 0, 4, st));
        for (const RowBand b : row_bands(H, prows)) {
            Scope sc(h, st, F_INDEX, 0.0, (double)b.rows() * W * (2 * D + 2));   // labels and features in; the sums leave through atomics
            HIPCHK(h, launch_mzones_accumulate(d_feat, D, H, W, (int)b.y0, (int)b.y1, d_labels, Z, k, d_centres, d_status, nullptr, d_acc, st));
        }
        {
            Scope sc(h, st, F_INDEX, 0.0, cells * (1 + D) * 16);
            HIPCHK(h, launch_mzones_update(d_acc, Z, k, D, d_status, d_centres, d_changed, st));
        }
        uint32_t moved = 0;                                      // a fixed point: nothing later changes a byte
        HIPCHK(h, hipMemcpyAsync(&moved, d_changed, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        if (!moved) {
            ran = (uint32_t)t;
            break;
        }
    }
    book.next();
    {
        Scope sc(h, st, F_INDEX, 0.0, cells * (2 + 8 * D));
        HIPCHK(h, launch_mzones_rank(d_centres, Z, k, D, d_status, d_zone_of, d_ranked, st));
    }
    for (const RowBand b : row_bands(H, rows)) {
        Scope sc(h, st, F_INDEX, 0.0, (double)b.rows() * W * (2 * D + 3));
        HIPCHK(h, launch_mzones_assign(d_feat, D, H, W, (int)b.y0, (int)b.y1, d_labels, Z, k, d_centres, d_status, d_zone_of, d_z[0], st));
    }
    book.next();
    int cur = 0;                                                 // the plane that holds the raster so far
    for (int s = 0; s < smooth; ++s) {
        for (const RowBand b : row_bands(H, prows)) {
            Scope sc(h, st, F_INDEX, 0.0, (double)b.rows() * W * 4);                 // a plane and the labels in (the neighbours from cache), a plane out
            HIPCHK(h, launch_mzones_mode(d_z[cur], d_labels, H, W, (int)b.y0, (int)b.y1, k, d_z[cur ^ 1], st));
        }
        cur ^= 1;
    }
    book.next();
    if (table) {
        HIPCHK(h, hipMemsetAsync(d_acc, 0, table_b, st));
        for (const RowBand b : row_bands(H, prows)) {
            Scope sc(h, st, F_INDEX, 0.0, (double)b.rows() * W * (2 * D + 3));
            HIPCHK(h, launch_mzones_accumulate(d_feat, D, H, W, (int)b.y0, (int)b.y1, d_labels, Z, k, nullptr, nullptr, d_z[cur], d_acc, st));
        }
    }
    book.next();
    HIPCHK(h, copy_rows(h, zone, d_z[cur], H, W, rows, hipMemcpyDeviceToHost, st));
    if (table) HIPCHK(h, hipMemcpyAsync(table, d_acc, table_b, hipMemcpyDeviceToHost, st));
    if (centres) HIPCHK(h, hipMemcpyAsync(centres, d_ranked, F * k * D * 4, hipMemcpyDeviceToHost, st));
    if (status) HIPCHK(h, hipMemcpyAsync(status, d_status, F, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (iterations) *iterations = ran;
    return book.close(h->mzones_stages);
}

}  // namespace

extern "C" {

int s2sr_zones_kmeans_i16(s2sr_handle* h, const int16_t* feat, int32_t D, int32_t H, int32_t W, const uint16_t* labels, int32_t Z, int32_t k, int32_t iters,
                          int64_t min_per_zone, int32_t smooth, int32_t band_rows, uint8_t* zone, int64_t* table, int32_t* centres, uint8_t* status,
                          uint32_t* iterations) {
    RUN_WITH_STREAM_RECOVERY(h, mzones_impl(h, feat, D, H, W, labels, Z, k, iters, min_per_zone, smooth, band_rows, zone, table, centres, status, iterations));
}

int s2sr_debug_mzones_stage_ms(s2sr_handle* h, double* ms, int32_t* launches) {
    return stage_times_out(h, &s2sr_handle::mzones_stages, ms && launches, "s2sr_debug_mzones_stage_ms: ms and launches are required", ms, launches);
}

}  // extern "C"
