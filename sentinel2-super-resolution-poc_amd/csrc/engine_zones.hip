// libs2sr engine, polygon rasterisation to zone labels (kernel and definition: zones.hip; checks and binning:
// zone_bins.h): a caller's features -> the uint16 label raster and the pixels per label, in row bands.
#include <stdio.h>

#include <mutex>

#include "engine_internal.h"
#include "zone_bins.h"

using namespace s2sr;
using namespace s2sr::engine;

namespace {

int zones_impl(s2sr_handle* h, const int32_t* xy, const int32_t* ring_start, const int32_t* feat_start, const uint16_t* label, int F, int Z, int H,
               int W, int band_rows, uint16_t* out, uint64_t* area) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!out) return fail(h, S2SR_E_INVALID, "s2sr_zones_rasterize_u16: out is required");
    if (band_rows < 0) return fail(h, S2SR_E_INVALID, "s2sr_zones_rasterize_u16: band_rows must be >= 0");
    if (const char* why = zone_check_tables(xy, ring_start, feat_start, label, F, Z, H, W))
        return fail(h, S2SR_E_INVALID, std::string("s2sr_zones_rasterize_u16: ") + why);
    ZoneBins bins;
    const char* why = zone_build_bins(xy, ring_start, feat_start, F, H, W, &bins);
    if (!why) why = zone_check_bins(bins, F);
    if (why) return fail(h, S2SR_E_INVALID, std::string("s2sr_zones_rasterize_u16: ") + why);
    const size_t R = (size_t)feat_start[F], V = (size_t)ring_start[R], T = (size_t)(bins.tiles_x * bins.tiles_y), nnz = bins.feat.size();
    const size_t row_b = (size_t)W * 2;
    // the tables, one behind the other in SL_TABLES: xy, ring_start, feat_start, label, the bins' starts and features, area
    const size_t o_ring = up256(V * 8), o_feat = o_ring + up256((R + 1) * 4), o_label = o_feat + up256(((size_t)F + 1) * 4);
    const size_t o_start = o_label + up256((size_t)F * 2), o_list = o_start + up256((T + 1) * 4), o_area = o_list + up256((nnz ? nnz : 1) * 4);
    const size_t area_b = area ? up256(((size_t)Z + 1) * 8) : 0;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    int rc = ensure_scratch(h, {{SL_DST, up256(row_b * H)}, {SL_TABLES, o_area + area_b}});
    if (rc) return rc;
    uint16_t* d_out = scratch<uint16_t>(h, SL_DST);
    char* tab = scratch<char>(h, SL_TABLES);
    unsigned long long* d_area = area ? (unsigned long long*)(tab + o_area) : nullptr;
    HIPCHK(h, hipMemcpyAsync(tab, xy, V * 8, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(tab + o_ring, ring_start, (R + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(tab + o_feat, feat_start, ((size_t)F + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(tab + o_label, label, (size_t)F * 2, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(tab + o_start, bins.start.data(), (T + 1) * 4, hipMemcpyHostToDevice, st));
    if (nnz) HIPCHK(h, hipMemcpyAsync(tab + o_list, bins.feat.data(), nnz * 4, hipMemcpyHostToDevice, st));
    if (area) HIPCHK(h, hipMemsetAsync(d_area, 0, area_b, st));
    const size_t rows = band_of(band_rows, H, row_b, kRasterBandBytes);                // the caller's, or ~64 MB of labels per band
    for (const RowBand b : row_bands(H, rows)) {
        {
            Scope sc(h, st, F_INDEX, 0.0, (double)b.rows() * row_b);
            HIPCHK(h, launch_zones_rasterize((const int32_t*)tab, (const int32_t*)(tab + o_ring), (const int32_t*)(tab + o_feat),
                                             (const uint16_t*)(tab + o_label), (const uint32_t*)(tab + o_start), (const int32_t*)(tab + o_list), H, W,
                                             (int)b.y0, (int)b.y1, d_out, d_area, st));
        }
        HIPCHK(h, hipMemcpyAsync(out + b.y0 * W, d_out + b.y0 * W, b.rows() * row_b, hipMemcpyDeviceToHost, st));
    }
    if (area) HIPCHK(h, hipMemcpyAsync(area, d_area, ((size_t)Z + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return S2SR_OK;
}

}  // namespace

extern "C" {

int s2sr_zones_rasterize_u16(s2sr_handle* h, const int32_t* xy, const int32_t* ring_start, const int32_t* feat_start, const uint16_t* label, int32_t F,
                             int32_t Z, int32_t H, int32_t W, int32_t band_rows, uint16_t* out, uint64_t* area) {
    RUN_WITH_STREAM_RECOVERY(h, zones_impl(h, xy, ring_start, feat_start, label, F, Z, H, W, band_rows, out, area));
}

}  // extern "C"
