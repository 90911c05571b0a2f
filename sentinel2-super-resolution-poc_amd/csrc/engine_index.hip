// libs2sr engine, normalised-difference indices on the SR grid (kernels and definition: index.hip): the index of
// two uint16 planes with its rendering, histogram and zonal sums, from host planes or from a channel of the uint16 image the
// previous call left on the device, in row bands; and the rendering of an int16 index raster that already exists.
#include <stdio.h>

#include <mutex>

#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

namespace {

constexpr size_t kLutBytes = 65536 * 4;

int index_nd_impl(s2sr_handle* h, const uint16_t* a, int ac, int ca, const uint16_t* b, int bc, int cb, int H, int W, int offset, int L, int K,
                  const uint8_t* valid, int vs, const uint16_t* zones, int zs, int Z, const uint8_t* lut, int band_rows, int16_t* out,
                  uint64_t* hist, int64_t* zonal, uint8_t* rgba, uint64_t* undefined) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!b || H <= 0 || W <= 0) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: a plane b and positive sizes are required");
    if (K < 1 || K > 16383) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: the scale K must be 1..16383");
    if (L < 0 || L > 65535 || offset < 0 || offset > 65535) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: offset and L must be 0..65535");
    if ((ac != 1 && ac != 3) || (bc != 1 && bc != 3)) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: ac and bc must be 1 or 3");
    if (!a) ac = 3;                                             // the kept image is [H, W, 3]
    if (ca < 0 || ca >= ac || cb < 0 || cb >= bc) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: a channel lies outside its image");
    if (valid && vs < 1) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: valid_scale must be >= 1");
    if (zones && zs < 1) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: zone_scale must be >= 1");
    if ((zones != nullptr) != (zonal != nullptr)) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: zones and zonal go together");
    if (zones && (Z < 1 || Z > 65535)) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: Z must be 1..65535");
    if (rgba && !lut) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: rgba needs a lut");
    if (!out && !hist && !zonal && !rgba && !undefined) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: every output is NULL");
    if (band_rows < 0) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: band_rows must be >= 0");
    if ((long long)H * W > 0x7fffffffLL) return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: the image is too large");
    KeptInput in(h);
    if (!a && !in.take(KEPT_U16, H, W))
        return fail(h, S2SR_E_INVALID, "s2sr_index_nd_u16: a == NULL, but the previous call on this handle did not leave a uint16 image of this size on the device");
    const size_t px = (size_t)H * W, arow_b = (size_t)W * ac * 2, brow_b = (size_t)W * bc * 2;
    const size_t vw = valid ? ((size_t)W + vs - 1) / vs : 0, vh = valid ? ((size_t)H + vs - 1) / vs : 0;
    const size_t zw = zones ? ((size_t)W + zs - 1) / zs : 0, zh = zones ? ((size_t)H + zs - 1) / zs : 0;
    const size_t hist_b = hist ? up256((size_t)(2 * K + 1) * 8) : 0, zonal_b = zonal ? up256((size_t)(Z + 1) * 24) : 0;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    const Slot out_slot = other(in.slot);                     // the index plane, the RGBA behind it: the other of 0 / 1
    int rc = ensure_scratch(h, {{SL_SRC, up256(arow_b * H), a != nullptr}, {out_slot, up256(px * 2) + up256(px * 4)}, {SL_MID, up256(brow_b * H)},
                                {SL_VALID, up256(vw * vh) + up256(zw * zh * 2), valid || zones}, {SL_TABLES, kLutBytes + 256 + hist_b + zonal_b}});
    if (rc) return rc;
    const uint16_t* d_a = scratch<const uint16_t>(h, in.slot);
    uint16_t* d_b = scratch<uint16_t>(h, SL_MID);
    int16_t* d_out = out ? scratch<int16_t>(h, out_slot) : nullptr;
    uint8_t* d_rgba = rgba ? scratch<uint8_t>(h, out_slot) + up256(px * 2) : nullptr;
    uint8_t* d_valid = valid ? scratch<uint8_t>(h, SL_VALID) : nullptr;
    uint16_t* d_zones = zones ? (uint16_t*)(scratch<char>(h, SL_VALID) + up256(vw * vh)) : nullptr;
    uint8_t* d_lut = lut ? scratch<uint8_t>(h, SL_TABLES) : nullptr;
    unsigned long long* d_undef = (unsigned long long*)(scratch<char>(h, SL_TABLES) + kLutBytes);     // the counter, then hist, then zonal
    unsigned long long* d_hist = hist ? d_undef + 32 : nullptr;
    unsigned long long* d_zonal = zonal ? d_undef + 32 + hist_b / 8 : nullptr;
    HIPCHK(h, hipMemsetAsync(d_undef, 0, 256 + hist_b + zonal_b, st));
    if (lut) HIPCHK(h, hipMemcpyAsync(d_lut, lut, kLutBytes, hipMemcpyHostToDevice, st));
    if (valid) HIPCHK(h, hipMemcpyAsync(d_valid, valid, vw * vh, hipMemcpyHostToDevice, st));
    if (zones) HIPCHK(h, hipMemcpyAsync(d_zones, zones, zw * zh * 2, hipMemcpyHostToDevice, st));
    const size_t rows = band_of(band_rows, H, (a ? arow_b : 0) + brow_b + (out ? (size_t)W * 2 : 0) + (rgba ? (size_t)W * 4 : 0), kRasterBandBytes);
    for (const RowBand band : row_bands(H, rows)) {
        if (a) HIPCHK(h, hipMemcpyAsync((char*)d_a + band.y0 * arow_b, (const char*)a + band.y0 * arow_b, band.rows() * arow_b, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync((char*)d_b + band.y0 * brow_b, (const char*)b + band.y0 * brow_b, band.rows() * brow_b, hipMemcpyHostToDevice, st));
        {
            Scope sc(h, st, F_INDEX, 0.0, (double)band.rows() * W * (4.0 + (out ? 2.0 : 0.0) + (rgba ? 4.0 : 0.0)));
            HIPCHK(h, launch_index_nd(d_a, ac, ca, d_b, bc, cb, H, W, (int)band.y0, (int)band.y1, offset, L, K, d_valid, vs, d_zones, zs, Z, d_lut, d_out,
                                      d_hist, d_zonal, d_rgba, d_undef, st));
        }
        if (out) HIPCHK(h, hipMemcpyAsync(out + band.y0 * W, d_out + band.y0 * W, band.rows() * W * 2, hipMemcpyDeviceToHost, st));
        if (rgba) HIPCHK(h, hipMemcpyAsync(rgba + band.y0 * W * 4, d_rgba + band.y0 * W * 4, band.rows() * W * 4, hipMemcpyDeviceToHost, st));
    }
    unsigned long long n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, d_undef, sizeof n, hipMemcpyDeviceToHost, st));
    if (hist) HIPCHK(h, hipMemcpyAsync(hist, d_hist, (size_t)(2 * K + 1) * 8, hipMemcpyDeviceToHost, st));
    if (zonal) HIPCHK(h, hipMemcpyAsync(zonal, d_zonal, (size_t)(Z + 1) * 24, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (undefined) *undefined = n;
    if (!a) h->scratch.keep(KEPT_U16, in.slot, H, W);         // the image is intact: the next index, a carried band or a display call reads it again
    return S2SR_OK;
}

int index_render_impl(s2sr_handle* h, const int16_t* idx, int H, int W, const uint8_t* lut, int band_rows, uint8_t* rgba) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!idx || !lut || !rgba || H <= 0 || W <= 0) return fail(h, S2SR_E_INVALID, "s2sr_index_render_i16: idx, lut, rgba and positive sizes are required");
    if (band_rows < 0) return fail(h, S2SR_E_INVALID, "s2sr_index_render_i16: band_rows must be >= 0");
    if ((long long)H * W > 0x7fffffffLL) return fail(h, S2SR_E_INVALID, "s2sr_index_render_i16: the image is too large");
    const size_t px = (size_t)H * W;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    int rc = ensure_scratch(h, {{SL_SRC, up256(px * 2)}, {SL_DST, up256(px * 4)}, {SL_TABLES, kLutBytes}});
    if (rc) return rc;
    int16_t* d_idx = scratch<int16_t>(h, SL_SRC);
    uint8_t* d_rgba = scratch<uint8_t>(h, SL_DST);
    uint8_t* d_lut = scratch<uint8_t>(h, SL_TABLES);
    HIPCHK(h, hipMemcpyAsync(d_lut, lut, kLutBytes, hipMemcpyHostToDevice, st));
    const size_t rows = band_of(band_rows, H, (size_t)W * 6, kRasterBandBytes);
    for (const RowBand band : row_bands(H, rows)) {
        HIPCHK(h, hipMemcpyAsync(d_idx + band.y0 * W, idx + band.y0 * W, band.rows() * W * 2, hipMemcpyHostToDevice, st));
        {
            Scope sc(h, st, F_INDEX, 0.0, (double)band.rows() * W * 6.0);
            HIPCHK(h, launch_index_render(d_idx, H, W, (int)band.y0, (int)band.y1, d_lut, d_rgba, st));
        }
        HIPCHK(h, hipMemcpyAsync(rgba + band.y0 * W * 4, d_rgba + band.y0 * W * 4, band.rows() * W * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(h, hipStreamSynchronize(st));
    return S2SR_OK;
}

}  // namespace

extern "C" {

int s2sr_index_nd_u16(s2sr_handle* h, const uint16_t* a, int32_t ac, int32_t ca, const uint16_t* b, int32_t bc, int32_t cb, int32_t H, int32_t W,
                      int32_t offset, int32_t L, int32_t K, const uint8_t* valid, int32_t valid_scale, const uint16_t* zones, int32_t zone_scale,
                      int32_t Z, const uint8_t* lut, int32_t band_rows, int16_t* out_i16, uint64_t* hist, int64_t* zonal, uint8_t* rgba,
                      uint64_t* undefined) {
    RUN_WITH_STREAM_RECOVERY(h, index_nd_impl(h, a, ac, ca, b, bc, cb, H, W, offset, L, K, valid, valid_scale, zones, zone_scale, Z, lut, band_rows,
                                              out_i16, hist, zonal, rgba, undefined));
}

int s2sr_index_render_i16(s2sr_handle* h, const int16_t* idx, int32_t H, int32_t W, const uint8_t* lut, int32_t band_rows, uint8_t* rgba) {
    RUN_WITH_STREAM_RECOVERY(h, index_render_impl(h, idx, H, W, lut, band_rows, rgba));
}

}  // extern "C"
