// libs2sr engine, the display rendering of 16-bit images (kernels and definition: display.hip): the histogram and
// the LUT pass over a uint16 [H, W, 3] image in row bands, from a host image or from the image the previous call left on the device.
#include <stdio.h>
#include <string.h>

#include <mutex>

#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

namespace {

constexpr size_t kHistBytes = 3 * 65536 * sizeof(uint64_t), kLutBytes = 3 * 65536;
constexpr size_t kBandSamples = (size_t)1 << 30;       // most samples one histogram launch counts (32-bit LDS counters)

// The source of a display call and its row bands.  img == NULL: the H x W image the last call kept, where it lies; a host image
// goes to SL_SRC.  Either way the image is what the call keeps at its end.
struct Source {
    KeptInput in;
    int rows = 0, nbands = 0;
    size_t row_s = 0, total = 0;         // samples per row and in the image
};

int plan_source(s2sr_handle* h, const char* who, const uint16_t* img, int H, int W, int band_rows, Source& s) {
    char b[256];
    if (H <= 0 || W <= 0 || band_rows < 0) {
        snprintf(b, sizeof b, "%s: H, W must be positive and band_rows >= 0", who);
        return fail(h, S2SR_E_INVALID, b);
    }
    s.row_s = (size_t)W * 3;
    s.total = s.row_s * H;
    if (s.row_s > kBandSamples) {
        snprintf(b, sizeof b, "%s: rows of more than 2^30 samples are not supported", who);
        return fail(h, S2SR_E_INVALID, b);
    }
    if (!img && !s.in.take(KEPT_U16, H, W)) {
        snprintf(b, sizeof b, "%s: img == NULL, but the previous call on this handle did not leave a uint16 image of this size on the device", who);
        return fail(h, S2SR_E_INVALID, b);
    }
    // the library's choice: ~32 MB of samples per band (its upload hides the band before's kernel); never more than one launch counts
    size_t rows = band_of(band_rows, H, s.row_s, (size_t)16 << 20);                     // (counted in samples here)
    if (rows > kBandSamples / s.row_s) rows = kBandSamples / s.row_s;
    s.rows = (int)rows;
    s.nbands = (H + s.rows - 1) / s.rows;
    return S2SR_OK;
}

// upload of band i of a host image into SL_SRC, on the copy stream, and the event behind it
int upload_band(s2sr_handle* h, const uint16_t* img, const Source& s, int H, int i, hipEvent_t ev) {
    const size_t y0 = (size_t)i * s.rows, y1 = y0 + s.rows < (size_t)H ? y0 + s.rows : H;
    HIPCHK(h, hipMemcpyAsync(scratch<uint16_t>(h, SL_SRC) + y0 * s.row_s, img + y0 * s.row_s, (y1 - y0) * s.row_s * 2, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(h, ev_record(h, ev, h->copy_stream, SITE_DISPLAY_UPLOAD));
    return S2SR_OK;
}

int display_hist_impl(s2sr_handle* h, const uint16_t* img, int H, int W, int nodata, int band_rows, uint64_t* hist) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!hist) return fail(h, S2SR_E_INVALID, "s2sr_display_hist_u16: hist is required");
    if (nodata < -1 || nodata > 65535) return fail(h, S2SR_E_INVALID, "s2sr_display_hist_u16: nodata must be -1 (none) or 0..65535");
    Source s{KeptInput(h)};
    int rc = plan_source(h, "s2sr_display_hist_u16", img, H, W, band_rows, s);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    if ((rc = ensure_scratch(h, {{SL_SRC, up256(s.total * 2), img != nullptr}, {SL_TABLES, kHistBytes + kLutBytes}}))) return rc;
    if ((rc = ensure_group_events(h, 4))) return rc;
    const uint16_t* d_img = scratch<const uint16_t>(h, s.in.slot);
    unsigned long long* d_hist = scratch<unsigned long long>(h, SL_TABLES);
    HIPCHK(h, hipMemsetAsync(d_hist, 0, kHistBytes, st));
    // a host image: band i + 1 uploads on the copy stream under band i's kernel
    if (img && (rc = upload_band(h, img, s, H, 0, h->group_done[0]))) return rc;
    for (int i = 0; i < s.nbands; ++i) {
        const size_t y0 = (size_t)i * s.rows, y1 = y0 + s.rows < (size_t)H ? y0 + s.rows : H;
        if (img) HIPCHK(h, ev_stream_wait(h, st, h->group_done[i & 1], SITE_DISPLAY_UPLOAD));
        {
            Scope sc(h, st, F_DHIST, 0.0, (double)(y1 - y0) * s.row_s * 2.0);
            HIPCHK(h, launch_display_hist(d_img, y0 * s.row_s, y1 * s.row_s, nodata, d_hist, st));
        }
        if (img && i + 1 < s.nbands && (rc = upload_band(h, img, s, H, i + 1, h->group_done[(i + 1) & 1]))) return rc;
    }
    HIPCHK(h, hipMemcpyAsync(hist, d_hist, kHistBytes, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    h->scratch.keep(KEPT_U16, s.in.slot, H, W);
    return S2SR_OK;
}

int display_apply_impl(s2sr_handle* h, const uint16_t* img, int H, int W, const uint8_t* lut, int band_rows, uint8_t* out) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!lut || !out) return fail(h, S2SR_E_INVALID, "s2sr_display_apply_u16: lut and out are required");
    Source s{KeptInput(h)};
    int rc = plan_source(h, "s2sr_display_apply_u16", img, H, W, band_rows, s);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    const Slot out_slot = other(s.in.slot);                   // the 8-bit image: the other of 0 / 1, as the pyramid calls do
    if ((rc = ensure_scratch(h, {{SL_SRC, up256(s.total * 2), img != nullptr}, {out_slot, s.total}, {SL_TABLES, kHistBytes + kLutBytes}}))) return rc;
    if ((rc = ensure_group_events(h, 4))) return rc;
    const uint16_t* d_img = scratch<const uint16_t>(h, s.in.slot);
    uint8_t* d_out = scratch<uint8_t>(h, out_slot);
    uint8_t* d_lut = scratch<uint8_t>(h, SL_TABLES) + kHistBytes;
    HIPCHK(h, hipMemcpyAsync(d_lut, lut, kLutBytes, hipMemcpyHostToDevice, st));
    // band i + 1 uploads under band i's kernel (a host image); band i's bytes leave under band i + 1's
    hipEvent_t* up = &h->group_done[0];
    hipEvent_t* done = &h->group_done[2];
    if (img && (rc = upload_band(h, img, s, H, 0, up[0]))) return rc;
    size_t pb0 = 0, pb1 = 0;                                 // the band before, in bytes of the output
    for (int i = 0; i < s.nbands; ++i) {
        const size_t y0 = (size_t)i * s.rows, y1 = y0 + s.rows < (size_t)H ? y0 + s.rows : H;
        if (img) HIPCHK(h, ev_stream_wait(h, st, up[i & 1], SITE_DISPLAY_UPLOAD));
        {
            Scope sc(h, st, F_DAPPLY, 0.0, (double)(y1 - y0) * s.row_s * 3.0);
            HIPCHK(h, launch_display_apply(d_img, y0 * s.row_s, y1 * s.row_s, d_lut, d_out, st));
        }
        HIPCHK(h, ev_record(h, done[i & 1], st, SITE_DISPLAY_BAND_D2H));
        if (img && i + 1 < s.nbands && (rc = upload_band(h, img, s, H, i + 1, up[(i + 1) & 1]))) return rc;
        if (i > 0) {
            HIPCHK(h, ev_stream_wait(h, h->copy_stream, done[(i - 1) & 1], SITE_DISPLAY_BAND_D2H));
            if ((rc = d2h_staged(h, out + pb0, d_out + pb0, pb1 - pb0, false))) return rc;
        }
        pb0 = y0 * s.row_s; pb1 = y1 * s.row_s;
    }
    HIPCHK(h, ev_stream_wait(h, h->copy_stream, done[(s.nbands - 1) & 1], SITE_DISPLAY_BAND_D2H));
    if ((rc = d2h_staged(h, out + pb0, d_out + pb0, pb1 - pb0, true))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    HIPCHK(h, hipStreamSynchronize(st));
    h->scratch.keep(KEPT_U16, s.in.slot, H, W);
    return S2SR_OK;
}

}  // namespace

extern "C" {

int s2sr_display_hist_u16(s2sr_handle* h, const uint16_t* img, int32_t H, int32_t W, int32_t nodata, int32_t band_rows, uint64_t* hist) {
    RUN_WITH_STREAM_RECOVERY(h, display_hist_impl(h, img, H, W, nodata, band_rows, hist));
}

int s2sr_display_apply_u16(s2sr_handle* h, const uint16_t* img, int32_t H, int32_t W, const uint8_t* lut, int32_t band_rows, uint8_t* out) {
    RUN_WITH_STREAM_RECOVERY(h, display_apply_impl(h, img, H, W, lut, band_rows, out));
}

}  // extern "C"
