// libs2sr engine, carrying an extra band to the SR grid (kernels and definition: bands.hip): a uint16 band [H, W]
// upsampled against the uint16 image [S H, S W, 3] of a 16-bit door, from a host image or from the image the previous call left on
// the device, in bands of guide rows.
#include <stdio.h>

#include <mutex>

#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

namespace {

constexpr size_t kHead = 256;      // SL_CONS: the inexact counter, then C (int64 [H, W]), then A (int32 [H, W])

// The rows each stage may finish once guide rows [0, final_rows) are final (last: and nothing more comes), as cons_out_end does for
// the consistency pass: a pixel's window reaches r input rows down, a block's interpolation one coefficient row further.
int coeffs_end(int S, int H, int r, int final_rows, bool last) {
    const int b = final_rows / S - r;
    return last ? H : b > 0 ? b : 0;
}
int apply_end(int H, int coeffs_done, bool last) { return last ? H : coeffs_done > 1 ? coeffs_done - 1 : 0; }

int carry_band_impl(s2sr_handle* h, const uint16_t* sr, const uint16_t* band, int H, int W, int S, int lo, int hi, const int32_t* w, int r, int eps,
                    const uint8_t* valid, int fill, int band_rows, uint16_t* out, uint64_t* inexact) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!band || !out || !w || H <= 0 || W <= 0) return fail(h, S2SR_E_INVALID, "s2sr_carry_band_u16: a band, guide weights, positive sizes and an output are required");
    if (S != 2 && S != 4) return fail(h, S2SR_E_INVALID, "s2sr_carry_band_u16: S must be 2 or 4");
    if (r < 1 || r > 4) return fail(h, S2SR_E_INVALID, "s2sr_carry_band_u16: the window radius r must be 1..4");
    if (eps < 1) return fail(h, S2SR_E_INVALID, "s2sr_carry_band_u16: eps must be >= 1");
    if (!(0 <= lo && lo < hi && hi <= 65535)) return fail(h, S2SR_E_INVALID, "s2sr_carry_band_u16: need 0 <= lo < hi <= 65535");
    if (w[0] < 0 || w[0] > 255 || w[1] < 0 || w[1] > 255 || w[2] < 0 || w[2] > 255 || w[0] + w[1] + w[2] < 1)
        return fail(h, S2SR_E_INVALID, "s2sr_carry_band_u16: the guide weights must be 0..255 and not all zero");
    if (fill < 0 || fill > 65535) return fail(h, S2SR_E_INVALID, "s2sr_carry_band_u16: fill must be 0..65535");
    if (band_rows < 0) return fail(h, S2SR_E_INVALID, "s2sr_carry_band_u16: band_rows must be >= 0");
    if ((long long)H * S > 0x3fffffffLL || (long long)W * S * 3 > 0x3fffffffLL) return fail(h, S2SR_E_INVALID, "s2sr_carry_band_u16: the image is too large");
    const int OH = H * S, OW = W * S;
    KeptInput in(h);
    if (!sr && !in.take(KEPT_U16, OH, OW))
        return fail(h, S2SR_E_INVALID, "s2sr_carry_band_u16: sr == NULL, but the previous call on this handle did not leave a uint16 image of this size on the device");
    const size_t px = (size_t)H * W, grow_b = (size_t)OW * 3 * 2, orow_b = (size_t)OW * 2;
    const int wt[3] = {w[0], w[1], w[2]};
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    const Slot out_slot = other(in.slot);                     // the carried plane: the other of 0 / 1, as the display pass's 8-bit image
    int rc = ensure_scratch(h, {{SL_SRC, grow_b * OH, sr != nullptr}, {out_slot, orow_b * OH}, {SL_MID, px * 2}, {SL_VALID, px, valid != nullptr},
                                {SL_CONS, kHead + px * (sizeof(long long) + sizeof(int32_t))}});
    if (rc) return rc;
    uint16_t* d_q = scratch<uint16_t>(h, in.slot);
    uint16_t* d_out = scratch<uint16_t>(h, out_slot);
    uint16_t* d_band = scratch<uint16_t>(h, SL_MID);
    uint8_t* d_valid = valid ? scratch<uint8_t>(h, SL_VALID) : nullptr;
    unsigned long long* d_cnt = scratch<unsigned long long>(h, SL_CONS);
    long long* d_C = (long long*)(scratch<char>(h, SL_CONS) + kHead);
    int32_t* d_A = (int32_t*)(d_C + px);
    HIPCHK(h, hipMemsetAsync(d_cnt, 0, kHead, st));
    HIPCHK(h, hipMemcpyAsync(d_band, band, px * 2, hipMemcpyHostToDevice, st));
    if (valid) HIPCHK(h, hipMemcpyAsync(d_valid, valid, px, hipMemcpyHostToDevice, st));
    const size_t rows = band_of(band_rows, OH, grow_b, (size_t)32 << 20);              // the library's choice: ~32 MB of guide
    int c_done = 0, a_done = 0;                               // input rows whose coefficients are there; block rows that have left
    for (const RowBand gb : row_bands(OH, rows)) {
        const int y1 = (int)gb.y1;
        if (sr) HIPCHK(h, hipMemcpyAsync((char*)d_q + gb.y0 * grow_b, (const char*)sr + gb.y0 * grow_b, gb.rows() * grow_b, hipMemcpyHostToDevice, st));
        const int ce = coeffs_end(S, H, r, y1, gb.last);
        if (ce > c_done) {
            Scope sc(h, st, F_BANDS, 0.0, (double)(ce - c_done) * W * (S * S * 6.0 + 2.0 + 12.0));
            HIPCHK(h, launch_band_coeffs(d_q, d_band, d_valid, d_A, d_C, H, W, S, c_done, ce, lo, hi, wt, r, (long long)eps, st));
            c_done = ce;
        }
        const int ae = apply_end(H, c_done, gb.last);
        if (ae > a_done) {
            {
                Scope sc(h, st, F_BANDS, 0.0, (double)(ae - a_done) * W * (S * S * 8.0 + 2.0 + 12.0));
                HIPCHK(h, launch_band_apply(d_q, d_band, d_valid, d_A, d_C, d_out, d_cnt, H, W, S, a_done, ae, lo, hi, wt, fill, st));
            }
            const size_t b0 = (size_t)a_done * S * orow_b, b1 = (size_t)ae * S * orow_b;
            HIPCHK(h, hipMemcpyAsync((char*)out + b0, (const char*)d_out + b0, b1 - b0, hipMemcpyDeviceToHost, st));
            a_done = ae;
        }
    }
    unsigned long long n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, d_cnt, sizeof n, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (inexact) *inexact = n;
    h->scratch.keep(KEPT_U16, in.slot, OH, OW);               // the guide is intact: the next band, or a display call, reads it again
    return S2SR_OK;
}

}  // namespace

extern "C" {

int s2sr_carry_band_u16(s2sr_handle* h, const uint16_t* sr, const uint16_t* band, int32_t H, int32_t W, int32_t S, int32_t lo, int32_t hi,
                        const int32_t* w, int32_t r, int32_t eps, const uint8_t* valid, int32_t fill, int32_t band_rows, uint16_t* out,
                        uint64_t* inexact) {
    RUN_WITH_STREAM_RECOVERY(h, carry_band_impl(h, sr, band, H, W, S, lo, hi, w, r, eps, valid, fill, band_rows, out, inexact));
}

}  // extern "C"
