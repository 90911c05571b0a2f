// The row bands of a banded raster pass (engine_index.hip, engine_zones.hip, engine_fields.hip, engine_fields_split.hip,
// engine_mzones.hip, engine_bands.hip, the consistency door of engine_aoi.hip): how many rows one band takes, and the bands of H
// rows taken that many at a time.  Plain host arithmetic, no HIP in here: tests/native/row_bands_main.cpp runs it under the
// sanitizers.
#pragma once
#include <stddef.h>

namespace s2sr {

// The rows of one band of a banded pass: the caller's band_rows, or the library's choice of budget_bytes moved per band (row_bytes:
// what one row moves); at least 1, at most H.
inline size_t band_of(int band_rows, size_t H, size_t row_bytes, size_t budget_bytes) {
    const size_t rows = band_rows > 0 ? (size_t)band_rows : budget_bytes / row_bytes;
    return rows < 1 ? 1 : rows > H ? H : rows;
}

struct RowBand {
    size_t y0, y1;             // rows [y0, y1)
    bool last;                 // y1 == H: nothing comes behind this band
    size_t rows() const { return y1 - y0; }
};

// for (const RowBand b : row_bands(H, rows)): [0, rows), [rows, 2 rows), ... and what is left of H; no band for H == 0.  An iterable,
// not a callback: the body may return from the function around it (HIPCHK).  No sum is formed that could pass H, so neither can wrap.
struct RowBands {
    size_t H, step;
    struct Iter {
        size_t y0, H, step;
        size_t end() const { return H - y0 > step ? y0 + step : H; }
        RowBand operator*() const { return RowBand{y0, end(), end() == H}; }
        Iter& operator++() { y0 = end(); return *this; }
        bool operator!=(const Iter& o) const { return y0 != o.y0; }
    };
    Iter begin() const { return Iter{0, H, step}; }
    Iter end() const { return Iter{H, H, step}; }
};
inline RowBands row_bands(size_t H, size_t rows) { return RowBands{H, rows ? rows : 1}; }

}  // namespace s2sr
