// Stand-alone driver of csrc/row_bands.h (the rows of a band and the bands of a raster), built with -fsanitize=address,undefined by
// tests/test_row_bands_cpu.py.  Arithmetic only: no raster is allocated, at no size.
#include <stdio.h>

#include "row_bands.h"

using namespace s2sr;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// ordered, disjoint, covering exactly [0, H); all but the last of `rows` rows; ceil(H / rows) of them; last on the final one alone
static size_t check_bands(size_t H, size_t rows) {
    size_t n = 0, at = 0, lasts = 0;
    bool short_seen = false;
    for (const RowBand b : row_bands(H, rows)) {
        EXPECT(b.y0 == at && b.y1 > b.y0 && b.y1 <= H);
        EXPECT(b.rows() == b.y1 - b.y0 && b.rows() <= rows);
        EXPECT(!short_seen);                       // nothing follows a band of fewer rows
        if (b.rows() != rows) short_seen = true;
        EXPECT(b.last == (b.y1 == H));
        EXPECT(lasts == 0);                        // nothing follows the last band
        lasts += b.last;
        at = b.y1;
        ++n;
    }
    EXPECT(at == H && lasts == 1);
    EXPECT(n == H / rows + (H % rows != 0));
    return n;
}

static void test_small_rasters() {
    for (size_t H = 1; H <= 70; ++H)
        for (size_t rows = 1; rows <= H + 2; ++rows) check_bands(H, rows);
}

static void test_no_rows_no_bands() {
    size_t n = 0;
    for (const RowBand b : row_bands(0, 4)) n += 1 + b.y0;
    EXPECT(n == 0);
}

static void test_rows_past_int32() {
    // y0 + rows passes 2^31 - 1 in the second band: ceil(0x7fffffff / 0x40000000) = 2 bands, the second one row short
    EXPECT(check_bands(0x7fffffff, 0x40000000) == 2);
    size_t n = 0;
    for (const RowBand b : row_bands(0x7fffffff, 0x40000000)) {
        EXPECT(b.y0 == n * 0x40000000u && b.y1 == (n ? 0x7fffffffu : 0x40000000u) && b.last == (n == 1));
        ++n;
    }
    // one row fewer per band: three, the last of a single row
    EXPECT(check_bands(0x7fffffff, 0x3fffffff) == 3);
    n = 0;
    for (const RowBand b : row_bands(0x7fffffff, 0x3fffffff)) {
        if (n == 2) EXPECT(b.y0 == 0x7ffffffeu && b.rows() == 1 && b.last);
        ++n;
    }
    // the largest size_t: one band, or two, and no sum that wraps
    EXPECT(check_bands((size_t)-1, (size_t)-1) == 1 && check_bands((size_t)-1, (size_t)-2) == 2);
}

static void test_band_of() {
    const size_t MB = (size_t)1 << 20;
    // a positive band_rows wins, whatever the budget says, and is clamped to H
    EXPECT(band_of(5, 100, 1000, 64 * MB) == 5);
    EXPECT(band_of(1, 100, 1, 1) == 1);
    EXPECT(band_of(100, 100, 1000, 64 * MB) == 100 && band_of(101, 100, 1000, 64 * MB) == 100);
    EXPECT(band_of(0x7fffffff, 7, 1000, 64 * MB) == 7);
    // otherwise budget / row_bytes, clamped to [1, H]
    EXPECT(band_of(0, 100000, 32768, 64 * MB) == 2048);
    EXPECT(band_of(0, 2047, 32768, 64 * MB) == 2047 && band_of(0, 2048, 32768, 64 * MB) == 2048 && band_of(0, 2049, 32768, 64 * MB) == 2048);
    EXPECT(band_of(-3, 100000, 32768, 64 * MB) == 2048);
    EXPECT(band_of(0, 1, 2, 64 * MB) == 1);
    // a row above the budget travels alone
    EXPECT(band_of(0, 100, 64 * MB + 1, 64 * MB) == 1 && band_of(0, 100, 64 * MB, 64 * MB) == 1 && band_of(0, 100, 32 * MB, 64 * MB) == 2);
    EXPECT(band_of(0, 100, (size_t)-1, 64 * MB) == 1);
}

int main() {
    test_small_rasters();
    test_no_rows_no_bands();
    test_rows_past_int32();
    test_band_of();
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
