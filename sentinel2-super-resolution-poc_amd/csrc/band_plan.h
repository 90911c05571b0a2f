// The bands of a chunked whole-image job (engine_aoi.hip): which output rows each chunk of window rows makes final.  Plain host
// arithmetic, no HIP in here: s2sr_debug_plan_bands exposes it to the CPU tests and tests/native/blend_plan_main.cpp runs it under
// the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace s2sr {

// chunk_r0[0 .. nchunks]: the first window row of each chunk, then ny.  last_row[stride * y]: the last window row output row y
// reads, monotone in y (the paste map's window row; the blend row table's later window).  A row is final once that window row is
// done, so chunk k makes rows [band_end[k - 1], band_end[k]) final (from 0 for k = 0): those whose last window row lies in front
// of the chunk's end.  The chunk that ends the image takes every row that is left.
inline void plan_bands(const int* chunk_r0, int nchunks, int ny, int OH, const int32_t* last_row, int stride, int* band_end) {
    int ye = 0;
    for (int k = 0; k < nchunks; ++k) {
        const int r1 = chunk_r0[k + 1] < ny ? chunk_r0[k + 1] : ny;
        if (r1 >= ny) ye = OH;
        while (ye < OH && last_row[(size_t)stride * ye] < r1) ++ye;
        band_end[k] = ye;
    }
}

}  // namespace s2sr
