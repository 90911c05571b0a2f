// Host side of the resampled tile levels (s2sr_tiles_resample_u8): one axis' tap tables are judged against the source extent
// and the int32 accumulator before anything reaches the device, and go up in the kernels' [K][n] order.  Plain C++, no device
// code: tests/native/resample_tables_main.cpp runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

namespace s2sr {

constexpr int kResampleMaxTaps = 64;       // S2SR_RESAMPLE_MAX_TAPS
constexpr int kResampleCoefBits = 22;

// n samples: first / count [n], coef [n][K]; extent = source pixels along the axis.  Returns nullptr when every index the
// kernels will form lies inside the source and no sample's sum can leave int32, else what is wrong.  On success *lo / *hi =
// the source range [min first, max first + count) over the samples that have taps (lo == hi == 0: none has).
inline const char* resample_check_axis(const int32_t* first, const int32_t* count, const int32_t* coef, int64_t n, int32_t K,
                                       int64_t extent, int32_t* lo, int32_t* hi) {
    if (K < 1 || K > kResampleMaxTaps) return "the tap count K must be 1..64";
    int64_t a = extent, b = 0;
    for (int64_t j = 0; j < n; ++j) {
        const int64_t f = first[j], c = count[j];
        if (c < 0 || c > K) return "a sample's tap count is not in 0..K";
        if (f < 0 || f + c > extent) return "a sample's taps leave the source";
        int64_t sum = 0;
        for (int64_t t = 0; t < c; ++t) {
            const int64_t k = coef[j * K + t];
            sum += k < 0 ? -k : k;
        }
        if (255 * sum + ((int64_t)1 << (kResampleCoefBits - 1)) >= ((int64_t)1 << 31)) return "a sample's coefficients can overflow the 32-bit sum";
        if (c > 0) {
            if (f < a) a = f;
            if (f + c > b) b = f + c;
        }
    }
    if (b <= a) a = b = 0;
    *lo = (int32_t)a;
    *hi = (int32_t)b;
    return nullptr;
}

// dst: [first n][count n][coef K x n]  (n * (2 + K) words)
inline void resample_pack_axis(const int32_t* first, const int32_t* count, const int32_t* coef, int64_t n, int32_t K, int32_t* dst) {
    for (int64_t j = 0; j < n; ++j) {
        dst[j] = first[j];
        dst[n + j] = count[j];
        for (int64_t t = 0; t < K; ++t) dst[(2 + t) * n + j] = coef[j * K + t];
    }
}

}  // namespace s2sr
