// Stand-alone driver of csrc/resample_tables.h (the host code of s2sr_tiles_resample_u8 that reads caller tables), built with
// -fsanitize=address,undefined by tests/test_resample_cpu.py.  Tables live in exact-size heap blocks, so a read past a table
// is reported; coefficients include INT32_MIN / INT32_MAX, so the absolute sums must not overflow.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "resample_tables.h"

using namespace s2sr;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Axis {
    std::vector<int32_t> first, count, coef;
    int K;
    int64_t n;
    Axis(int64_t n_, int K_) : first(n_, 0), count(n_, 0), coef((size_t)n_ * (K_ > 0 ? K_ : 0), 0), K(K_), n(n_) {}
    const char* check(int64_t extent, int32_t* lo, int32_t* hi) const {
        return resample_check_axis(first.data(), count.data(), coef.data(), n, K, extent, lo, hi);
    }
};

int main() {
    std::mt19937 rng(7);
    int32_t lo = -1, hi = -1;
    for (int K : {1, 2, 6, 13, 64}) {
        const int64_t n = 256, extent = 100;
        Axis a(n, K);
        int32_t want_lo = (int32_t)extent, want_hi = 0;
        for (int64_t j = 0; j < n; ++j) {
            a.count[j] = (int32_t)(rng() % (K + 1));
            a.first[j] = (int32_t)(rng() % (extent - a.count[j] + 1));
            for (int t = 0; t < K; ++t) a.coef[j * K + t] = (int32_t)(rng() % 200001) - 100000;
            if (a.count[j]) {
                if (a.first[j] < want_lo) want_lo = a.first[j];
                if (a.first[j] + a.count[j] > want_hi) want_hi = a.first[j] + a.count[j];
            }
        }
        EXPECT(a.check(extent, &lo, &hi) == nullptr && lo == want_lo && hi == want_hi);
        std::vector<int32_t> packed((size_t)n * (2 + K));
        resample_pack_axis(a.first.data(), a.count.data(), a.coef.data(), n, K, packed.data());
        for (int64_t j = 0; j < n; ++j) {
            EXPECT(packed[j] == a.first[j] && packed[n + j] == a.count[j]);
            for (int t = 0; t < K; ++t) EXPECT(packed[(2 + t) * n + j] == a.coef[j * K + t]);
        }
        Axis b = a;                             // taps past the end, by one
        b.count[5] = K; b.first[5] = (int32_t)extent - K + 1;
        EXPECT(b.check(extent, &lo, &hi) != nullptr);
        b = a; b.first[0] = -1; b.count[0] = 1;
        EXPECT(b.check(extent, &lo, &hi) != nullptr);
        b = a; b.count[7] = K + 1;
        EXPECT(b.check(extent, &lo, &hi) != nullptr);
        b = a; b.count[7] = -1;
        EXPECT(b.check(extent, &lo, &hi) != nullptr);
        b = a; b.first[9] = INT32_MAX; b.count[9] = K;       // first + count beyond int32
        EXPECT(b.check(extent, &lo, &hi) != nullptr);
        b = a; b.count[3] = K; b.first[3] = 0;
        for (int t = 0; t < K; ++t) b.coef[3 * K + t] = t & 1 ? INT32_MIN : INT32_MAX;
        EXPECT(b.check(extent, &lo, &hi) != nullptr);        // the overflow bound, with sums far beyond int32
        b = a; b.count[3] = 1; b.first[3] = 0; b.coef[3 * K] = 8413341;           // 255 * 8413341 + 2^21 = 2^31 - 2^21 + 255 ... just inside
        EXPECT((255 * (int64_t)8413341 + (1 << 21) < ((int64_t)1 << 31)) == (b.check(extent, &lo, &hi) == nullptr));
        b.coef[3 * K] = -8421505;                                                 // 255 * 8421505 + 2^21 >= 2^31
        EXPECT(b.check(extent, &lo, &hi) != nullptr);
    }
    {
        Axis a(256, 4);                         // no sample has taps: an empty source range
        EXPECT(a.check(10, &lo, &hi) == nullptr && lo == 0 && hi == 0);
        Axis k0(256, 0), k65(256, 65);
        EXPECT(k0.check(10, &lo, &hi) != nullptr && k65.check(10, &lo, &hi) != nullptr);
    }
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
