// Stand-alone driver of the poison logic of csrc/redzone.h (namespace poison: the pattern, the chunked fill, the read-back), built
// with -fsanitize=address,undefined by tests/test_poison_cpu.py.  The "device" is the heap: every range is an exact-size malloc
// block and the two callbacks are memcpy, so a fill or a read-back one byte past the caller's bytes is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "redzone.h"

using namespace s2sr;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static size_t g_writes = 0, g_reads = 0, g_fail_after = (size_t)-1;
static bool io_write(void*, void* dst, const uint8_t* src, size_t n) {
    if (g_writes >= g_fail_after) return false;
    memcpy(dst, src, n);
    ++g_writes;
    return true;
}
static bool io_read(void*, uint8_t* dst, const void* src, size_t n) { memcpy(dst, src, n); ++g_reads; return true; }
static const redzone::DeviceIo kIo{io_write, io_read, nullptr};

static void test_patterns() {
    EXPECT(poison::valid(0) && poison::valid(1) && poison::valid(2) && !poison::valid(3) && !poison::valid(-1));
    bool constant = true;
    for (size_t i = 0; i < 3 * poison::kPeriod; ++i) {
        EXPECT(poison::byte_at(poison::kOnes, i) == 0xFF);
        const uint8_t b = poison::byte_at(poison::kPositional, i);
        EXPECT(b != 0);
        EXPECT(b == redzone::pattern(false, i));
        EXPECT(b == poison::byte_at(poison::kPositional, i + poison::kPeriod));   // what lets one chunk serve every chunk
        constant = constant && b == poison::byte_at(poison::kPositional, 0);
    }
    EXPECT(!constant);
    EXPECT(poison::kChunk % poison::kPeriod == 0);
    // what pattern 1 reads as: -1 as an int32, a NaN as an fp32
    int32_t i32; float f32;
    uint8_t four[4];
    for (int k = 0; k < 4; ++k) four[k] = poison::byte_at(poison::kOnes, (size_t)k);
    memcpy(&i32, four, 4); memcpy(&f32, four, 4);
    EXPECT(i32 == -1 && f32 != f32);
}

// every size around the chunk boundaries, at exact-size blocks inside a guarded frame the fill must not touch
static void test_fill_sizes() {
    const size_t C = poison::kChunk;
    const size_t sizes[] = {0, 1, 2, 255, 256, 257, 4096, 65535, 65536, 65537, C - 1, C, C + 1, 2 * C, 2 * C + 77777};
    for (int pat = 1; pat <= 2; ++pat)
        for (size_t n : sizes) {
            uint8_t* blk = (uint8_t*)malloc(n ? n : 1);    // exact size: ASan sees byte n
            memset(blk, 0, n ? n : 1);
            const size_t w0 = g_writes;
            EXPECT(poison::fill(kIo, blk, n, pat));
            EXPECT(g_writes - w0 == (n + C - 1) / C);
            size_t bad = 0;
            for (size_t i = 0; i < n; ++i) bad += blk[i] != poison::byte_at(pat, i);
            EXPECT(bad == 0);
            if (!n) EXPECT(blk[0] == 0);
            size_t first = 12345;
            EXPECT(poison::first_unpoisoned(kIo, blk, n, pat, &first) && first == n);
            if (n) {                                       // one byte put right anywhere is found, the first of two is reported
                const size_t at[] = {0, n / 2, n - 1};
                for (size_t a : at) {
                    const uint8_t good = blk[a];
                    blk[a] = 0;
                    blk[n - 1] = 0;
                    EXPECT(poison::first_unpoisoned(kIo, blk, n, pat, &first) && first == a);
                    blk[a] = good;
                    blk[n - 1] = poison::byte_at(pat, n - 1);
                }
                // the other pattern does not pass for this one
                EXPECT(poison::first_unpoisoned(kIo, blk, n, 3 - pat, &first));
                EXPECT(first < n || (n == 1 && poison::byte_at(3 - pat, 0) == poison::byte_at(pat, 0)));
            }
            free(blk);
        }
}

// a range in the middle of a block (a scratch slot's bytes between its zones): nothing outside it changes
static void test_fill_inside_a_frame() {
    const size_t front = 4096, n = poison::kChunk + 4099, back = 4096;
    std::vector<uint8_t> blk(front + n + back, 0x33);
    for (int pat = 1; pat <= 2; ++pat) {
        EXPECT(poison::fill(kIo, blk.data() + front, n, pat));
        size_t outside = 0, inside = 0;
        for (size_t i = 0; i < front; ++i) outside += blk[i] != 0x33;
        for (size_t i = 0; i < back; ++i) outside += blk[front + n + i] != 0x33;
        for (size_t i = 0; i < n; ++i) inside += blk[front + i] != poison::byte_at(pat, i);
        EXPECT(outside == 0 && inside == 0);
    }
}

// the mode off writes nothing; a failing device write is reported
static void test_off_and_failure() {
    std::vector<uint8_t> blk(1000, 0x44);
    const size_t w0 = g_writes;
    EXPECT(poison::fill(kIo, blk.data(), blk.size(), poison::kOff));
    EXPECT(g_writes == w0);
    for (uint8_t b : blk) EXPECT(b == 0x44);
    std::vector<uint8_t> big(2 * poison::kChunk + 5, 0);
    g_fail_after = g_writes + 1;                           // the second chunk fails
    EXPECT(!poison::fill(kIo, big.data(), big.size(), poison::kOnes));
    g_fail_after = (size_t)-1;
    EXPECT(big[0] == 0xFF && big[poison::kChunk] == 0);
}

// poison under red zones: the fill of the user bytes leaves both zones whole
static void test_with_zones() {
    const size_t Z = 4096, n = 70001;
    redzone::Registry reg;
    char* base = (char*)malloc(n + 2 * Z);
    memset(base, 0, n + 2 * Z);
    EXPECT(reg.add(kIo, base + Z, n, Z, Z));
    for (int pat = 1; pat <= 2; ++pat) {
        EXPECT(poison::fill(kIo, base + Z, n, pat));
        size_t checked = 0, bad = 0;
        redzone::Damage d;
        EXPECT(reg.check_all(kIo, &checked, &bad, &d) && checked == 1 && bad == 0);
        size_t first = 0;
        EXPECT(poison::first_unpoisoned(kIo, base + Z, n, pat, &first) && first == n);
    }
    redzone::Record r;
    EXPECT(reg.remove(kIo, base + Z, &r) && reg.sticky() == 0);
    free(r.base());
}

int main() {
    test_patterns();
    test_fill_sizes();
    test_fill_inside_a_frame();
    test_off_and_failure();
    test_with_zones();
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
