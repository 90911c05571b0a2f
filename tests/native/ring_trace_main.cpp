// Stand-alone driver of csrc/ring_trace.h (the host code that walks the rings around the labels of a raster), so that it runs under
// the address and undefined-behaviour sanitizers without Python or a GPU: tests/test_fields_cpu.py builds it with
// -fsanitize=address,undefined and runs it twice.
//   ring_trace <file>   the file holds whitespace-separated integers: the number of cases, then per case H W Z and the H W labels.
//                       Each raster is copied to an exact-size heap block, traced, and taken through the capacity protocol: a call
//                       at capacity 0 writes nothing and reports the counts, one vertex or one ring too few writes nothing either,
//                       exact-size tables are filled.  Prints "case <i> <vertices> <rings>" and per ring "<label>: x y x y ...".
//   ring_trace          the refusals, random rasters of up to 40 x 40 pixels whose rings are checked for closure, unit axis-parallel
//                       steps between direction changes, a turn at every vertex and an area sum that equals each label's pixel count;
//                       prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <set>
#include <utility>
#include <vector>

#include "ring_trace.h"

using namespace s2sr;

#define REQUIRE(cond)                                                         \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static int protocol(const RingTrace& t, std::vector<int32_t>* xy_out) {
    const uint64_t V = t.xy.size() / 2, R = t.ring_label.size();
    uint64_t counts[2] = {99, 99};
    REQUIRE(!ring_trace_copy(t, 0, 0, nullptr, nullptr, nullptr, counts));
    REQUIRE(counts[0] == V && counts[1] == R);
    // exact-size heap blocks: a write past either end is the sanitizer's
    std::unique_ptr<int32_t[]> xy(new int32_t[2 * V + 1]), rs(new int32_t[R + 1]);
    std::unique_ptr<uint16_t[]> rl(new uint16_t[R + 1]);
    if (V) {
        memset(xy.get(), 0x5a, (2 * V + 1) * 4);
        REQUIRE(!ring_trace_copy(t, V - 1, R, xy.get(), rs.get(), rl.get(), counts) && counts[0] == V && counts[1] == R);
        for (uint64_t i = 0; i < 2 * V; ++i) REQUIRE(xy[i] == 0x5a5a5a5a);
        REQUIRE(!ring_trace_copy(t, V, R - 1, xy.get(), rs.get(), rl.get(), counts) && counts[0] == V && counts[1] == R);
        for (uint64_t i = 0; i < 2 * V; ++i) REQUIRE(xy[i] == 0x5a5a5a5a);
    }
    REQUIRE(ring_trace_copy(t, V, R, xy.get(), rs.get(), rl.get(), counts) && counts[0] == V && counts[1] == R);
    REQUIRE(rs[0] == 0 && (uint64_t)rs[R] == V);
    xy_out->assign(xy.get(), xy.get() + 2 * V);
    return 0;
}

static int from_file(const char* path) {
    FILE* f = fopen(path, "r");
    REQUIRE(f);
    long cases = 0;
    REQUIRE(fscanf(f, "%ld", &cases) == 1);
    for (long i = 0; i < cases; ++i) {
        long H, W, Z;
        REQUIRE(fscanf(f, "%ld %ld %ld", &H, &W, &Z) == 3 && H > 0 && W > 0);
        std::unique_ptr<uint16_t[]> lab(new uint16_t[(size_t)H * W]);
        for (long k = 0; k < H * W; ++k) {
            long v;
            REQUIRE(fscanf(f, "%ld", &v) == 1 && v >= 0 && v <= 65535);
            lab[k] = (uint16_t)v;
        }
        RingTrace t;
        REQUIRE(ring_trace(lab.get(), (int)H, (int)W, (int)Z, &t) == nullptr);
        std::vector<int32_t> xy;
        if (protocol(t, &xy)) return 1;
        printf("case %ld %zu %zu\n", i, xy.size() / 2, t.ring_label.size());
        for (size_t r = 0; r < t.ring_label.size(); ++r) {
            printf("%u:", (unsigned)t.ring_label[r]);
            for (int32_t v = t.ring_start[r]; v < t.ring_start[r + 1]; ++v) printf(" %d %d", xy[2 * v], xy[2 * v + 1]);
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}

static int self_checks() {
    RingTrace t;
    uint16_t one = 1;
    REQUIRE(ring_trace(nullptr, 1, 1, 1, &t) != nullptr);
    REQUIRE(ring_trace(&one, 0, 1, 1, &t) != nullptr && ring_trace(&one, 1, -1, 1, &t) != nullptr);
    REQUIRE(ring_trace(&one, 65536, 32768, 1, &t) != nullptr);
    REQUIRE(ring_trace(&one, 1, 1, 0, &t) != nullptr && ring_trace(&one, 1, 1, 65536, &t) != nullptr);
    REQUIRE(ring_trace(&one, 1, 1, 1, &t) == nullptr && t.xy.size() == 8 && t.ring_label.size() == 1);
    uint32_t seed = 12345;
    const auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int round = 0; round < 200; ++round) {
        const int H = 1 + (int)(rnd() % 40), W = 1 + (int)(rnd() % 40), nl = 1 + (int)(rnd() % 4), Z = 3;
        std::unique_ptr<uint16_t[]> lab(new uint16_t[(size_t)H * W]);
        std::map<uint32_t, long long> pixels;
        for (int k = 0; k < H * W; ++k) {
            lab[k] = (uint16_t)(rnd() % (nl + 1));
            if (lab[k] >= 1 && lab[k] <= Z) pixels[lab[k]] += 1;
        }
        REQUIRE(ring_trace(lab.get(), H, W, Z, &t) == nullptr);
        std::vector<int32_t> xy;
        if (protocol(t, &xy)) return 1;
        std::map<uint32_t, long long> area2;
        for (size_t r = 0; r < t.ring_label.size(); ++r) {
            const int32_t a = t.ring_start[r], b = t.ring_start[r + 1];
            REQUIRE(b - a >= 4 && (b - a) % 2 == 0 && t.ring_label[r] >= 1 && t.ring_label[r] <= Z);
            REQUIRE(r == 0 || t.ring_label[r - 1] <= t.ring_label[r]);
            std::set<std::pair<int32_t, int32_t>> seen;
            long long s = 0;
            int repeated = 0;
            for (int32_t v = a; v < b; ++v) {
                const int32_t n = v + 1 < b ? v + 1 : a, p = v > a ? v - 1 : b - 1;
                const int32_t x = xy[2 * v], y = xy[2 * v + 1], xn = xy[2 * n], yn = xy[2 * n + 1], xp = xy[2 * p], yp = xy[2 * p + 1];
                REQUIRE(x >= 0 && x <= W && y >= 0 && y <= H);
                REQUIRE((x == xn) != (y == yn));                                 // axis-parallel, not degenerate
                REQUIRE((x == xn) != (x == xp));                                 // a turn at every vertex: no collinear one is left
                repeated += !seen.insert({x, y}).second;
                REQUIRE(y > xy[2 * a + 1] || (y == xy[2 * a + 1] && x >= xy[2 * a]));   // it starts at its smallest (y, x)
                s += (long long)x * yn - (long long)xn * y;
            }
            REQUIRE(repeated <= (b - a) / 4);                                    // a ring may touch itself at a corner, never run along itself
            area2[t.ring_label[r]] -= s;                                         // counterclockwise on a north-up map: negative with y down
        }
        for (const auto& kv : pixels) REQUIRE(area2[kv.first] == 2 * kv.second);  // exteriors minus holes: the label's pixels
        REQUIRE(area2.size() == pixels.size());
    }
    printf("ok\n");
    return 0;
}

int main(int argc, char** argv) { return argc > 1 ? from_file(argv[1]) : self_checks(); }
