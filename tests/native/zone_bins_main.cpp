// Stand-alone driver of csrc/zone_bins.h (the host code that checks a caller's polygon tables and bins the features to the tiles the
// rasteriser walks), built with -fsanitize=address,undefined by tests/test_zones_cpu.py.  Tables and bins live in exact-size heap
// blocks, so a read or write past one is reported.
//
//   zone_bins <file>   the file holds whitespace-separated integers: the number of cases, then per case F Z H W V R, the 2 V
//                      coordinates, the R + 1 ring starts, the F + 1 feature starts and the F labels.  Per case the program prints
//                      "case <i> <tiles_x> <tiles_y> <dropped>" and one line per tile, "<tile>:" and its features.
//   zone_bins          the refusals of zone_check_tables, one thing wrong at a time, and the checks of zone_check_bins; prints "ok".
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "zone_bins.h"

using namespace s2sr;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Tables {
    std::vector<int32_t> xy, ring_start, feat_start;
    std::vector<uint16_t> label;
    int64_t F = 0, Z = 0, H = 0, W = 0;
    const char* check() const { return zone_check_tables(xy.data(), ring_start.data(), feat_start.data(), label.data(), F, Z, H, W); }
};

static bool read_case(FILE* f, Tables* t) {
    long long F, Z, H, W, V, R, v;
    if (fscanf(f, "%lld %lld %lld %lld %lld %lld", &F, &Z, &H, &W, &V, &R) != 6 || F < 0 || V < 0 || R < 0) return false;
    t->F = F; t->Z = Z; t->H = H; t->W = W;
    t->xy.resize((size_t)(2 * V));
    t->ring_start.resize((size_t)R + 1);
    t->feat_start.resize((size_t)F + 1);
    t->label.resize((size_t)F);
    for (auto& x : t->xy) { if (fscanf(f, "%lld", &v) != 1) return false; x = (int32_t)v; }
    for (auto& x : t->ring_start) { if (fscanf(f, "%lld", &v) != 1) return false; x = (int32_t)v; }
    for (auto& x : t->feat_start) { if (fscanf(f, "%lld", &v) != 1) return false; x = (int32_t)v; }
    for (auto& x : t->label) { if (fscanf(f, "%lld", &v) != 1) return false; x = (uint16_t)v; }
    return true;
}

static int print_cases(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { printf("cannot open %s\n", path); return 1; }
    int n = 0;
    if (fscanf(f, "%d", &n) != 1) { fclose(f); return 1; }
    for (int i = 0; i < n; ++i) {
        Tables t;
        if (!read_case(f, &t)) { printf("case %d: unreadable\n", i); fclose(f); return 1; }
        if (const char* why = t.check()) { printf("case %d refused: %s\n", i, why); fclose(f); return 1; }
        ZoneBins b;
        const char* why = zone_build_bins(t.xy.data(), t.ring_start.data(), t.feat_start.data(), t.F, t.H, t.W, &b);
        if (!why) why = zone_check_bins(b, t.F);
        if (why) { printf("case %d: %s\n", i, why); fclose(f); return 1; }
        printf("case %d %lld %lld %lld\n", i, (long long)b.tiles_x, (long long)b.tiles_y, (long long)b.dropped);
        for (size_t tile = 0; tile + 1 < b.start.size(); ++tile) {
            printf("%zu:", tile);
            for (uint32_t k = b.start[tile]; k < b.start[tile + 1]; ++k) printf(" %d", b.feat[k]);
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}

// two triangles and a square with a hole on a 70 x 130 grid
static Tables good() {
    Tables t;
    t.F = 3; t.Z = 5; t.H = 70; t.W = 130;
    t.xy = {0, 0, 5000, 0, 0, 5000,  20000, 100, 33000, 100, 33000, 17000,  100, 100, 30000, 100, 30000, 17000, 100, 17000,  900, 900, 2000, 900, 2000, 2000};
    t.ring_start = {0, 3, 6, 10, 13};
    t.feat_start = {0, 1, 2, 4};
    t.label = {1, 5, 2};
    return t;
}

int main(int argc, char** argv) {
    if (argc > 1) return print_cases(argv[1]);
    Tables g = good();
    EXPECT(g.check() == nullptr);
    ZoneBins b;
    EXPECT(zone_build_bins(g.xy.data(), g.ring_start.data(), g.feat_start.data(), g.F, g.H, g.W, &b) == nullptr);
    EXPECT(b.tiles_x == 3 && b.tiles_y == 2 && b.dropped == 0 && zone_check_bins(b, g.F) == nullptr);
    EXPECT(b.start.size() == 7 && b.feat.size() == b.start[6]);
    Tables t = g; t.H = 0; EXPECT(t.check() != nullptr);
    t = g; t.W = -1; EXPECT(t.check() != nullptr);
    t = g; t.H = 65536; t.W = 32768; EXPECT(t.check() != nullptr);              // H W = 2^31
    t = g; t.H = 65535; t.W = 32768; EXPECT(t.check() == nullptr);
    t = g; t.F = 0; EXPECT(t.check() != nullptr);
    t = g; t.Z = 0; EXPECT(t.check() != nullptr);
    t = g; t.Z = 65536; EXPECT(t.check() != nullptr);
    t = g; t.Z = 4; EXPECT(t.check() != nullptr);                                 // the label 5 lies above it
    t = g; t.label[1] = 0; EXPECT(t.check() != nullptr);
    t = g; t.feat_start[0] = 1; EXPECT(t.check() != nullptr);
    t = g; t.feat_start[2] = 0; EXPECT(t.check() != nullptr);                     // decreases
    t = g; t.ring_start[0] = 1; EXPECT(t.check() != nullptr);
    t = g; t.ring_start[2] = 2; EXPECT(t.check() != nullptr);                     // decreases
    t = g; t.ring_start[1] = 2; EXPECT(t.check() != nullptr);                     // a ring of 2 vertices
    t = g; t.xy[7] = kZoneCoordMax + 1; EXPECT(t.check() != nullptr);
    t = g; t.xy[8] = -kZoneCoordMax - 1; EXPECT(t.check() != nullptr);
    t = g; t.xy[7] = kZoneCoordMax; t.xy[8] = -kZoneCoordMax; EXPECT(t.check() == nullptr);
    EXPECT(zone_check_tables(nullptr, g.ring_start.data(), g.feat_start.data(), g.label.data(), g.F, g.Z, g.H, g.W) != nullptr);
    EXPECT(zone_check_tables(g.xy.data(), nullptr, g.feat_start.data(), g.label.data(), g.F, g.Z, g.H, g.W) != nullptr);
    EXPECT(zone_check_tables(g.xy.data(), g.ring_start.data(), nullptr, g.label.data(), g.F, g.Z, g.H, g.W) != nullptr);
    EXPECT(zone_check_tables(g.xy.data(), g.ring_start.data(), g.feat_start.data(), nullptr, g.F, g.Z, g.H, g.W) != nullptr);
    {
        // features without a ring are legal, meet no tile and are counted as dropped
        Tables e = g;
        e.F = 5;
        e.feat_start = {0, 1, 2, 4, 4, 4};
        e.label = {1, 5, 2, 3, 3};
        EXPECT(e.check() == nullptr);
        ZoneBins be;
        EXPECT(zone_build_bins(e.xy.data(), e.ring_start.data(), e.feat_start.data(), e.F, e.H, e.W, &be) == nullptr && be.dropped == 2);
        EXPECT(zone_check_bins(be, e.F) == nullptr);
    }
    {
        // the bins' own checks, one entry wrong at a time
        ZoneBins w = b;
        w.start[2] = w.start[1] - 1; EXPECT(w.start[1] == 0 || zone_check_bins(w, g.F) != nullptr);
        w = b; w.start[6] += 1; EXPECT(zone_check_bins(w, g.F) != nullptr);
        w = b; w.feat[0] = 3; EXPECT(zone_check_bins(w, g.F) != nullptr);
        w = b; w.feat[0] = -1; EXPECT(zone_check_bins(w, g.F) != nullptr);
        w = b; w.start.pop_back(); EXPECT(zone_check_bins(w, g.F) != nullptr);
        bool two = false;
        for (size_t k = 0; k + 1 < b.start.size(); ++k)
            if (b.start[k + 1] - b.start[k] >= 2 && !two) {
                w = b;
                w.feat[b.start[k] + 1] = w.feat[b.start[k]];
                EXPECT(zone_check_bins(w, g.F) != nullptr);                       // does not ascend
                two = true;
            }
        EXPECT(two);
    }
    {
        // spans at the extremes of the coordinate range and of the tile count
        int64_t t0, t1;
        zone_tile_span(-kZoneCoordMax, kZoneCoordMax, 3, &t0, &t1); EXPECT(t0 == 0 && t1 == 3);
        zone_tile_span(-kZoneCoordMax, -1, 3, &t0, &t1); EXPECT(t0 >= t1);
        zone_tile_span(-1, 0, 3, &t0, &t1); EXPECT(t0 == 0 && t1 == 1);
        zone_tile_span(16383, 16383, 3, &t0, &t1); EXPECT(t0 == 0 && t1 == 1);
        zone_tile_span(16384, 16384, 3, &t0, &t1); EXPECT(t0 == 1 && t1 == 2);
        zone_tile_span(3 * 16384, kZoneCoordMax, 3, &t0, &t1); EXPECT(t0 >= t1);
        zone_tile_span(-16384, -16384, 3, &t0, &t1); EXPECT(t0 >= t1);
    }
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
