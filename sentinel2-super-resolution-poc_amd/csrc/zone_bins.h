// Host side of the polygon rasteriser (kernel: zones.hip): the checks of the caller's tables and the binning of
// features to the tiles of the label grid.  Plain host arithmetic, no HIP in here, so tests/native/zone_bins_main.cpp runs it on
// exact-size heap tables under the address and undefined-behaviour sanitizers.
//
// Units.  Coordinates are int32 in 1/256 of a label pixel, x along columns, y along rows, from the grid's top-left corner; the
// centre of pixel (r, c) is (256 c + 128, 256 r + 128).  Every coordinate lies in [-2^29, 2^29].
//
// Tiles.  The H x W grid is cut into tiles of 64 x 64 pixels, tile (ty, tx) holding rows [64 ty, 64 ty + 64) and columns
// [64 tx, 64 tx + 64): in coordinate units the half-open square [16384 tx, 16384 tx + 16384) x [16384 ty, 16384 ty + 16384).  A
// feature is a CANDIDATE of every tile whose square its bounding box [xmin, xmax] x [ymin, ymax] (closed, over all its vertices)
// meets:  xmax >= 16384 tx  and  xmin < 16384 (tx + 1),  and the same in y.  A centre a feature holds lies inside the feature's
// bounding box, so a tile's candidates are a superset of the features that label a pixel of it.  A feature without a vertex, or
// whose box meets no tile, is dropped.  The bins are CSR: start[T + 1] (T = tiles_y * tiles_x, row-major) into feat[], the
// features of one tile in ascending order: counts, then a scan, then a fill.
#pragma once
#include <stdint.h>

#include <vector>

namespace s2sr {

constexpr int kZoneTile = 64;                       // pixels per tile side
constexpr int kZoneSub = 256;                       // coordinate units per pixel
constexpr int32_t kZoneCoordMax = 1 << 29;          // |x|, |y| <= 2^29: every product of the inside rule fits int64
constexpr int64_t kZoneTileUnits = (int64_t)kZoneTile * kZoneSub;

// What s2sr_zones_rasterize_u16 refuses before the device is touched.  nullptr when good, else what is wrong.
inline const char* zone_check_tables(const int32_t* xy, const int32_t* ring_start, const int32_t* feat_start, const uint16_t* label, int64_t F,
                                     int64_t Z, int64_t H, int64_t W) {
    if (H <= 0 || W <= 0) return "H and W must be positive";
    if (H * W > 0x7fffffffLL) return "the label grid is too large (H W must stay below 2^31)";
    if (F < 1 || F > 0x7fffffffLL) return "F must be at least 1";
    if (Z < 1 || Z > 65535) return "Z must be 1..65535";
    if (!xy || !ring_start || !feat_start || !label) return "xy, ring_start, feat_start and label are required";
    if (feat_start[0] != 0) return "feat_start must start at 0";
    for (int64_t f = 0; f < F; ++f) {
        if (feat_start[f + 1] < feat_start[f]) return "feat_start must not decrease";
        if (label[f] < 1 || label[f] > Z) return "a label outside 1..Z";
    }
    const int64_t R = feat_start[F];
    if (ring_start[0] != 0) return "ring_start must start at 0";
    for (int64_t r = 0; r < R; ++r) {
        if (ring_start[r + 1] < ring_start[r]) return "ring_start must not decrease";
        if (ring_start[r + 1] - ring_start[r] < 3) return "a ring of fewer than 3 vertices";
    }
    const int64_t V = ring_start[R];
    for (int64_t i = 0; i < 2 * V; ++i)
        if (xy[i] < -kZoneCoordMax || xy[i] > kZoneCoordMax) return "a coordinate outside +-2^29";
    return nullptr;
}

struct ZoneBins {
    int64_t tiles_x = 0, tiles_y = 0;
    std::vector<uint32_t> start;       // [tiles_y * tiles_x + 1]
    std::vector<int32_t> feat;         // [start.back()]
    int64_t dropped = 0;               // features that meet no tile
};

// the tiles [t0, t1) along one axis of `tiles` tiles that the closed interval [lo, hi] meets (t0 >= t1: none)
inline void zone_tile_span(int64_t lo, int64_t hi, int64_t tiles, int64_t* t0, int64_t* t1) {
    // hi >= 16384 t  <=>  t <= floor(hi / 16384);  lo < 16384 (t + 1)  <=>  t >= floor(lo / 16384)   (floor towards -inf)
    const int64_t a = lo >= 0 ? lo / kZoneTileUnits : -((-lo + kZoneTileUnits - 1) / kZoneTileUnits);
    const int64_t b = hi >= 0 ? hi / kZoneTileUnits : -((-hi + kZoneTileUnits - 1) / kZoneTileUnits);
    *t0 = a < 0 ? 0 : a;
    *t1 = b + 1 > tiles ? tiles : b + 1;
}

// Tables that zone_check_tables accepted -> bins.  nullptr when good; more than 2^31 - 1 candidates in all are refused.
inline const char* zone_build_bins(const int32_t* xy, const int32_t* ring_start, const int32_t* feat_start, int64_t F, int64_t H, int64_t W,
                                   ZoneBins* bins) {
    bins->tiles_x = (W + kZoneTile - 1) / kZoneTile;
    bins->tiles_y = (H + kZoneTile - 1) / kZoneTile;
    const int64_t T = bins->tiles_x * bins->tiles_y;
    bins->dropped = 0;
    int64_t total = 0;
    std::vector<int64_t> span((size_t)F * 4);                // per feature: tx0, tx1, ty0, ty1
    std::vector<uint64_t> count((size_t)T + 1, 0);
    for (int64_t f = 0; f < F; ++f) {
        int64_t* s = &span[(size_t)f * 4];
        s[0] = s[1] = s[2] = s[3] = 0;
        const int64_t v0 = ring_start[feat_start[f]], v1 = ring_start[feat_start[f + 1]];
        if (v0 < v1) {
            int32_t xmin = xy[2 * v0], xmax = xmin, ymin = xy[2 * v0 + 1], ymax = ymin;
            for (int64_t v = v0 + 1; v < v1; ++v) {
                const int32_t x = xy[2 * v], y = xy[2 * v + 1];
                xmin = x < xmin ? x : xmin; xmax = x > xmax ? x : xmax;
                ymin = y < ymin ? y : ymin; ymax = y > ymax ? y : ymax;
            }
            zone_tile_span(xmin, xmax, bins->tiles_x, &s[0], &s[1]);
            zone_tile_span(ymin, ymax, bins->tiles_y, &s[2], &s[3]);
        }
        if (s[0] >= s[1] || s[2] >= s[3]) {
            s[1] = s[0];                                      // an empty span: the fill skips it
            ++bins->dropped;
            continue;
        }
        total += (s[1] - s[0]) * (s[3] - s[2]);               // (each factor <= 2^25, F < 2^31: no overflow before the refusal)
        if (total > 0x7fffffffLL) return "the features meet more than 2^31 - 1 tiles in all";
        for (int64_t ty = s[2]; ty < s[3]; ++ty)
            for (int64_t tx = s[0]; tx < s[1]; ++tx) ++count[(size_t)(ty * bins->tiles_x + tx) + 1];
    }
    for (int64_t t = 0; t < T; ++t) count[(size_t)t + 1] += count[(size_t)t];
    bins->start.resize((size_t)T + 1);
    for (int64_t t = 0; t <= T; ++t) bins->start[(size_t)t] = (uint32_t)count[(size_t)t];
    bins->feat.assign((size_t)count[(size_t)T], -1);
    std::vector<uint32_t> at(bins->start.begin(), bins->start.end() - 1);
    for (int64_t f = 0; f < F; ++f) {                         // features ascend, so every tile's list does
        const int64_t* s = &span[(size_t)f * 4];
        for (int64_t ty = s[2]; ty < s[3]; ++ty)
            for (int64_t tx = s[0]; tx < s[1]; ++tx) bins->feat[at[(size_t)(ty * bins->tiles_x + tx)]++] = (int32_t)f;
    }
    return nullptr;
}

// What the kernel relies on: the starts ascend from 0 to feat.size(), and every tile's features ascend inside [0, F).
inline const char* zone_check_bins(const ZoneBins& b, int64_t F) {
    const size_t T = (size_t)(b.tiles_x * b.tiles_y);
    if (b.start.size() != T + 1 || b.start[0] != 0 || b.start[T] != b.feat.size()) return "zone bins: the starts do not span the list";
    for (size_t t = 0; t < T; ++t) {
        if (b.start[t + 1] < b.start[t]) return "zone bins: the starts decrease";
        for (uint32_t i = b.start[t]; i < b.start[t + 1]; ++i) {
            if (b.feat[i] < 0 || b.feat[i] >= F) return "zone bins: a feature outside the list";
            if (i > b.start[t] && b.feat[i] <= b.feat[i - 1]) return "zone bins: a tile's features do not ascend";
        }
    }
    return nullptr;
}

}  // namespace s2sr
