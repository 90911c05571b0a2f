// Host side of the fields pass (kernels: fields.hip): a uint16 label raster -> the rings around its labels, in
// pixel corners.  Plain host arithmetic, no HIP in here, so tests/native/ring_trace_main.cpp runs it under ASan / UBSan.
//
// The rule (tests/fields_model.py restates it):
//   corners      pixel (r, c) covers x in [c, c + 1], y in [r, r + 1]; x along columns, y along rows, from the raster's top-left
//   boundary     of label l: the unit pixel edges between a pixel of l and anything else; outside the raster is anything else
//   direction    each edge runs so that l's pixel lies on its left as seen on screen: down the pixel's left side, right along its
//                bottom, up its right side, left along its top.  Exterior rings then run counterclockwise on a north-up map (RFC
//                7946), holes clockwise
//   corners with two ways on: the walk turns left (then straight, then right): pixels of l that touch only diagonally get rings of
//                their own that touch.  Everything else is then 8-connected, so a ring MAY TOUCH ITSELF at a corner: two holes of
//                one label that meet at a corner are one ring through that corner twice, and a hole that meets the outside at a
//                corner is a notch of the exterior ring.  No ring crosses itself or runs along itself, every ring turns at every
//                vertex, and under the even-odd rule of zones.hip a label's rings burn back to exactly its pixels
//   vertices     collinear ones are dropped; a ring starts at its smallest (y, x) vertex (never a touching corner) and is not closed (last -> first is implied)
//   order        by label, then by start vertex (y, x).  Label 0 and labels above Z are not traced
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace s2sr {

struct RingTrace {
    std::vector<int32_t> xy;            // [V][2]: x, y
    std::vector<int32_t> ring_start;    // [R + 1] into xy
    std::vector<uint16_t> ring_label;   // [R]
};

// 0, or why not (the raster's size, more vertices than int32 starts can address)
inline const char* ring_trace(const uint16_t* labels, int H, int W, int Z, RingTrace* out) {
    out->xy.clear();
    out->ring_start.assign(1, 0);
    out->ring_label.clear();
    if (!labels) return "labels is required";
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return "H and W must be positive and H W < 2^31";
    if (Z < 1 || Z > 65535) return "Z must be in 1..65535";
    const auto at = [&](int r, int c) -> uint32_t { return r < 0 || c < 0 || r >= H || c >= W ? 0u : labels[(size_t)r * W + c]; };
    // the edge that leaves corner (x, y) in direction d (0 down, 1 right, 2 up, 3 left; d + 1 is the left turn) for label l
    const auto edge = [&](int x, int y, int d, uint32_t l) -> bool {
        switch (d) {
            case 0: return at(y, x) == l && at(y, x - 1) != l;            // the left side of pixel (y, x)
            case 1: return at(y - 1, x) == l && at(y, x) != l;            // the bottom of pixel (y - 1, x)
            case 2: return at(y - 1, x - 1) == l && at(y - 1, x) != l;    // the right side of pixel (y - 1, x - 1)
            default: return at(y, x - 1) == l && at(y - 1, x - 1) != l;   // the top of pixel (y, x - 1)
        }
    };
    static const int dx[4] = {0, 1, 0, -1}, dy[4] = {1, 0, -1, 0};
    struct Ring { uint32_t label; int32_t y, x; size_t first, count; };
    std::vector<Ring> rings;
    std::vector<int32_t> raw, one;                               // the rings' vertices as found; one ring
    std::vector<bool> seen((size_t)H * W, false);                // the pixel's top edge is part of a ring already
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            const uint32_t l = at(r, c);
            if (l < 1 || l > (uint32_t)Z || at(r - 1, c) == l || seen[(size_t)r * W + c]) continue;
            // every ring holds an edge that runs left: start on this one, (c + 1, r) -> (c, r)
            one.clear();
            int x = c + 1, y = r, d = 3;
            do {
                x += dx[d];
                y += dy[d];
                if (d == 3) seen[(size_t)y * W + x] = true;
                int nd = (d + 1) & 3;
                if (!edge(x, y, nd, l)) nd = d;
                if (nd == d && !edge(x, y, nd, l)) nd = (d + 3) & 3;
                if (nd != d) {
                    one.push_back(x);
                    one.push_back(y);
                }
                d = nd;
            } while (!(x == c + 1 && y == r && d == 3));
            const size_t n = one.size() / 2;
            size_t best = 0;
            for (size_t i = 1; i < n; ++i)
                if (one[2 * i + 1] < one[2 * best + 1] || (one[2 * i + 1] == one[2 * best + 1] && one[2 * i] < one[2 * best])) best = i;
            if (raw.size() / 2 + n > 0x7fffffffull) return "more than 2^31 - 1 vertices";
            rings.push_back(Ring{l, one[2 * best + 1], one[2 * best], raw.size() / 2, n});
            for (size_t i = 0; i < n; ++i) {
                raw.push_back(one[2 * ((best + i) % n)]);
                raw.push_back(one[2 * ((best + i) % n) + 1]);
            }
        }
    std::sort(rings.begin(), rings.end(), [](const Ring& a, const Ring& b) {
        return a.label != b.label ? a.label < b.label : a.y != b.y ? a.y < b.y : a.x < b.x;
    });
    out->xy.reserve(raw.size());
    for (const Ring& g : rings) {
        out->xy.insert(out->xy.end(), raw.begin() + 2 * g.first, raw.begin() + 2 * (g.first + g.count));
        out->ring_start.push_back((int32_t)(out->xy.size() / 2));
        out->ring_label.push_back((uint16_t)g.label);
    }
    return nullptr;
}

// The capacity protocol of s2sr_labels_trace_u16: counts = vertices, rings, always; the tables (xy [xy_cap][2], ring_start
// [ring_cap + 1], ring_label [ring_cap]) only when both capacities suffice.  True when they were written.
inline bool ring_trace_copy(const RingTrace& t, uint64_t xy_cap, uint64_t ring_cap, int32_t* xy, int32_t* ring_start, uint16_t* ring_label,
                            uint64_t* counts) {
    const uint64_t V = t.xy.size() / 2, R = t.ring_label.size();
    counts[0] = V;
    counts[1] = R;
    if (V > xy_cap || R > ring_cap || !xy || !ring_start || !ring_label) return false;
    std::copy(t.xy.begin(), t.xy.end(), xy);
    std::copy(t.ring_start.begin(), t.ring_start.end(), ring_start);
    std::copy(t.ring_label.begin(), t.ring_label.end(), ring_label);
    return true;
}

}  // namespace s2sr
