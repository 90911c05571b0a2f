// Stand-alone driver of csrc/blend_plan.h (the host code that builds and range-checks the tables the seam-blended stitch indexes
// window tiles with), built with -fsanitize=address,undefined by tests/test_blend_cpu.py.  Maps and tables live in exact-size heap
// blocks, so a read or write past one is reported.  The paste map of an axis is rebuilt here from the window rule of
// s2sr_plan_tiles (far edge first, near edge pulled in, halo cropped on every side with a neighbour, later windows overwrite).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "band_plan.h"
#include "blend_plan.h"

using namespace s2sr;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Axis {
    std::vector<int32_t> map;      // 2 per output coordinate: distinct window, offset inside its output
    int nwin = 0, ext = 0;
    int64_t n = 0;
};

static Axis paste_axis(int len, int tile, int pad, int scale) {
    Axis a;
    const int K = (len + tile - 1) / tile, win = tile + 2 * pad;
    a.n = (int64_t)len * scale;
    a.map.assign(2 * (size_t)a.n, -1);
    int prev_start = -1;
    for (int k = 0; k < K; ++k) {
        const int end = k * tile + win < len ? k * tile + win : len, start = end - win > 0 ? end - win : 0;
        if (start != prev_start) { ++a.nwin; prev_start = start; }
        a.ext = (end - start) * scale;
        const int o1 = start * scale + (k > 0 ? pad * scale : 0), o2 = end * scale - (k < K - 1 ? pad * scale : 0);
        for (int o = o1; o < o2; ++o) { a.map[2 * (size_t)o] = a.nwin - 1; a.map[2 * (size_t)o + 1] = o - start * scale; }
    }
    return a;
}

int main() {
    long seams = 0, shortened = 0;
    for (int tile : {8, 16, 256})
        for (int pad : {0, 2, 3, 10})
            for (int scale : {2, 4})
                for (int len = 1; len <= (tile == 256 ? 3 : 6) * tile + 1; len += tile == 256 ? 7 : 1) {
                    const Axis a = paste_axis(len, tile, pad, scale);
                    std::vector<int32_t> tab((size_t)kBlendStride * a.n);
                    const char* why = blend_plan_axis(a.map.data(), a.n, a.nwin, a.ext, pad * scale, tab.data());
                    bool hole = false;            // pad > tile / 2 on an image shorter than two pads: the plan leaves pixels uncovered
                    for (int64_t o = 0; o < a.n; ++o) hole = hole || a.map[2 * o] < 0;
                    EXPECT((why == nullptr) == !hole && (!hole || 2 * pad > tile));
                    if (why) { if (!hole) printf("  tile %d pad %d scale %d len %d: %s\n", tile, pad, scale, len, why); continue; }
                    EXPECT(blend_check_axis(tab.data(), a.n, a.nwin, a.ext) == nullptr);
                    EXPECT(blend_check_band(tab.data(), 0, a.n, 0, a.nwin) == nullptr);
                    for (int64_t o = 0; o < a.n; ++o) {
                        const int32_t* e = &tab[kBlendStride * o];
                        if (e[4] == 0) { EXPECT(e[0] == a.map[2 * o] && e[1] == a.map[2 * o + 1] && e[5] == 1); continue; }
                        EXPECT(pad > 0 && e[2] == e[0] + 1 && e[5] % 4 == 0 && e[5] <= 4 * pad * scale && (e[4] & 1));
                        if (e[4] == 1) { ++seams; shortened += e[5] < 4 * pad * scale; }
                    }
                    std::vector<int32_t> dev = tab;
                    blend_device_axis(dev.data(), a.n);
                    for (int64_t o = 0; o < a.n; ++o) {
                        float w;
                        memcpy(&w, &dev[kBlendStride * o + 4], 4);
                        EXPECT(w >= 0.f && w < 1.f && (w == 0.f) == (tab[kBlendStride * o + 4] == 0) && dev[kBlendStride * o + 5] == 0);
                    }
                }
    EXPECT(seams > 1000 && shortened > 50);
    {
        // refusals: the good axis of 200 LR pixels at 16 / 3, scale 4, then one thing wrong at a time
        const Axis a = paste_axis(200, 16, 3, 4);
        std::vector<int32_t> tab((size_t)kBlendStride * a.n);
        EXPECT(blend_plan_axis(a.map.data(), a.n, a.nwin, a.ext, 12, tab.data()) == nullptr);
        Axis b = a;
        b.map[2 * 77] = -1;                                        // an uncovered pixel
        EXPECT(blend_plan_axis(b.map.data(), b.n, b.nwin, b.ext, 12, tab.data()) != nullptr);
        b = a; b.map[2 * 77] = a.nwin;                             // a window beyond the job
        EXPECT(blend_plan_axis(b.map.data(), b.n, b.nwin, b.ext, 12, tab.data()) != nullptr);
        b = a; b.map[2 * 77 + 1] = a.ext;                          // an offset beyond the window
        EXPECT(blend_plan_axis(b.map.data(), b.n, b.nwin, b.ext, 12, tab.data()) != nullptr);
        b = a; b.map[2 * 77 + 1] = -1;
        EXPECT(blend_plan_axis(b.map.data(), b.n, b.nwin, b.ext, 12, tab.data()) != nullptr);
        EXPECT(blend_plan_axis(a.map.data(), a.n, a.nwin, a.ext, -1, tab.data()) != nullptr);
        EXPECT(blend_plan_axis(a.map.data(), 0, a.nwin, a.ext, 12, tab.data()) != nullptr);
        EXPECT(blend_plan_axis(nullptr, a.n, a.nwin, a.ext, 12, tab.data()) != nullptr);
        // windows without a halo pasted edge to edge, asked for a ramp: it would read before the second window's first row
        Axis c;
        c.n = 64; c.nwin = 2; c.ext = 32;
        c.map.resize(128);
        for (int o = 0; o < 64; ++o) { c.map[2 * o] = o / 32; c.map[2 * o + 1] = o % 32; }
        std::vector<int32_t> tc((size_t)kBlendStride * c.n);
        EXPECT(blend_plan_axis(c.map.data(), c.n, c.nwin, c.ext, 4, tc.data()) != nullptr);
        EXPECT(blend_plan_axis(c.map.data(), c.n, c.nwin, c.ext, 0, tc.data()) == nullptr);
        // a ramp wider than INT32 arithmetic would like: half-widths are cut to the seam distances first
        EXPECT(blend_plan_axis(c.map.data(), c.n, c.nwin, c.ext, INT32_MAX, tc.data()) != nullptr);
        // the table checks, one entry wrong at a time
        EXPECT(blend_plan_axis(a.map.data(), a.n, a.nwin, a.ext, 12, tab.data()) == nullptr);
        for (int f = 0; f < 6; ++f)
            for (int32_t bad : {(int32_t)-1, (int32_t)INT32_MAX, (int32_t)INT32_MIN}) {
                if (f == 5 && bad == INT32_MAX && tab[kBlendStride * 300 + 4] == 0) continue;   // 0 / anything positive is still weight 0
                std::vector<int32_t> t = tab;
                t[kBlendStride * 300 + f] = bad;
                EXPECT(blend_check_axis(t.data(), a.n, a.nwin, a.ext) != nullptr);
            }
        std::vector<int32_t> t = tab;
        t[kBlendStride * 10 + 2] = 1;                              // two windows where no ramp is
        EXPECT(t[kBlendStride * 10 + 4] == 0 && blend_check_axis(t.data(), a.n, a.nwin, a.ext) != nullptr);
        // bands: rows of window 1 are not in a buffer that holds window 0 only, nor in one that starts at window 2
        EXPECT(blend_check_band(tab.data(), 0, a.n, 0, 1) != nullptr && blend_check_band(tab.data(), 0, a.n, 2, a.nwin) != nullptr);
        EXPECT(blend_check_band(tab.data(), 0, 8, 0, 1) == nullptr && blend_check_band(tab.data(), 5, 5, 7, 7) == nullptr);
        // the bands of every cut of the axis' windows into two and three chunks (band_plan.h), over the paste map and over the
        // table's later window: in order, up to the axis' end (also when the output is cropped by a row), inside their chunk's buffer
        for (int r1 = 1; r1 < a.nwin; ++r1)
            for (int r2 = r1; r2 < a.nwin; ++r2)
                for (int crop = 0; crop < 2; ++crop) {
                    std::vector<int> r0 = {0, r1};
                    if (r2 > r1) r0.push_back(r2);
                    r0.push_back(a.nwin);
                    const int nch = (int)r0.size() - 1, OH = (int)a.n - crop;
                    std::vector<int> end(nch), end_map(nch);
                    plan_bands(r0.data(), nch, a.nwin, OH, tab.data() + 2, kBlendStride, end.data());
                    plan_bands(r0.data(), nch, a.nwin, OH, a.map.data(), 2, end_map.data());
                    EXPECT(end[nch - 1] == OH && end_map[nch - 1] == OH);
                    for (int k = 0; k < nch; ++k) {
                        const int yb = k ? end[k - 1] : 0;
                        EXPECT(yb <= end[k] && end[k] <= end_map[k]);      // a ramp's rows wait for the later window
                        EXPECT(blend_check_band(tab.data(), yb, end[k], r0[k] - (k > 0), r0[k + 1]) == nullptr);
                    }
                }
    }
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("ok: %ld seams, %ld with a shortened ramp\n", seams, shortened);
    return 0;
}
