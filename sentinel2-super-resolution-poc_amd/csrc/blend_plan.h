// The blend plan of the seam-blended stitch (s2sr_enhance_blend_*): plain host arithmetic over a window job's paste maps, no HIP in
// here, so tests/native/blend_plan_main.cpp runs it under the address and undefined-behaviour sanitizers.
//
// One axis at a time.  The paste map of an axis holds, per output coordinate o, the window that owns o under the overwrite rule
// and o's offset inside that window's output (o - scale * start of the window).  A seam S is a coordinate whose owner differs from
// the owner of S - 1.  Around each seam lies a ramp of half-width r = min(pad * scale, half the distance to the previous seam or
// the axis start, half the distance to the next seam or the axis end); inside [S - r, S + r) the output cross-fades from window
// a = owner(S - 1) to window b = owner(S) with the weight of b  w = (2 (o - S + r) + 1) / (4 r), symmetric about the seam.
// The table has six ints per coordinate: {a, ia, b, ib, num, den}, ia / ib the offsets inside a's / b's output, w = num / den;
// outside every ramp a = b = owner, ia = ib, num = 0, den = 1.
#pragma once
#include <stdint.h>
#include <string.h>

namespace s2sr {

constexpr int kBlendStride = 6;

// Every entry of a table inside its window (offsets in [0, ext)) and every window inside the job (indices in [0, nwin)), weights
// in [0, 1).  nullptr when good, else what is wrong.
inline const char* blend_check_axis(const int32_t* tab, int64_t n, int nwin, int ext) {
    if (!tab || n <= 0 || nwin <= 0 || ext <= 0) return "blend plan: empty axis";
    for (int64_t o = 0; o < n; ++o) {
        const int32_t* e = tab + kBlendStride * o;
        if (e[0] < 0 || e[0] >= nwin || e[2] < 0 || e[2] >= nwin) return "blend plan: a window index outside the job";
        if (e[1] < 0 || e[1] >= ext || e[3] < 0 || e[3] >= ext) return "blend plan: a ramp reaches outside its window";
        if (e[5] <= 0 || e[4] < 0 || e[4] >= e[5]) return "blend plan: a weight outside [0, 1)";
        if (e[4] == 0 && (e[0] != e[2] || e[1] != e[3])) return "blend plan: two windows outside a ramp";
    }
    return nullptr;
}

// map: 2 ints per coordinate (window, offset), n coordinates; nwin distinct windows on the axis, each ext output pixels long;
// ramp = pad * scale.  Writes tab[6 n].  nullptr when good; a map or a ramp that leaves its windows is refused (the table is then
// not to be used).
inline const char* blend_plan_axis(const int32_t* map, int64_t n, int nwin, int ext, int ramp, int32_t* tab) {
    if (!map || !tab || n <= 0 || nwin <= 0 || ext <= 0 || ramp < 0) return "blend plan: empty axis";
    for (int64_t o = 0; o < n; ++o) {
        const int32_t w = map[2 * o], i = map[2 * o + 1];
        if (w < 0 || w >= nwin) return "blend plan: an output pixel no window of the job covers";
        if (i < 0 || i >= ext) return "blend plan: a paste offset outside its window";
        int32_t* e = tab + kBlendStride * o;
        e[0] = w; e[1] = i; e[2] = w; e[3] = i; e[4] = 0; e[5] = 1;
    }
    int64_t prev = 0;                                   // the seam before S (or the axis start)
    for (int64_t S = 1; S < n; ++S) {
        if (map[2 * S] == map[2 * (S - 1)]) continue;
        int64_t next = S + 1;                           // the seam after S (or the axis end)
        while (next < n && map[2 * next] == map[2 * (next - 1)]) ++next;
        int64_t r = ramp;
        if ((S - prev) / 2 < r) r = (S - prev) / 2;
        if ((next - S) / 2 < r) r = (next - S) / 2;
        const int32_t a = map[2 * (S - 1)], b = map[2 * S];
        const int64_t base_a = (S - 1) - map[2 * (S - 1) + 1], base_b = S - map[2 * S + 1];   // scale * start of a, of b
        for (int64_t o = S - r; o < S + r; ++o) {
            const int64_t ia = o - base_a, ib = o - base_b;
            if (ia < 0 || ia >= ext || ib < 0 || ib >= ext) return "blend plan: a ramp reaches outside its window";
            int32_t* e = tab + kBlendStride * o;
            e[0] = a; e[1] = (int32_t)ia; e[2] = b; e[3] = (int32_t)ib;
            e[4] = (int32_t)(2 * (o - S + r) + 1); e[5] = (int32_t)(4 * r);
        }
        prev = S;
    }
    return blend_check_axis(tab, n, nwin, ext);
}

// Rows [yb, ye) of a row table, pasted from a buffer that holds window rows [first, last): every a and b inside it.
inline const char* blend_check_band(const int32_t* rows, int64_t yb, int64_t ye, int first, int last) {
    for (int64_t o = yb; o < ye; ++o) {
        const int32_t* e = rows + kBlendStride * o;
        if (e[0] < first || e[0] >= last || e[2] < first || e[2] >= last) return "blend plan: a band reads a window row its chunk does not hold";
    }
    return nullptr;
}

// The table as the kernel reads it: num / den replaced by the fp32 weight's bits (one correctly rounded division) and a zero.
inline void blend_device_axis(int32_t* tab, int64_t n) {
    for (int64_t o = 0; o < n; ++o) {
        int32_t* e = tab + kBlendStride * o;
        const float w = (float)e[4] / (float)e[5];
        memcpy(&e[4], &w, 4);
        e[5] = 0;
    }
}

}  // namespace s2sr
