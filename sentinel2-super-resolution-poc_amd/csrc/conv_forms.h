// Which instantiation of conv_trunk_f16, conv_trunk_f8 (conv_trunk.hip) and conv3x3_f16 (conv3x3.hip) a launch takes: one table
// row per instantiation the library carries, and the picks that turn a launch's plain numbers into a row.  The launchers are
// generated from the tables (entry I instantiates the kernel of row I), so a form exists exactly when it has a row here.
// Plain C++, no device code and no HIP header: tests/native/conv_forms_main.cpp sweeps the picks under the address and
// undefined-behaviour sanitizers, and tests/test_conv_forms_cpu.py holds them to tests/forms_model.py.
#pragma once
#include <stdint.h>

#include "../../include/s2sr.h"

namespace s2sr {

enum Epilogue : int {
    EPI_LRELU = 0,      // y = lrelu(acc)                  -> fp16 blocks        (RDB conv1..4, up1, up2, hr)
    EPI_RDB5 = 1,       // v = acc*0.2 + (x+lo)            -> fp16 x_next, lo    (RDB conv5, rdb1/rdb2)
    EPI_RDB5_RRDB = 2,  // v = (acc*0.2+(x+lo))*0.2 + R; R=v-> fp16 x_next, lo    (RDB conv5 of rdb3)
    EPI_FIRST = 3,      // v = acc*in_scale + bias; F=R=v  -> fp16 x, lo          (conv_first)
    EPI_BODY = 4,       // v = F + acc                     -> fp16               (conv_body + trunk skip)
    EPI_LAST = 5,       // out fp32 NCHW and/or u8 NHWC (x255, clip, truncate)   (conv_last)
    EPI_DEBUG = 6,      // out fp32 NCHW, all Cout, optional lrelu               (s2sr_debug_conv)
    // SRVGGNetCompact (S2SR_ARCH_COMPACT): per-channel PReLU, pixel-shuffle tail
    EPI_PRELU = 7,      // y = prelu(acc, slope[c])        -> fp16 blocks        (compact body convs)
    EPI_CFIRST = 8,     // y = prelu(acc*in_scale + bias)  -> fp16 blocks        (compact first conv; no lo / R / F)
    EPI_CLAST = 9,      // pixel_shuffle(acc, 4) + x/255 -> fp32 NCHW and/or u8 NHWC at 4x (compact last conv, rows permuted on the host)
};

// conv kernel (conv3x3.hip): one enumerator per family of instantiations.  The loader decides a conv's form once (engine.hip,
// ConvW::form); pick_tail_form only adds the whole-patch (FULL) variant, which depends on the launch's geometry, and refuses
// parameters that do not fit the form.
enum ConvForm : int {
    CF_NONE = 0,                                    // not a launch_conv conv
    CF_FIRST, CF_BODY, CF_HR, CF_LAST,              // 8 waves, 16x32 patches, fp16 (conv_first in hp mode too: [w_hi][w_lo] on exact integers)
    // split-operand (hp) convs, cin 64: fp16 main term + e4m3 correction planes in; body / hr write such planes as well
    CF_BODY_SPLIT, CF_HR_SPLIT,
    CF_HR_SPLIT_NOHI,                               // conv_hr in front of a folded conv_last: no e4m3(x_hi) planes out
    CF_LAST_SPLIT8, CF_LAST_FOLD,                   // conv_last on all four planes (8 stages) / w_lo folded into idle couts (6 stages)
    CF_PRELU, CF_CFIRST, CF_CLAST,                  // SRVGGNetCompact: PReLU / pixel-shuffle epilogues
    CF_DEBUG1, CF_DEBUG1_UP, CF_DEBUG2, CF_DEBUG2_UP,   // s2sr_debug_conv: 1 or 2 cout tiles, plain or nearest-2x on load
};

// The host-only switches the picks read.  The engine hands them to the launchers next to the kernel arguments, never inside them.
struct FormSwitches {
    bool small8 = true;      // S2SR_SMALL8=0: single tiles keep the 16x32-patch forms of the fp16 RDB convs instead of 8x32
    bool f16_full = true;    // S2SR_F16_FULL=0: never the whole-patch (FULL) forms: the generic epilogue everywhere
};

// A pick answers a row index, or one of these (the launchers turn them into hipErrorNotSupported / hipErrorInvalidValue).
constexpr int kFormNotSupported = -1;   // not a form of this library (a removed form's hook number, not a trunk conv)
constexpr int kFormInvalid = -2;        // a form of the library that these parameters do not fit

// ------------------------------------------------------------------------------------------
// The RRDB trunk convs (conv_trunk.hip)
// ------------------------------------------------------------------------------------------
// One row = one instantiation; the fields are those of s2sr_debug_trunk_form (include/s2sr.h), which trunk_form_record fills
// from the row.  kernel 1: conv_trunk_f16<ct, rows / 4, ring, epi, full, pl>; kernel 2: conv_trunk_f8<ct, rows / 4, ring, epi,
// npl, prod> (its record says pl 2: a pair-step takes two planes).  hook: the public number that names the row
// (s2sr_debug_conv_trunk's `form`), 0 = none.  A hook number belongs to the rows of one (kernel, ct) class: conv1-4 answer to
// 1, 2, 5, 6, 7, 8, 10, conv5 to 1, 5, 10, the fp8 rows to none.
struct TrunkForm {
    int id;          // the row's TrunkRow name == its index
    int kernel, ct, rows, ring, full, pl, prod, npl, epi;
    int hook;
};
enum TrunkRow : int {
    TF_16, TF_32, TF_8,                              // conv1-4, generic epilogue (px_live): 16x32, 32x32, 8x32 patches
    TF_32_WHOLE, TF_16_WHOLE, TF_8_WHOLE,            // FULL 1: whole patches, no mosaic
    TF_16_EXTENT, TF_32_EXTENT,                      // FULL 3: ragged, no mosaic: the extent test alone
    TF_32_MOS276,                                    // FULL 2: mosaics of 276-pixel windows (tile 256, pad 10)
    TF_8X2_WHOLE, TF_8X2_EXTENT,                     // 8x32 patches, two planes per stage
    TF_C5_8X2, TF_C5_8X2_RRDB,                       // conv5 (the _RRDB row of a pair follows its EPI_RDB5 row)
    TF_C5_8, TF_C5_8_RRDB,
    TF_C5_16, TF_C5_16_RRDB,
    TF8_RESIDENT, TF8_STREAMED,                      // fp8 conv1-3 (weights resident in LDS) / conv4 (streamed), loader wave
    TF8_C5, TF8_C5_RRDB,
    TF_COUNT
};
inline constexpr TrunkForm kTrunkForms[TF_COUNT] = {
    //  id              kernel ct rows ring full pl prod npl epi            hook
    {TF_16,             1, 1, 16, 5, 0, 1, 0, 0, EPI_LRELU,      1},
    {TF_32,             1, 1, 32, 3, 0, 1, 0, 0, EPI_LRELU,      2},
    {TF_8,              1, 1,  8, 7, 0, 1, 0, 0, EPI_LRELU,      5},
    {TF_32_WHOLE,       1, 1, 32, 3, 1, 1, 0, 0, EPI_LRELU,      6},   // the whole-patch forms answer invalid-value on ragged sizes / mosaics
    {TF_16_WHOLE,       1, 1, 16, 5, 1, 1, 0, 0, EPI_LRELU,      7},
    {TF_8_WHOLE,        1, 1,  8, 7, 1, 1, 0, 0, EPI_LRELU,      8},
    {TF_16_EXTENT,      1, 1, 16, 5, 3, 1, 0, 0, EPI_LRELU,      0},
    {TF_32_EXTENT,      1, 1, 32, 3, 3, 1, 0, 0, EPI_LRELU,      0},
    {TF_32_MOS276,      1, 1, 32, 3, 2, 1, 0, 0, EPI_LRELU,      0},
    {TF_8X2_WHOLE,      1, 1,  8, 3, 1, 2, 0, 0, EPI_LRELU,      0},
    {TF_8X2_EXTENT,     1, 1,  8, 3, 3, 2, 0, 0, EPI_LRELU,      10},
    {TF_C5_8X2,         1, 2,  8, 2, 0, 2, 0, 0, EPI_RDB5,       10},  // double-buffered
    {TF_C5_8X2_RRDB,    1, 2,  8, 2, 0, 2, 0, 0, EPI_RDB5_RRDB,  10},
    {TF_C5_8,           1, 2,  8, 5, 0, 1, 0, 0, EPI_RDB5,       5},
    {TF_C5_8_RRDB,      1, 2,  8, 5, 0, 1, 0, 0, EPI_RDB5_RRDB,  5},
    {TF_C5_16,          1, 2, 16, 4, 0, 1, 0, 0, EPI_RDB5,       1},
    {TF_C5_16_RRDB,     1, 2, 16, 4, 0, 1, 0, 0, EPI_RDB5_RRDB,  1},
    {TF8_RESIDENT,      2, 1, 16, 6, 0, 2, 1, 4, EPI_LRELU,      0},
    {TF8_STREAMED,      2, 1, 16, 6, 0, 2, 1, 0, EPI_LRELU,      0},
    {TF8_C5,            2, 2, 16, 4, 0, 2, 0, 0, EPI_RDB5,       0},
    {TF8_C5_RRDB,       2, 2, 16, 4, 0, 2, 0, 0, EPI_RDB5_RRDB,  0},
};
constexpr bool trunk_rows_in_order() {
    for (int i = 0; i < TF_COUNT; ++i)
        if (kTrunkForms[i].id != i) return false;
    return true;
}
static_assert(trunk_rows_in_order(), "kTrunkForms is written in TrunkRow order");

// the record s2sr_debug_trunk_taps returns per launch (loe: 1, conv_trunk_f16's one lo encoding; wv: the MFMA waves)
inline s2sr_debug_trunk_form trunk_form_record(const TrunkForm& f) {
    return s2sr_debug_trunk_form{f.kernel, f.ct, f.rows, f.ring, f.full, f.pl, f.prod, 0, f.kernel == 1 ? 1 : 0, 4, f.npl, f.epi};
}

struct TrunkQuery {
    int N, H, W;                             // the launch's images and their live extent
    int mos_py, mos_ry, mos_px, mos_rx;      // window mosaic (ConvParams), all 0 = off
    int ct, epi;                             // cout tiles and epilogue: (1, EPI_LRELU) conv1-4, (2, EPI_RDB5 / EPI_RDB5_RRDB) conv5
    bool fp8;                                // conv_trunk_f8 (S2SR_PREC_FP8), else conv_trunk_f16
    int nstage;                              // planes per patch (fp8: padded to an even count)
    FormSwitches sw;
    int hook;                                // s2sr_debug_conv_trunk's form number, 0 = by launch size
};

// the row of this (kernel, ct, epi) class that answers to `hook`, or kFormNotSupported
constexpr int trunk_row_of_hook(int kernel, int ct, int epi, int hook) {
    for (int i = 0; i < TF_COUNT; ++i) {
        const TrunkForm& f = kTrunkForms[i];
        if (hook != 0 && f.hook == hook && f.kernel == kernel && f.ct == ct && f.epi == epi) return i;
    }
    return kFormNotSupported;
}

// Returns a row of kTrunkForms, or kFormNotSupported: not a trunk conv, or a hook number no row of the conv's class answers to.
// What a row then refuses for the launch's geometry (a whole-patch form on a ragged size or a mosaic, FULL 2 off the 277 / 276
// mosaic, FULL 3 with a mosaic, a plane count that is no multiple of pl) its launcher answers with hipErrorInvalidValue.
inline int pick_trunk_form(const TrunkQuery& q) {
    const bool conv14 = q.ct == 1 && q.epi == EPI_LRELU, conv5 = q.ct == 2 && (q.epi == EPI_RDB5 || q.epi == EPI_RDB5_RRDB);
    if (q.fp8) {
        // The loader-wave form (conv_trunk_f8 PROD) is the one fp8 conv1-4 form, so a hook number is refused: conv1-3 keep their
        // weights resident in LDS (<= 4 planes incl. a phantom, next to the 6-slot slab ring), conv4 streams them (6 planes would
        // cost two slab slots).  The other forms the measurements buried: four waves without the loader (-3 %),
        // all weights streamed or all resident (+-1 %), two waves per SIMD.
        if (conv14) return q.hook != 0 ? kFormNotSupported : q.nstage <= 4 ? TF8_RESIDENT : TF8_STREAMED;
        if (conv5) return q.epi == EPI_RDB5 ? TF8_C5 : TF8_C5_RRDB;      // one form: the hook is not looked at
        return kFormNotSupported;
    }
    if (q.hook == 4) return kFormNotSupported;               // the loader wave: the forms the measurements buried are refused
    const long cols = (q.W + 31) / 32;
    if (conv14) {
        if (const int named = trunk_row_of_hook(1, 1, EPI_LRELU, q.hook); named >= 0) return named;   // per-layer parity hook: name the patch form
        if (q.hook == 3 || q.hook == 9 || q.hook == 11) return kFormNotSupported;   // Winograd, weights from global, 64x32
        // (any other number picks by launch size, like 0)
        // 32x32 patches (8 rows per wave, 3-deep ring) unless that leaves most CUs without a patch (single tiles):
        // then 16x32 patches (4 rows per wave, 5-deep ring) spread the image over twice as many workgroups.  Both
        // forms accumulate in the same order, so the result does not depend on the choice.
        const long n32 = cols * ((q.H + 31) / 32) * q.N;
        // ... and 8x32 patches (2 rows per wave, 7-deep ring) for a single tile: 256 patches for 256 CUs instead of 128 (one 256x256 tile
        // is launch-bound: 351 dependent launches; S2SR_SMALL8=0 keeps the 16x32 form)
        const bool full = q.mos_py == 0 && q.H % 32 == 0 && q.W % 32 == 0 && q.sw.f16_full;   // whole patches only
        const bool plain = q.mos_py == 0 && q.sw.f16_full;                                   // ragged, but no mosaic: the extent test alone
        if (n32 < 96 && q.sw.small8)
            // two planes per stage (double-buffered) where the epilogue needs no mosaic test: half the barriers per patch
            // (profiles/r04_latency_anatomy.txt); the 7-deep one-plane ring otherwise
            return full ? TF_8X2_WHOLE : plain ? TF_8X2_EXTENT : TF_8;
        if (n32 < 192) return full ? TF_16_WHOLE : plain ? TF_16_EXTENT : TF_16;
        if (full) return TF_32_WHOLE;
        if (plain) return TF_32_EXTENT;
        if (q.sw.f16_full && q.mos_py == 277 && q.mos_ry == 276 && q.mos_px == 277 && q.mos_rx == 276) return TF_32_MOS276;
        return TF_32;
    }
    // conv5: 16x32 patches (4 rows per wave, 4-deep ring); single tiles take 8x32 patches, two planes per stage on a double-buffered
    // ring: one 256x256 tile is 128 patches of 16x32 -- half the CUs idle through twelve MFMA-bound stages (r04 kernel trace: 24 us
    // per conv5 launch, 69 of them = 37 % of one tile's latency) -- and 256 of 8x32.  Same accumulation order, same bytes.
    // (No whole-patch form here: <2, 4, 4, EPI, FULL = 1> was measured at 221.8 -> 220.2 us and 247.9 -> 246.1 us per headline launch,
    // 0.3 % of a step and inside the step's repeat spread -- DESIGN.md section 9, profiles/serpentine_bench.txt.)
    if (conv5) {
        if (q.hook != 0) return trunk_row_of_hook(1, 2, q.epi, q.hook);          // 1, 5, 10; anything else (the removed 2 among them) is refused
        const long n16 = cols * ((q.H + 15) / 16) * q.N;
        const bool small = n16 < 192 && q.sw.small8;
        return (small ? TF_C5_8X2 : TF_C5_16) + (q.epi == EPI_RDB5_RRDB ? 1 : 0);
    }
    return kFormNotSupported;
}

// ------------------------------------------------------------------------------------------
// Head, tail and compact convs (conv3x3.hip)
// ------------------------------------------------------------------------------------------
// One row = one instantiation conv3x3_f16<ct, np, waves, epi, up, ring, hpo, occ, f8, ph, full>.  form: the ConvForm the row serves;
// CF_NONE: a sub-pixel up-conv row (ph = its output row parity).  full: the whole-patch variant (no ragged edge, no mosaic).
struct TailForm {
    int form, ct, epi;
    bool up;
    int waves, np, ring, hpo, occ;
    bool f8;
    int ph;
    bool full;
};
inline constexpr TailForm kTailForms[] = {
    // the generic form: 8 waves x 2 rows (16x32 patches), a 5-deep ring for one cout tile, 4-deep for two
    //  form           ct epi          up     waves np ring hpo occ f8     ph  full
    {CF_FIRST,         2, EPI_FIRST,  false, 8, 2, 4, 0, 1, false, -1, false},
    {CF_BODY,          2, EPI_BODY,   false, 8, 2, 4, 0, 1, false, -1, false},
    {CF_HR,            2, EPI_LRELU,  false, 8, 2, 4, 0, 1, false, -1, false},
    {CF_LAST,          1, EPI_LAST,   false, 8, 2, 5, 0, 1, false, -1, false},
    // SRVGGNetCompact: the same 8-wave, 16x32-patch form with the PReLU / pixel-shuffle epilogues
    {CF_PRELU,         2, EPI_PRELU,  false, 8, 2, 4, 0, 1, false, -1, false},
    {CF_CFIRST,        2, EPI_CFIRST, false, 8, 2, 4, 0, 1, false, -1, false},
    {CF_CLAST,         2, EPI_CLAST,  false, 8, 2, 4, 0, 1, false, -1, false},
    {CF_DEBUG1,        1, EPI_DEBUG,  false, 8, 2, 5, 0, 1, false, -1, false},
    {CF_DEBUG1_UP,     1, EPI_DEBUG,  true,  8, 2, 5, 0, 1, false, -1, false},
    {CF_DEBUG2,        2, EPI_DEBUG,  false, 8, 2, 4, 0, 1, false, -1, false},
    {CF_DEBUG2_UP,     2, EPI_DEBUG,  true,  8, 2, 4, 0, 1, false, -1, false},
    // split-operand forms (hpo: which e4m3 planes the epilogue writes; conv_last: 3 = the folded 6-stage schedule, 0 = the 8-stage one)
    {CF_BODY_SPLIT,    2, EPI_BODY,   false, 8, 2, 4, 1, 1, true,  -1, false},
    {CF_BODY_SPLIT,    2, EPI_BODY,   false, 8, 2, 4, 1, 1, true,  -1, true},
    {CF_HR_SPLIT,      2, EPI_LRELU,  false, 8, 2, 4, 1, 1, true,  -1, false},
    {CF_HR_SPLIT_NOHI, 2, EPI_LRELU,  false, 8, 2, 4, 2, 1, true,  -1, false},
    {CF_HR_SPLIT_NOHI, 2, EPI_LRELU,  false, 8, 2, 4, 2, 1, true,  -1, true},
    {CF_LAST_SPLIT8,   1, EPI_LAST,   false, 8, 2, 4, 0, 1, true,  -1, false},
    {CF_LAST_FOLD,     1, EPI_LAST,   false, 8, 2, 4, 3, 1, true,  -1, false},
    {CF_LAST_FOLD,     1, EPI_LAST,   false, 8, 2, 4, 3, 1, true,  -1, true},
    // sub-pixel up-convs, one row parity per launch: split-operand (8x32 source patches), then plain fp16 (the same four fp16
    // stages, no correction planes in or out)
    {CF_NONE,          4, EPI_LRELU,  false, 8, 1, 4, 1, 1, true,   0, true},
    {CF_NONE,          4, EPI_LRELU,  false, 8, 1, 4, 1, 1, true,   1, true},
    {CF_NONE,          4, EPI_LRELU,  false, 8, 1, 4, 1, 1, true,   0, false},
    {CF_NONE,          4, EPI_LRELU,  false, 8, 1, 4, 1, 1, true,   1, false},
    {CF_NONE,          4, EPI_LRELU,  false, 8, 2, 4, 0, 1, false,  0, false},
    {CF_NONE,          4, EPI_LRELU,  false, 8, 2, 4, 0, 1, false,  1, false},
};
constexpr int kTailFormCount = (int)(sizeof(kTailForms) / sizeof(kTailForms[0]));

struct TailQuery {
    int form;                  // ConvForm
    int H, W, mos_py;          // live extent of a launch image (the up-convs: of the source), mosaic period (0 = off)
    bool slope, src_lo;        // the launch brings PReLU slopes / a second operand tensor
    FormSwitches sw;
};

constexpr int tail_row(int form, int ph, bool f8, bool full) {
    for (int i = 0; i < kTailFormCount; ++i) {
        const TailForm& f = kTailForms[i];
        if (f.form == form && f.ph == ph && f.f8 == f8 && f.full == full) return i;
    }
    return kFormInvalid;
}

// the launch has whole patches of th x 32 and nothing else: no ragged edge, no mosaic separators (and the switch allows it)
constexpr bool whole_patches(int H, int W, int mos_py, int th, const FormSwitches& sw) {
    return mos_py == 0 && H % th == 0 && W % 32 == 0 && sw.f16_full;
}

// launch_conv: the row of q.form -- its whole-patch variant where the form has one and the launch has nothing but whole 16x32
// patches -- or kFormInvalid: CF_NONE / not a ConvForm, or the operand the form's epilogue reads is missing.
inline int pick_tail_form(const TailQuery& q) {
    if (q.form == CF_NONE) return kFormInvalid;   // the RDB convs run on conv_trunk.hip, the up-convs in sub-pixel form (pick_phase_form)
    if ((q.form == CF_PRELU || q.form == CF_CFIRST) && !q.slope) return kFormInvalid;
    if (q.form == CF_CLAST && !q.src_lo) return kFormInvalid;
    const bool f8 = q.form >= CF_BODY_SPLIT && q.form <= CF_LAST_FOLD;   // the split-operand forms
    if (whole_patches(q.H, q.W, q.mos_py, 16, q.sw))
        if (const int r = tail_row(q.form, -1, f8, true); r >= 0) return r;
    return tail_row(q.form, -1, f8, false);
}

// launch_conv_phase: one ROW parity py of an up-conv in sub-pixel form; H, W = source dims.  The split-operand form takes whole
// 8x32 source patches where the launch has nothing else.
inline int pick_phase_form(int py, bool f8, int H, int W, int mos_py, const FormSwitches& sw) {
    if (py != 0 && py != 1) return kFormInvalid;
    return tail_row(CF_NONE, py, f8, f8 && whole_patches(H, W, mos_py, 8, sw));
}

}  // namespace s2sr
