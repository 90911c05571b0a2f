"""The kernel-form rule of the conv launchers, restated in plain Python from the if-ladders that csrc/conv_forms.h replaced.

Transcribed from the last commit that carried the ladders (fc0ce7c); the line references below are to that commit's
csrc/conv_trunk.hip and csrc/conv3x3.hip.  tests/test_conv_forms_cpu.py holds the picks of conv_forms.h to this model over a
sweep; the model knows nothing of the tables' row order: it answers instantiations.

A trunk answer is the launch's form record (kernel, ct, rows, ring, full, pl, prod, npl, epi) -- what the launcher templates
wrote into s2sr_debug_trunk_form (conv_trunk.hip:722: conv_trunk_f16<CT, NP, R, EPI, FULL, PL> -> (1, CT, 4 NP, R, FULL, PL,
0, 0, EPI); conv_trunk.hip:1372: conv_trunk_f8<CT, NP, RS, EPI, NPL, PROD> -> (2, CT, 4 NP, RS, 0, 2, PROD, NPL, EPI)) -- or
NOT_SUPPORTED.  A tail answer is the template argument list of conv3x3.hip's launch_t, (CT, EPI, UP, WAVES, NP, R, HPO, OCC, F8,
PH, FULL), or INVALID.  What a chosen instantiation's launcher then refuses for the launch's geometry (conv_trunk.hip:702-705,
conv3x3.hip:904) is not part of the pick and not modelled.

One deliberate difference from that commit: fp16 conv5 with a hook number other than 0, 1, 5, 10 ran the 16x32 form
(conv_trunk.hip:1423-1430: `small` false, not 10); it is refused now, as conv1-4 refuse the removed numbers."""
from functools import lru_cache

NOT_SUPPORTED = "not supported"
INVALID = "invalid value"

EPI_LRELU, EPI_RDB5, EPI_RDB5_RRDB, EPI_FIRST, EPI_BODY, EPI_LAST, EPI_DEBUG, EPI_PRELU, EPI_CFIRST, EPI_CLAST = range(10)
(CF_NONE, CF_FIRST, CF_BODY, CF_HR, CF_LAST, CF_BODY_SPLIT, CF_HR_SPLIT, CF_HR_SPLIT_NOHI, CF_LAST_SPLIT8, CF_LAST_FOLD,
 CF_PRELU, CF_CFIRST, CF_CLAST, CF_DEBUG1, CF_DEBUG1_UP, CF_DEBUG2, CF_DEBUG2_UP) = range(17)


def f16(ct, np_, r, epi, full=0, pl=1):
    return (1, ct, 4 * np_, r, full, pl, 0, 0, epi)


def f8(ct, np_, rs, epi, npl=0, prod=0):
    return (2, ct, 4 * np_, rs, 0, 2, prod, npl, epi)


def trunk_geometry(N, H, W, mos):
    """What the ladders read of a launch's geometry.  mos: (mos_py, mos_ry, mos_px, mos_rx), all 0 = off."""
    n32 = ((W + 31) // 32) * ((H + 31) // 32) * N                 # conv_trunk.hip:1395
    n16 = ((W + 31) // 32) * ((H + 15) // 16) * N                 # conv_trunk.hip:1422
    whole32 = mos[0] == 0 and H % 32 == 0 and W % 32 == 0         # conv_trunk.hip:1398, without the switch
    return (n32 < 96, n32 < 192, n16 < 192, whole32, mos[0] == 0, tuple(mos) == (277, 276, 277, 276))


@lru_cache(maxsize=None)
def trunk_ladder(geometry, small8, f16_full, ct, epi, fp8, nstage, hook):
    n32_lt96, n32_lt192, n16_lt192, whole32, no_mosaic, mos276 = geometry
    if fp8:
        if ct == 1 and epi == EPI_LRELU:                          # conv_trunk.hip:1480-1485
            if hook != 0:                                         # engine_debug.hip:407 (kind == 3 && form != 0)
                return NOT_SUPPORTED
            return f8(1, 4, 6, EPI_LRELU, 4, 1) if nstage <= 4 else f8(1, 4, 6, EPI_LRELU, 0, 1)
        if ct == 2 and epi == EPI_RDB5:                           # conv_trunk.hip:1486 (no hook argument: kinds 4-5 ignore it)
            return f8(2, 4, 4, EPI_RDB5)
        if ct == 2 and epi == EPI_RDB5_RRDB:                      # conv_trunk.hip:1487
            return f8(2, 4, 4, EPI_RDB5_RRDB)
        return NOT_SUPPORTED                                      # conv_trunk.hip:1488
    if hook == 4:                                                 # conv_trunk.hip:1382
        return NOT_SUPPORTED
    if ct == 1 and epi == EPI_LRELU:                              # conv_trunk.hip:1383
        named = {1: f16(1, 4, 5, EPI_LRELU), 2: f16(1, 8, 3, EPI_LRELU), 5: f16(1, 2, 7, EPI_LRELU),          # :1384-1386
                 6: f16(1, 8, 3, EPI_LRELU, 1), 7: f16(1, 4, 5, EPI_LRELU, 1), 8: f16(1, 2, 7, EPI_LRELU, 1),  # :1387-1389
                 10: f16(1, 2, 3, EPI_LRELU, 3, 2)}                                                            # :1390
        if hook in named:
            return named[hook]
        if hook in (3, 9, 11):                                    # conv_trunk.hip:1391
            return NOT_SUPPORTED
        full = whole32 and f16_full                               # conv_trunk.hip:1398 (f16_form bit 2 = not f16_full)
        plain = no_mosaic and f16_full                            # conv_trunk.hip:1399
        if n32_lt96 and small8:                                   # conv_trunk.hip:1400 (f16_form bit 1 = not small8)
            if full:
                return f16(1, 2, 3, EPI_LRELU, 1, 2)              # :1403
            if plain:
                return f16(1, 2, 3, EPI_LRELU, 3, 2)              # :1404
            return f16(1, 2, 7, EPI_LRELU)                        # :1405
        if n32_lt192:                                             # conv_trunk.hip:1407-1409
            return f16(1, 4, 5, EPI_LRELU, 1) if full else f16(1, 4, 5, EPI_LRELU, 3) if plain else f16(1, 4, 5, EPI_LRELU)
        if full:
            return f16(1, 8, 3, EPI_LRELU, 1)                     # :1410
        if plain:
            return f16(1, 8, 3, EPI_LRELU, 3)                     # :1411
        if f16_full and mos276:                                   # conv_trunk.hip:1412
            return f16(1, 8, 3, EPI_LRELU, 2)
        return f16(1, 8, 3, EPI_LRELU)                            # :1414
    if ct == 2 and epi in (EPI_RDB5, EPI_RDB5_RRDB):              # conv_trunk.hip:1420
        if hook == 2:                                             # :1421
            return NOT_SUPPORTED
        if hook not in (0, 1, 5, 10):                             # the tightening (module docstring)
            return NOT_SUPPORTED
        small = hook == 5 or (hook == 0 and n16_lt192 and small8)  # :1423
        if hook == 10 or (small and hook == 0):                   # :1424-1426
            return f16(2, 2, 2, epi, 0, 2)
        return f16(2, 2, 5, epi) if small else f16(2, 4, 4, epi)  # :1429-1430
    return NOT_SUPPORTED                                          # conv_trunk.hip:1432


def trunk_pick(N, H, W, mos, small8, f16_full, ct, epi, fp8, nstage, hook):
    return trunk_ladder(trunk_geometry(N, H, W, mos), small8, f16_full, ct, epi, fp8, nstage, hook)


def _w(ct, epi, up):
    """launch_w, conv3x3.hip:927-930: the generic form, 8 waves x 2 rows"""
    return (ct, epi, up, 8, 2, 5 if ct == 1 else 4, 0, 1, False, -1, False)


def tail_pick(form, H, W, mos_py, f16_full, slope, src_lo):
    """launch_conv, conv3x3.hip:932-960.  The refusal at conv3x3.hip:944 read tail_form bit 1, which the engine set exactly for
    CF_HR_SPLIT_NOHI (engine.hip:213): it never fired, and is not restated."""
    full = mos_py == 0 and H % 16 == 0 and W % 32 == 0 and f16_full                                    # :934 (tail_form bit 3 = not f16_full)
    if form == CF_FIRST:
        return _w(2, EPI_FIRST, False)                            # :936
    if form == CF_BODY:
        return _w(2, EPI_BODY, False)                             # :937
    if form == CF_HR:
        return _w(2, EPI_LRELU, False)                            # :938
    if form == CF_LAST:
        return _w(1, EPI_LAST, False)                             # :939
    if form == CF_BODY_SPLIT:                                     # :941
        return (2, EPI_BODY, False, 8, 2, 4, 1, 1, True, -1, full)
    if form == CF_HR_SPLIT:                                       # :942
        return (2, EPI_LRELU, False, 8, 2, 4, 1, 1, True, -1, False)
    if form == CF_HR_SPLIT_NOHI:                                  # :945
        return (2, EPI_LRELU, False, 8, 2, 4, 2, 1, True, -1, full)
    if form == CF_LAST_SPLIT8:                                    # :946
        return (1, EPI_LAST, False, 8, 2, 4, 0, 1, True, -1, False)
    if form == CF_LAST_FOLD:                                      # :948
        return (1, EPI_LAST, False, 8, 2, 4, 3, 1, True, -1, full)
    if form == CF_PRELU:                                          # :950
        return _w(2, EPI_PRELU, False) if slope else INVALID
    if form == CF_CFIRST:                                         # :951
        return _w(2, EPI_CFIRST, False) if slope else INVALID
    if form == CF_CLAST:                                          # :952
        return _w(2, EPI_CLAST, False) if src_lo else INVALID
    if form == CF_DEBUG1:
        return _w(1, EPI_DEBUG, False)                            # :953
    if form == CF_DEBUG1_UP:
        return _w(1, EPI_DEBUG, True)                             # :954
    if form == CF_DEBUG2:
        return _w(2, EPI_DEBUG, False)                            # :955
    if form == CF_DEBUG2_UP:
        return _w(2, EPI_DEBUG, True)                             # :956
    return INVALID                                                # :957-959 (CF_NONE and anything else)


def phase_pick(py, f8_, H, W, mos_py, f16_full):
    """launch_conv_phase, conv3x3.hip:964-977"""
    if py not in (0, 1):
        return INVALID                                            # :976
    if f8_ and mos_py == 0 and H % 8 == 0 and W % 32 == 0 and f16_full:                                 # :965-967
        return (4, EPI_LRELU, False, 8, 1, 4, 1, 1, True, py, True)
    if f8_:
        return (4, EPI_LRELU, False, 8, 1, 4, 1, 1, True, py, False)                                    # :970-971
    return (4, EPI_LRELU, False, 8, 2, 4, 0, 1, False, py, False)                                       # :973-974
