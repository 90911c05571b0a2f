"""The whole-image door and its forms (include/s2sr.h: s2sr_enhance_args, s2sr_enhance, the table of forms under it).

Every other GPU test reaches s2sr_enhance through the forms of native.Engine, which are spellings of Engine.enhance.  Here the
eleven exported C forms are called directly, with raw ctypes arguments, and held byte for byte to Engine.enhance given the fields
the header's table states for them; every refusal, a form's own or the record's (engine_aoi.hip check_call), is held to its code
and its text, and to leaving the handle as it was; and one record that no form spells is held to its definition.
1-block nets and the images of tests/doors.py."""
import ctypes as C

import numpy as np
import pytest

import doors
import gpu_engines
from diag import keep, same
from s2sr import native

pytestmark = pytest.mark.gpu

INVALID = -1                     # S2SR_E_INVALID
LO, HI = doors.SUB
X = doors.Inputs()
CASES = [("x4_hp", "chunked", doors.IMAGES["chunked"]), ("x4_hp", "untiled", doors.IMAGES["untiled"]), ("x2plus", "odd39_tiled", (39, 39, 16, 3))]


def engine(name):
    return gpu_engines.default(*doors.CONFIGS[name])


def ptr(a):
    return None if a is None else a.ctypes.data


def images(H, W):
    """the 8-bit and the 16-bit image and the mask doors.py gives a case of this size"""
    seed = 7 + 1000 * H + W
    return X.u8((H, W, 3), seed), X.u16((H, W, 3), H), doors._valid(H, W, seed)


def buffers(S, H, W, dtype):
    """caller-owned outputs (q, f32, inexact), filled as doors.py fills them"""
    return (np.full((S * H, S * W, 3), doors.FILL, dtype), np.full((S * H, S * W, 3), doors.FILL, np.float32), np.full(3, doors.FILL, np.uint64))


def mask(valid, radius=5, out_nodata=3):
    return native.Mask(valid.ctypes.data, radius, out_nodata)


# form -> (bits, the raw call: fn(lib, h, img, g = (H, W, tile, pad), m, prm, q, f, bad) -> rc, the outputs it fills, the fields of the
# header's table for Engine.enhance).  The options are given the values that make each form do the most: a post-process with the
# exchange, the blend, a mask, mode 2 for 8 bits and mode 1 for 16.
FORMS = {
    "s2sr_enhance_u8": (8, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_u8(h, ptr(i), *g, ptr(q)), "q", {}),
    "s2sr_enhance_job_u8": (8, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_job_u8(h, ptr(i), *g, C.byref(p), ptr(q)), "q",
                            dict(swap_rb=True, prm=True)),
    "s2sr_enhance_f32": (8, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_f32(h, ptr(i), *g, ptr(f)), "f", dict(quantised=False, want_f32=True)),
    "s2sr_tile_process_f32": (8, lambda L, h, i, g, m, p, q, f, b: L.s2sr_tile_process_f32(h, ptr(i), *g, ptr(f)), "f",
                              dict(force_tiled=True, quantised=False, want_f32=True)),
    "s2sr_enhance_u16": (16, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_u16(h, ptr(i), *g, LO, HI, ptr(q), ptr(f)), "qf",
                         dict(lo=LO, hi=HI, want_f32=True)),
    "s2sr_enhance_blend_u8": (8, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_blend_u8(h, ptr(i), *g, None, 0, ptr(q), ptr(f)), "qf",
                              dict(blend=True, want_f32=True)),
    "s2sr_enhance_blend_u8-job": (8, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_blend_u8(h, ptr(i), *g, C.byref(p), 1, ptr(q), None), "q",
                                  dict(blend=True, prm=True, swap_rb=True)),
    "s2sr_enhance_blend_u16": (16, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_blend_u16(h, ptr(i), *g, LO, HI, ptr(q), ptr(f)), "qf",
                               dict(lo=LO, hi=HI, blend=True, want_f32=True)),
    "s2sr_enhance_masked_u8": (8, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_masked_u8(h, ptr(i), *g, C.byref(p), 1, 1, C.byref(m), ptr(q)), "q",
                               dict(prm=True, swap_rb=True, blend=True, valid=True)),
    "s2sr_enhance_masked_u16": (16, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_masked_u16(h, ptr(i), *g, LO, HI, 1, C.byref(m), ptr(q)), "q",
                                dict(lo=LO, hi=HI, blend=True, valid=True)),
    "s2sr_enhance_consistent_u8": (8, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_consistent_u8(h, ptr(i), *g, C.byref(p), 1, 1, C.byref(m), 2,
                                                                                                     ptr(q), ptr(b)), "qb",
                                   dict(prm=True, swap_rb=True, blend=True, valid=True, consistency=2)),
    "s2sr_enhance_consistent_u16": (16, lambda L, h, i, g, m, p, q, f, b: L.s2sr_enhance_consistent_u16(h, ptr(i), *g, LO, HI, 1, C.byref(m), 1,
                                                                                                        ptr(q), ptr(b)), "qb",
                                    dict(lo=LO, hi=HI, blend=True, valid=True, consistency=1)),
}
assert {n.split("-")[0] for n in FORMS} == {n for n in native.EXPORTED_SYMBOLS if n.startswith("s2sr_enhance_") or n == "s2sr_tile_process_f32"}


# every form on the x4 net; the 8-bit forms on x2plus (the 16-bit ones exist on the x4 RRDB nets only: their refusal is held below)
FORM_CASES = [(n, c, s, form) for n, c, s in CASES for form in FORMS if n == "x4_hp" or FORMS[form][0] == 8]


@pytest.mark.parametrize("name,case,shape,form", FORM_CASES, ids=[f"{c[0]}-{c[1]}-{c[3]}" for c in FORM_CASES])
def test_each_c_form_is_the_record_the_header_states(name, case, shape, form):
    bits, call, outs, fields = FORMS[form]
    e, (H, W, tile, pad) = engine(name), shape
    img8, img16, valid = images(H, W)
    img = img16 if bits == 16 else img8
    q, f, bad = buffers(e.scale, H, W, img.dtype)
    m, prm = mask(valid), native.pp_wow()
    rc = call(native.load_library(), e._h, img, (H, W, tile, pad), m, prm, q, f, bad)
    assert rc == 0, native.load_library().s2sr_last_error(e._h)
    fields = dict(fields)
    if fields.pop("valid", False):
        fields.update(valid=valid, radius=5, out_nodata=3)
    if fields.pop("prm", False):
        fields.update(prm=native.pp_wow())
    r = e.enhance(img, tile=tile, pad=pad, **fields)
    got = tuple({"q": q, "f": f, "b": bad}[k] for k in outs)
    want = tuple({"q": r.q, "f": r.f32, "b": r.inexact}[k] for k in outs)
    assert all(w is not None for w in want) and sum(w is not None for w in r) == len(outs)      # the record gave what the form gives
    same(got, keep(want), f"{form} on {name}-{case}")


def record(e, img, q=True, f32=False, inexact=False, size=None, bits=None, tile=256, pad=10, lo=0, hi=65535, prm=None, swap_rb=0, blend=0,
           force_tiled=0, m=None, consistency=0):
    """s2sr_enhance on a record given field by field, nothing checked on this side -> (rc, the handle's last error)."""
    H, W, _ = img.shape
    Q, F, bad = buffers(e.scale, H, W, img.dtype)
    a = native.EnhanceArgs(C.sizeof(native.EnhanceArgs) if size is None else size, 8 * img.itemsize if bits is None else bits, ptr(img), H, W, tile,
                           pad, lo, hi, None if prm is None else C.pointer(prm), swap_rb, blend, force_tiled, None if m is None else C.pointer(m),
                           consistency, ptr(Q) if q else None, ptr(F) if f32 else None, ptr(bad) if inexact else None)
    rc = e._lib.s2sr_enhance(e._h, C.byref(a))
    return rc, e._lib.s2sr_last_error(e._h).decode()


def refusals(e, img8, img16, valid):
    """(what, fn() -> (rc, text), a substring of the refusal's text as the library's source has it)"""
    H, W, _ = img8.shape
    g, L, h = (H, W, 256, 10), e._lib, e._h
    q8, f, bad = buffers(e.scale, H, W, np.uint8)
    q16 = buffers(e.scale, H, W, np.uint16)[0]
    wow, ok = native.pp_wow(), mask(valid)
    raw = lambda rc: (rc, L.s2sr_last_error(h).decode())
    rec = lambda img=img8, **kw: record(e, img, **kw)
    yield "size - 4", lambda: rec(size=C.sizeof(native.EnhanceArgs) - 4), "size must be sizeof(s2sr_enhance_args)"
    yield "size + 8", lambda: rec(size=C.sizeof(native.EnhanceArgs) + 8), "size must be sizeof(s2sr_enhance_args)"
    yield "bits 12", lambda: rec(bits=12), "bits must be 8 or 16"
    yield "no output", lambda: rec(q=False), "s2sr_enhance: an image, positive sizes and at least one output are required"
    yield "a job without out", lambda: rec(q=False, prm=wow, swap_rb=1), "s2sr_enhance: an image, positive sizes and at least one output are required"
    yield "a job without out, blend form", lambda: raw(L.s2sr_enhance_blend_u8(h, ptr(img8), *g, C.byref(wow), 1, None, None)), \
        "s2sr_enhance_blend: an image, positive sizes and at least one output are required"
    yield "a job without out, masked form", lambda: raw(L.s2sr_enhance_masked_u8(h, ptr(img8), *g, C.byref(wow), 1, 0, C.byref(ok), None)), \
        "s2sr_enhance_masked_u8: an image, positive sizes and out_u8 are required"
    yield "tile 0", lambda: rec(tile=0), "s2sr_enhance: an image, positive sizes"
    yield "16 bits with prm", lambda: rec(img16, prm=wow), "prm and swap_rb belong to 8-bit images"
    yield "16 bits with swap_rb", lambda: rec(img16, swap_rb=1), "prm and swap_rb belong to 8-bit images"
    for what, kw in (("a 16-bit image", dict(img=img16)), ("out", dict(q=True)), ("prm", dict(prm=wow)), ("swap_rb", dict(swap_rb=1)),
                     ("blend", dict(blend=1)), ("a mask", dict(m=ok)), ("a mode", dict(consistency=1))):
        yield f"force_tiled with {what}", lambda kw=kw: rec(**{**dict(q=False, f32=True, force_tiled=1), **kw}), "force_tiled is s2sr_tile_process_f32"
    yield "8 bits, both outputs, no blend", lambda: rec(f32=True), "out and out_f32 together needs blend"
    # the forms' own
    yield "blend_u8 without image", lambda: raw(L.s2sr_enhance_blend_u8(h, None, *g, None, 0, ptr(q8), None)), "s2sr_enhance_blend_u8: an image is required"
    yield "blend_u16 without image", lambda: raw(L.s2sr_enhance_blend_u16(h, None, *g, LO, HI, ptr(q16), None)), "s2sr_enhance_blend_u16: an image is required"
    yield "masked_u8 without m", lambda: raw(L.s2sr_enhance_masked_u8(h, ptr(img8), *g, None, 0, 0, None, ptr(q8))), \
        "s2sr_enhance_masked_u8: a mask is required (m == NULL)"
    yield "masked_u16 without m", lambda: raw(L.s2sr_enhance_masked_u16(h, ptr(img16), *g, LO, HI, 0, None, ptr(q16))), \
        "s2sr_enhance_masked_u16: a mask is required (m == NULL)"
    for mode in (0, 3):
        yield f"consistent_u8 mode {mode}", lambda mode=mode: raw(L.s2sr_enhance_consistent_u8(h, ptr(img8), *g, None, 0, 0, None, mode, ptr(q8), ptr(bad))), \
            "consistency: mode must be 1 (S2SR_CONSISTENCY_EXACT) or 2 (S2SR_CONSISTENCY_SMOOTH)"
        yield f"consistent_u16 mode {mode}", lambda mode=mode: raw(L.s2sr_enhance_consistent_u16(h, ptr(img16), *g, LO, HI, 0, None, mode, ptr(q16), ptr(bad))), \
            "consistency: mode must be 1 (S2SR_CONSISTENCY_EXACT) or 2 (S2SR_CONSISTENCY_SMOOTH)"
    yield "u16 form without output", lambda: raw(L.s2sr_enhance_u16(h, ptr(img16), *g, LO, HI, None, None)), \
        "s2sr_enhance_u16: an image, positive sizes and at least one output are required"
    # the record's, as they stood before the record was public
    flt = "the float image is the net's own output: not with a post-process or swap_rb"
    yield "fp32 with prm", lambda: rec(q=False, f32=True, prm=wow), flt
    yield "fp32 with swap_rb", lambda: rec(q=False, f32=True, swap_rb=1), flt
    yield "fp32 with prm, blend form", lambda: raw(L.s2sr_enhance_blend_u8(h, ptr(img8), *g, C.byref(wow), 0, ptr(q8), ptr(f))), flt
    yield "fp32 with a mask", lambda: rec(q=False, f32=True, m=ok), "nodata: the float image is the net's own output and is never masked"
    yield "fp32 with a mode", lambda: rec(q=False, f32=True, consistency=1), "consistency: the float image is the net's own output and is never corrected"
    yield "radius 0", lambda: rec(m=mask(valid, radius=0)), "nodata: the fill radius must be 1..64"
    yield "radius 65", lambda: rec(m=mask(valid, radius=65)), "nodata: the fill radius must be 1..64"
    yield "out_nodata 256", lambda: rec(m=mask(valid, out_nodata=256)), "nodata: out_nodata must be 0..255"
    yield "out_nodata 65536", lambda: rec(img16, m=mask(valid, out_nodata=65536)), "nodata: out_nodata must be 0..65535"
    yield "a mask without valid", lambda: rec(m=native.Mask(None, 5, 0)), "nodata: a mask (valid, uint8 [H, W]) is required"
    yield "mode 3", lambda: rec(consistency=3, inexact=True), "consistency: mode must be 1 (S2SR_CONSISTENCY_EXACT) or 2 (S2SR_CONSISTENCY_SMOOTH)"
    yield "lo == hi", lambda: rec(img16, lo=500, hi=500), "need 0 <= lo < hi <= 65535"
    yield "lo > hi", lambda: rec(img16, lo=HI, hi=LO), "need 0 <= lo < hi <= 65535"


def test_refusals_by_form_and_by_record_leave_the_handle_working():
    e = engine("x4_hp")
    H, W, tile, pad = doors.IMAGES["untiled"]
    img8, img16, valid = images(H, W)
    base = keep(e.enhance_u8(img8, tile=tile, pad=pad))
    n = 0
    for what, call, text in refusals(e, img8, img16, valid):
        rc, err = call()
        assert rc == INVALID and text in err, (what, rc, err)
        same(keep(e.enhance_u8(img8, tile=tile, pad=pad)), base, f"enhance_u8 after the refusal of: {what}")
        n += 1
    assert n == 40                                           # (the generator is not silently empty or cut short)
    lib = e._lib
    assert lib.s2sr_enhance(e._h, None) == INVALID and lib.s2sr_enhance_job_u8(e._h, ptr(img8), H, W, tile, pad, None, None) == INVALID
    same(keep(e.enhance_u8(img8, tile=tile, pad=pad)), base, "enhance_u8 after a NULL record and a job without out")


@pytest.mark.parametrize("name,text", [("x2plus", "16-bit input is not available on a scale-2 handle"),
                                       ("compact", "16-bit input is not available on an S2SR_ARCH_COMPACT handle")], ids=["x2plus", "compact"])
def test_a_16_bit_image_is_refused_where_the_net_has_no_16_bit_input(name, text):
    e = engine(name)
    H, W, tile, pad = doors.IMAGES["untiled"]
    img8, img16, _ = images(H, W)
    base = keep(e.enhance_u8(img8, tile=tile, pad=pad))
    q16 = buffers(e.scale, H, W, np.uint16)[0]
    for rc, err in (record(e, img16, lo=LO, hi=HI),
                    (e._lib.s2sr_enhance_u16(e._h, ptr(img16), H, W, tile, pad, LO, HI, ptr(q16), None), e._lib.s2sr_last_error(e._h).decode())):
        assert rc == INVALID and text in err, (rc, err)
        same(keep(e.enhance_u8(img8, tile=tile, pad=pad)), base, f"enhance_u8 on {name} after the refusal")


@pytest.mark.parametrize("case", ["chunked", "untiled"])
def test_a_post_process_alone_is_the_post_process_on_the_plain_image(case):
    """A record no form spells: prm without swap_rb, blend, mask or mode.  The header defines it: the post-process on the plain door's
    image in the order given.  (chunked: three chunks, so the post-process runs in bands behind the paste; untiled: on the whole image.)"""
    e = engine("x4_hp")
    H, W, tile, pad = doors.IMAGES[case]
    img = images(H, W)[0]
    want = keep(e.postprocess_u8(keep(e.enhance_u8(img, tile=tile, pad=pad)), native.pp_wow()))
    r = e.enhance(img, tile=tile, pad=pad, prm=native.pp_wow())
    assert r.f32 is None and r.inexact is None
    same(keep(r.q), want, f"enhance(prm) on {case}")
