"""The record of a whole-image call on both sides of the boundary: native.EnhanceArgs is field for field the s2sr_enhance_args of
include/s2sr.h, and s2sr_enhance refuses a call without handle or record."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from s2sr import native

REPO = Path(__file__).resolve().parent.parent
C_TYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32}


def header_fields():
    """[(name, ctypes type)] of s2sr_enhance_args as the header declares it: comments stripped, one declaration per ';', several
    names per declaration."""
    header = (REPO / "include" / "s2sr.h").read_text()
    body = re.search(r"typedef struct s2sr_enhance_args \{(.*?)\} s2sr_enhance_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = re.fullmatch(r"(.*?[\s*])([A-Za-z_0-9]+(?:\s*,\s*[A-Za-z_0-9]+)*)", decl, re.S).groups()
        ctype = " ".join(ctype.split())
        for n in re.split(r"\s*,\s*", names):
            out.append((n, ctype))
    return out


def test_enhance_args_is_the_headers_struct():
    declared = header_fields()
    assert [n for n, _ in declared] == [n for n, _ in native.EnhanceArgs._fields_]
    for (name, ctype), (_, py) in zip(declared, native.EnhanceArgs._fields_):
        if ctype.endswith("*"):
            assert C.sizeof(py) == C.sizeof(C.c_void_p), name
            want = {"const s2sr_pp_params*": C.POINTER(native.PPParams), "const s2sr_mask*": C.POINTER(native.Mask)}.get(ctype, C.c_void_p)
            assert py is want, (name, ctype, py)
        else:
            assert py is C_TYPES[ctype], (name, ctype, py)
    assert native._PROTOS["s2sr_enhance"] == (C.c_int, [C.c_void_p, C.POINTER(native.EnhanceArgs)])


def test_enhance_without_a_handle_is_refused():
    a = native.EnhanceArgs(size=C.sizeof(native.EnhanceArgs), bits=8)
    lib = native.load_library()
    assert lib.s2sr_enhance(None, C.byref(a)) == -1
    assert lib.s2sr_enhance(None, None) == -1


@pytest.mark.gpu
def test_enhance_without_a_record_is_refused():
    import doors
    import gpu_engines
    e = gpu_engines.default(*doors.CONFIGS["x4_hp"])
    img = np.zeros((8, 8, 3), np.uint8)
    want = np.array(e.enhance_u8(img))
    assert e._lib.s2sr_enhance(e._h, None) == -1
    assert np.array_equal(e.enhance_u8(img), want)
