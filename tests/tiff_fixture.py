"""A small TIFF writer for the tests of the reader (s2sr/tiff_lite.py): every layout the reader accepts, written by hand."""
import struct
import zlib

import numpy as np


def write_tiff(path, arr, bo="<", big=False, tile=None, comp=1, pred=1, planar=1, extra=()):
    """arr [H, W, B] (u8/u16/i16/f32).  extra: iterable of (tag, type, values) geo tags."""
    H, W, B = arr.shape
    dt = arr.dtype.newbyteorder(bo)
    fmt = {"u": 1, "i": 2, "f": 3}[arr.dtype.kind]
    cw, ch = (tile, tile) if tile else (W, 16)
    nx, ny = (W + cw - 1) // cw, (H + ch - 1) // ch
    chunks = []
    for pl in range(B if planar == 2 else 1):
        for iy in range(ny):
            for ix in range(nx):
                rows = ch if tile else min(ch, H - iy * ch)
                blk = np.zeros((rows, cw, 1 if planar == 2 else B), arr.dtype)
                src = arr[iy * ch:iy * ch + rows, ix * cw:ix * cw + cw, pl:pl + 1] if planar == 2 else \
                    arr[iy * ch:iy * ch + rows, ix * cw:ix * cw + cw, :]
                blk[:src.shape[0], :src.shape[1]] = src
                if pred == 2:
                    d = blk.copy()
                    d[:, 1:] = blk[:, 1:] - blk[:, :-1]          # wraps modulo the sample width
                    blk = d
                raw = blk.astype(dt).tobytes()
                chunks.append(zlib.compress(raw) if comp == 8 else raw)
    hdr = 16 if big else 8
    offs, pos = [], hdr
    for c in chunks:
        offs.append(pos)
        pos += len(c) + (len(c) & 1)
    ent = [(256, 4, (W,)), (257, 4, (H,)), (258, 3, (arr.dtype.itemsize * 8,) * B), (259, 3, (comp,)),
           (262, 3, (2 if B >= 3 else 1,)), (277, 3, (B,)), (284, 3, (planar,)), (317, 3, (pred,)), (339, 3, (fmt,) * B)]
    o_t, c_t = (324, 325) if tile else (273, 279)
    big_t = 16 if big else 4
    ent += [(o_t, big_t, tuple(offs)), (c_t, big_t, tuple(len(c) for c in chunks))]
    ent += [(322, 3, (cw,)), (323, 3, (ch,))] if tile else [(278, 3, (ch,))]
    ent += list(extra)
    ent.sort()
    tsz = {3: ("H", 2), 4: ("I", 4), 12: ("d", 8), 16: ("Q", 8), 2: ("s", 1)}
    esz, inl = (20, 8) if big else (12, 4)
    ifd_off = pos
    val_pos = ifd_off + (8 if big else 2) + esz * len(ent) + (8 if big else 4)
    ifd, tail = b"", b""
    for tag, typ, vals in ent:
        if typ == 2:
            data = vals.encode() + b"\0"
            cnt = len(data)
        else:
            f, _ = tsz[typ]
            data = struct.pack(bo + f * len(vals), *vals)
            cnt = len(vals)
        e = struct.pack(bo + "HH", tag, typ) + struct.pack(bo + ("Q" if big else "I"), cnt)
        if len(data) <= inl:
            e += data.ljust(inl, b"\0")
        else:
            e += struct.pack(bo + ("Q" if big else "I"), val_pos + len(tail))
            tail += data + (b"\0" if len(data) & 1 else b"")
        ifd += e
    with open(path, "wb") as f:
        f.write(b"II" if bo == "<" else b"MM")
        if big:
            f.write(struct.pack(bo + "HHHQ", 43, 8, 0, ifd_off))
        else:
            f.write(struct.pack(bo + "HI", 42, ifd_off))
        for c in chunks:
            f.write(c + (b"\0" if len(c) & 1 else b""))
        f.write(struct.pack(bo + ("Q" if big else "H"), len(ent)) + ifd + struct.pack(bo + ("Q" if big else "I"), 0) + tail)
