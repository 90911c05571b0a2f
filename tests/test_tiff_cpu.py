"""CPU tests of the raster input glue: the TIFF reader that takes over where PIL stops (multi-band
16-bit GeoTIFFs, the reference reads them with rasterio, server/app/wow_sr.py:59-79) and the
native TIFF-LZW decoder.  Files are produced by PIL where PIL can write them and by a small
writer below (strips / tiles, chunky / planar, Deflate + predictor, big endian, BigTIFF)."""
import struct
import zlib

import os
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

from s2sr import rasterio_lite as rio
from s2sr import tiff_lite
from tiff_fixture import write_tiff


def _scene(H, W, B, dtype, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (np.sin(xx / 9.0) + np.cos(yy / 7.0) + 2.2) * (900 if np.dtype(dtype).itemsize > 1 else 50)
    a = np.stack([base * (1 + 0.1 * b) + rng.integers(0, 40, (H, W)) for b in range(B)], -1)
    return a.astype(dtype)


@pytest.mark.parametrize("mode", ["rgb8", "i16", "rgb8_noise"])
def test_lzw_against_pil(tmp_path, mode):
    """PIL writes the LZW file, the native decoder (through tiff_lite) must return PIL's own pixels.
    The noise image forces the code table through every width and several ClearCodes."""
    if mode == "rgb8":
        arr = _scene(150, 211, 3, np.uint8)
        im = Image.fromarray(arr, "RGB")
    elif mode == "rgb8_noise":
        arr = np.random.default_rng(5).integers(0, 256, (120, 333, 3), dtype=np.uint8)
        im = Image.fromarray(arr, "RGB")
    else:
        arr = _scene(97, 130, 1, np.uint16)[..., 0]
        im = Image.fromarray(arr)
    p = tmp_path / f"{mode}.tif"
    im.save(p, format="TIFF", compression="tiff_lzw")
    got, tags = tiff_lite.read_tiff(p)
    assert tags[tiff_lite.COMPRESSION][0] == 5
    want = np.asarray(Image.open(p))
    assert np.array_equal(got if got.shape[2] > 1 else got[..., 0], want)


@pytest.mark.parametrize("kw", [
    dict(),                                             # chunky strips, uncompressed, little endian
    dict(comp=8, pred=2),                               # Deflate + horizontal differencing
    dict(tile=64, comp=8, pred=2),                      # tiled (edge tiles padded)
    dict(planar=2, comp=8),                             # separate planes
    dict(bo=">", tile=32),                              # big endian, tiled
    dict(big=True, comp=8, pred=2, tile=128),           # BigTIFF
])
def test_multiband_uint16_roundtrip(tmp_path, kw):
    arr = _scene(143, 201, 4, np.uint16, seed=3)        # 4 bands like a B02/B03/B04/B08 delivery
    p = tmp_path / "s2.tif"
    write_tiff(p, arr, **kw)
    got, _ = tiff_lite.read_tiff(p)
    assert got.dtype == np.uint16 and np.array_equal(got, arr)


def test_other_sample_types_and_errors(tmp_path):
    for dt in (np.uint8, np.int16, np.float32):
        arr = _scene(40, 50, 3, dt, seed=1)
        write_tiff(tmp_path / "t.tif", arr, comp=8, pred=(1 if np.dtype(dt).kind == "f" else 2))
        got, _ = tiff_lite.read_tiff(tmp_path / "t.tif")
        assert got.dtype == np.dtype(dt) and np.array_equal(got, arr)
    (tmp_path / "bad.tif").write_bytes(b"not a tiff at all")
    with pytest.raises(tiff_lite.TiffError):
        tiff_lite.read_tiff(tmp_path / "bad.tif")
    write_tiff(tmp_path / "jpeg.tif", _scene(16, 16, 3, np.uint8), comp=1)
    raw = bytearray((tmp_path / "jpeg.tif").read_bytes())
    raw = raw.replace(struct.pack("<HHI", 259, 3, 1) + struct.pack("<H", 1), struct.pack("<HHI", 259, 3, 1) + struct.pack("<H", 7))
    (tmp_path / "jpeg.tif").write_bytes(bytes(raw))
    with pytest.raises(tiff_lite.TiffError, match="compression 7"):
        tiff_lite.read_tiff(tmp_path / "jpeg.tif")


def test_read_rgb_u8_on_sentinel_like_geotiff(tmp_path):
    """What apply_wow_sr does with a 4-band uint16 GeoTIFF (wow_sr.py:59-79): bands 1-3, one min-max
    over the 3-band stack to 0..255 (truncating), geo tags carried to the x4 output."""
    arr = _scene(90, 120, 4, np.uint16, seed=7)
    arr[..., 3] += 20000                                   # band 4 (NIR) must not influence the stretch
    geo = [(33550, 12, (10.0, 10.0, 0.0)), (33922, 12, (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0)),
           (34735, 3, (1, 1, 0, 1, 3072, 0, 1, 32633)), (34737, 2, "WGS 84 / UTM zone 33N|")]
    p = tmp_path / "aoi.tif"
    write_tiff(p, arr, tile=64, comp=8, pred=2, extra=geo)
    # the reason tiff_lite goes first: PIL squeezes this file to 8-bit RGBA without a word
    assert np.asarray(Image.open(p)).dtype == np.uint8
    rgb, georef = rio.read_rgb_u8(p)
    img = arr[..., :3]
    want = ((img - img.min()) / (img.max() - img.min()) * 255).astype(np.uint8)   # the reference's expression
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, want)
    assert georef.pixel_size == (10.0, 10.0)
    assert georef.scaled(4).pixel_size == (2.5, 2.5)
    out = tmp_path / "out.tif"
    rio.write_geotiff_rgb(out, np.repeat(np.repeat(rgb, 4, 0), 4, 1), georef.scaled(4))
    back, g2 = rio.read_rgb_u8(out)
    assert back.shape == (360, 480, 3) and g2.pixel_size == (2.5, 2.5)
    assert tuple(g2.tags[33922]) == (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0)


def test_lzw_encoder_roundtrip_and_libtiff_reads_it(tmp_path):
    """Native LZW encoder: decodes back through the native decoder, and libtiff (via PIL) reads the
    GeoTIFFs written with it -- pixels and geo tags -- for sizes around the strip height."""
    from s2sr import native
    rng = np.random.default_rng(2)
    for data in (b"", b"a", b"ab" * 5000, bytes(range(256)) * 64, rng.integers(0, 256, 300000, dtype=np.uint8).tobytes(),
                 rng.integers(0, 3, 200000, dtype=np.uint8).tobytes()):
        enc = native.tiff_lzw_encode(data)
        assert native.tiff_lzw_decode(enc, len(data)) == data
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (2.5, 2.5, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0),
                      rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633),
                      rio.TAG_GEOASCII: "WGS 84 / UTM zone 33N|"})
    for shape in ((1, 1, 3), (63, 5, 3), (64, 64, 3), (65, 7, 3), (300, 411, 3)):
        a = _scene(shape[0], shape[1], 3, np.uint8, seed=shape[0])
        p = tmp_path / "o.tif"
        rio.write_geotiff_rgb(p, a, geo)
        im = Image.open(p)
        assert np.array_equal(np.asarray(im), a), shape
        tv = im.tag_v2
        assert tv[259] == 5 and tuple(tv[33550]) == (2.5, 2.5, 0.0) and tuple(tv[34735])[-1] == 32633
        assert tv[34737].startswith("WGS 84 / UTM zone 33N")
        back, g2 = rio.read_rgb_u8(p)
        assert np.array_equal(back, a) and g2.pixel_size == (2.5, 2.5)
    # strips the dictionary coder would EXPAND (8-bit texture: most lookups miss, every miss is a 9..12-bit code for one byte) go
    # out in the literal form -- every byte a 9-bit code, a ClearCode every 250: a valid LZW stream of 1.13x the input for any
    # decoder, here libtiff's and the native one -- while compressible strips keep the dictionary form
    noise = rng.integers(0, 256, 786432, dtype=np.uint8)
    enc = native.tiff_lzw_encode(noise)
    assert 1.12 < len(enc) / noise.size < 1.135 and native.tiff_lzw_decode(enc, noise.size) == noise.tobytes()
    ramp = (np.arange(786432) // 300 % 256).astype(np.uint8)
    assert len(native.tiff_lzw_encode(ramp)) < 0.2 * ramp.size
    a = rng.integers(0, 256, (200, 500, 3), dtype=np.uint8)          # 96-KB strips of noise: literal form
    a[130:] = 77                                                      # ... and the last strip a constant: dictionary form
    p = tmp_path / "lit.tif"
    rio.write_geotiff_rgb(p, a, geo)
    assert p.stat().st_size < 1.14 * 130 * 1500 + 20000
    assert np.array_equal(np.asarray(Image.open(p)), a)
    assert np.array_equal(rio.read_rgb_u8(p)[0], a)
    # an RGBA raster (the tiler's warp result next to its <stem>_3857.tif): alpha dropped strip by strip, the same file as from the RGB copy
    rgba = np.dstack([a, rng.integers(0, 256, a.shape[:2], dtype=np.uint8)])
    rio.write_geotiff_rgb(tmp_path / "from_rgba.tif", rgba, geo)
    assert (tmp_path / "from_rgba.tif").read_bytes() == p.read_bytes()
    with pytest.raises(ValueError):
        rio.write_geotiff_rgb(tmp_path / "bad.tif", rgba[..., :2], geo)
    with pytest.raises(ValueError):
        rio.write_geotiff_rgb(tmp_path / "bad.tif", rgba, geo, remember=True)
    assert not (tmp_path / "bad.tif").exists()


def test_large_files_are_read_in_slices(tmp_path):
    """Files of 8 MB and more are read in 2-MB slices from the host pool (tiff_lite._read_file), their LZW strips decoded straight
    into the rows of the result: a 1536 x 2048 RGB raster (literal-form and dictionary-form strips mixed) comes back exactly, with its
    geo tags, and the reader still refuses a file that is cut short."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (1536, 2048, 3), dtype=np.uint8)
    a[700:900] = (np.arange(2048) // 9 % 256).astype(np.uint8)[None, :, None]           # compressible strips in between
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (2.5, 2.5, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0)})
    p = tmp_path / "big.tif"
    rio.write_geotiff_rgb(p, a, geo)
    assert p.stat().st_size > (8 << 20)
    back, tags = tiff_lite.read_tiff(p)
    assert np.array_equal(back, a) and tuple(tags[rio.TAG_PIXEL_SCALE]) == (2.5, 2.5, 0.0)
    assert np.array_equal(np.asarray(Image.open(p)), a)
    cut = tmp_path / "cut.tif"
    cut.write_bytes(p.read_bytes()[:9 << 20])
    with pytest.raises(tiff_lite.TiffError):
        tiff_lite.read_tiff(cut)


def test_png_encoder_bands_form_one_stream():
    """Parallel PNG encoder: bands deflated independently and stitched with sync flushes + a combined
    Adler-32 must decode (PIL / zlib) to the input, for RGB and RGBA, with and without threads."""
    import io
    import zlib
    rng = np.random.default_rng(3)
    data = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1, 70000, 5, 300001)]
    ad = 1
    for d in data:
        ad = rio._adler32_combine(ad, zlib.adler32(d), len(d))
    assert ad == zlib.adler32(b"".join(data))
    for shape in ((1, 1, 3), (5, 7, 4), (129, 64, 3), (300, 401, 3), (513, 100, 4)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        for workers in (1, 4):
            im = Image.open(io.BytesIO(rio.encode_png(a, band_rows=128, workers=workers)))
            assert im.mode == ("RGB" if shape[2] == 3 else "RGBA") and np.array_equal(np.asarray(im), a), (shape, workers)
    with pytest.raises(ValueError):
        rio.encode_png(np.zeros((4, 4, 2), np.uint8))


def test_malformed_tiffs_are_tiff_errors_and_stay_bounded(tmp_path, monkeypatch):
    """Uploaded files reach read_tiff (sr_routes /api/enhance): whatever a damaged file breaks, the outcome is an array or a
    TiffError (read_rgb_u8 then falls back to PIL), never another exception, and never an allocation beyond the configured cap."""
    monkeypatch.setenv("S2SR_TIFF_MAX_BYTES", str(1 << 24))
    rng = np.random.default_rng(11)
    arr = _scene(61, 83, 3, np.uint16, seed=2)
    seeds = []
    for i, kw in enumerate([dict(), dict(comp=8, pred=2), dict(tile=32, comp=8), dict(planar=2), dict(big=True, comp=8, tile=64), dict(bo=">")]):
        write_tiff(tmp_path / f"s{i}.tif", arr, **kw)
        seeds.append((tmp_path / f"s{i}.tif").read_bytes())
    Image.fromarray(_scene(64, 90, 3, np.uint8)).save(tmp_path / "lzw.tif", format="TIFF", compression="tiff_lzw")
    Image.fromarray(_scene(64, 90, 3, np.uint8)).save(tmp_path / "pb.tif", format="TIFF", compression="packbits")
    seeds += [(tmp_path / "lzw.tif").read_bytes(), (tmp_path / "pb.tif").read_bytes()]
    outcomes = {"array": 0, "error": 0}
    p = tmp_path / "m.tif"
    for it in range(600):
        raw = bytearray(seeds[it % len(seeds)])
        kind = it % 4
        if kind == 0:                                   # a few random bytes anywhere
            for _ in range(1 + it % 5):
                raw[rng.integers(len(raw))] = rng.integers(256)
        elif kind == 1:                                 # damage inside the header / first IFD entries, where the geometry lives
            bo = "<" if raw[:2] == b"II" else ">"
            big = struct.unpack_from(bo + "H", raw, 2)[0] == 43
            off = struct.unpack_from(bo + ("Q" if big else "I"), raw, 8 if big else 4)[0]
            for _ in range(3):
                raw[min(len(raw) - 1, off + int(rng.integers(0, 260)))] = rng.integers(256)
        elif kind == 2:                                 # truncation
            raw = raw[:int(rng.integers(0, len(raw)))]
        else:                                           # a 4-byte field set to an extreme value
            pos = int(rng.integers(0, max(1, len(raw) - 4)))
            raw[pos:pos + 4] = [b"\xff\xff\xff\xff", b"\0\0\0\0", b"\xff\xff\xff\x7f", b"\0\0\0\x80"][it // 4 % 4]
        p.write_bytes(bytes(raw))
        try:
            got, _ = tiff_lite.read_tiff(p)
        except tiff_lite.TiffError:
            outcomes["error"] += 1
        else:
            assert got.nbytes <= (1 << 24)
            outcomes["array"] += 1
    assert outcomes["array"] > 20 and outcomes["error"] > 100, outcomes      # both sides of the line were exercised
    # a Deflate chunk that inflates far beyond its geometry is cut at the geometry (decompression bomb)
    bomb = tmp_path / "bomb.tif"
    write_tiff(bomb, _scene(16, 16, 3, np.uint8), comp=8)
    good = zlib.compress(_scene(16, 16, 3, np.uint8).tobytes())
    evil = zlib.compress(_scene(16, 16, 3, np.uint8).tobytes() + bytes(1 << 26))
    raw = (bomb).read_bytes()
    assert good in raw and len(evil) < 200000
    if True:        # append the evil stream and point the single strip at it
        at = len(raw)
        raw2 = bytearray(raw + evil)
        raw2 = raw2.replace(struct.pack("<HHII", 279, 4, 1, len(good)), struct.pack("<HHII", 279, 4, 1, len(evil)))
        raw2 = raw2.replace(struct.pack("<HHII", 273, 4, 1, raw.index(good)), struct.pack("<HHII", 273, 4, 1, at))
        bomb.write_bytes(bytes(raw2))
        import tracemalloc
        tracemalloc.start()
        got, _ = tiff_lite.read_tiff(bomb)
        peak = tracemalloc.get_traced_memory()[1]
        tracemalloc.stop()
        assert np.array_equal(got, _scene(16, 16, 3, np.uint8)) and peak < (1 << 22), peak
    # dimensions above the cap are refused before any allocation
    write_tiff(tmp_path / "big.tif", _scene(8, 8, 3, np.uint8))
    raw = bytearray((tmp_path / "big.tif").read_bytes())
    for tag in (256, 257):
        assert struct.pack("<HHII", tag, 4, 1, 8) in raw
        raw = raw.replace(struct.pack("<HHII", tag, 4, 1, 8), struct.pack("<HHII", tag, 4, 1, 60000))
    (tmp_path / "big.tif").write_bytes(bytes(raw))
    with pytest.raises(tiff_lite.TiffError, match="S2SR_TIFF_MAX_BYTES"):
        tiff_lite.read_tiff(tmp_path / "big.tif")


def test_native_png_encoder_decodes_to_the_input():
    """csrc/pngenc.hip through the C ABI (s2sr_png_encode / s2sr_png_idat_band): PIL must read back the input pixels for noise
    (stored blocks), constants (one run), upsampled and mixed content, strided views, and a Fibonacci histogram whose Huffman
    tree is deeper than the 15 bits deflate allows (the length-limiting repair)."""
    import io
    import zlib
    from s2sr import native
    rng = np.random.default_rng(9)

    def roundtrip(img, tag):
        b = native.png_encode(img)
        Image.open(io.BytesIO(b)).verify()                                  # chunk CRCs
        got = np.asarray(Image.open(io.BytesIO(b)))
        assert got.shape == img.shape and np.array_equal(got, img), tag
        return b

    for shape in ((1, 1, 3), (1, 1, 4), (2, 3, 3), (5, 7, 4), (256, 256, 4), (300, 257, 3), (257, 2, 3), (3, 5000, 4)):
        roundtrip(rng.integers(0, 256, shape, dtype=np.uint8), ("noise", shape))
        roundtrip(np.zeros(shape, np.uint8), ("zeros", shape))
        up = np.repeat(np.repeat(rng.integers(0, 256, (shape[0] // 6 + 1, shape[1] // 6 + 1, shape[2]), dtype=np.uint8), 6, 0), 6, 1)
        roundtrip(np.ascontiguousarray(up[:shape[0], :shape[1]]), ("upsampled", shape))
        m = rng.integers(0, 256, shape, dtype=np.uint8)
        m[rng.random(shape[:2]) < 0.7] = 7
        roundtrip(m, ("mixed", shape))
    f = [1, 1]
    while len(f) < 24:
        f.append(f[-1] + f[-2])
    vals = np.concatenate([np.full(c, v * 7 % 256, np.uint8) for v, c in enumerate(f)])
    rng.shuffle(vals)
    roundtrip(vals[:vals.size // 12 * 12].reshape(-1, 4, 3), "fibonacci")
    big = rng.integers(0, 256, (300, 400, 3), dtype=np.uint8)
    roundtrip(big[10:200, 20:300], "view")
    # the chunk CRCs come from the carry-less-multiply CRC-32 where the CPU has it (pngenc.hip crc32_clmul); S2SR_CRC_TABLES=1
    # selects the table walk: a fresh process with it must write the same files
    import subprocess
    import sys
    code = ("import sys, numpy as np; sys.path.insert(0, %r); from s2sr import native; "
            "rng = np.random.default_rng(3); "
            "sys.stdout.buffer.write(b''.join(native.png_encode(rng.integers(0, 256, s, dtype=np.uint8)) for s in ((3, 5, 3), (40, 41, 4), (256, 256, 4))))"
            % str(Path(__file__).resolve().parent.parent / "sentinel2-super-resolution-poc_amd"))
    outs = [subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, check=True).stdout
            for env in ({}, {"S2SR_CRC_TABLES": "1"})]
    assert len(outs[0]) > 1000 and outs[0] == outs[1]
    # a compressible tile must actually compress, about as well as zlib with the same settings
    yy, xx = np.mgrid[0:256, 0:256]
    tile = np.empty((256, 256, 4), np.uint8)
    tile[..., :3] = np.clip(110 + 70 * np.sin(xx / 140.0)[..., None] * np.cos(yy / 100.0)[..., None]
                            + np.repeat(np.repeat(rng.integers(-12, 13, (43, 43, 3)), 6, 0), 6, 1)[:256, :256], 0, 255)
    tile[..., 3] = 255
    from app.tiling import _png_from_filtered, filter_sub_rgba
    ref = _png_from_filtered(filter_sub_rgba(tile), 1, zlib.Z_RLE)
    assert len(roundtrip(tile, "tile")) < 1.03 * len(ref)
    # the banded writer on both routes (native: level 1 + Z_RLE; zlib: anything else)
    a = rng.integers(0, 256, (300, 401, 3), dtype=np.uint8)
    a[50:200] = 9
    for kw in (dict(), dict(level=3), dict(strategy=zlib.Z_DEFAULT_STRATEGY)):
        for workers in (None, 1, 4):
            got = np.asarray(Image.open(io.BytesIO(rio.encode_png(a, band_rows=64, workers=workers, **kw))))
            assert np.array_equal(got, a), (kw, workers)
    with pytest.raises(ValueError):
        native.png_encode(np.zeros((4, 4, 2), np.uint8))


def test_native_tile_writer(tmp_path):
    """s2sr_png_write_tiles: a row of RGBA tiles -> z/x/y.png files in one native call (directories on demand, fully transparent
    tiles skipped, None paths skipped), and an unwritable path is an error, not a silent loss."""
    from s2sr import native
    rng = np.random.default_rng(4)
    t = rng.integers(0, 256, (5, 64, 64, 4), dtype=np.uint8)
    t[..., 3] = 255
    t[1, ..., 3] = 0                                   # outside the raster
    t[2, :, :32, 3] = 0                                # half covered: written
    paths = [tmp_path / "18" / str(100 + i) / "7.png" for i in range(5)]
    paths[3] = None
    wrote = native.png_write_tiles(t, paths)
    assert wrote.tolist() == [1, 0, 1, 0, 1]
    assert not (tmp_path / "18" / "101").exists() and not (tmp_path / "18" / "103").exists()
    for i in (0, 2, 4):
        assert np.array_equal(np.asarray(Image.open(paths[i])), t[i])
    assert native.png_write_tiles(t[1:2], [tmp_path / "x.png"], skip_transparent=False).tolist() == [1]
    big = rng.integers(0, 256, (2, 3, 64, 64, 4), dtype=np.uint8)               # a slice of a level array: tiles one stride apart
    native.png_write_tiles(big[1, 0:2], [tmp_path / "a.png", tmp_path / "b.png"], skip_transparent=False)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "b.png")), big[1, 1])
    (tmp_path / "file").write_bytes(b"x")
    with pytest.raises(native.S2srError, match="could not be written"):
        native.png_write_tiles(t[:1], [tmp_path / "file" / "sub" / "1.png"])
    with pytest.raises(ValueError):
        native.png_write_tiles(t, paths[:2])


def test_host_codec_under_address_and_ub_sanitizers(tmp_path):
    """csrc/hostcodec.hip holds no device code: built with g++ -fsanitize=address,undefined into tests/native/fuzz_hostcodec.cpp's
    harness (round trips at exact buffer sizes, short buffers, truncated / bit-flipped / random streams)."""
    import shutil
    import subprocess
    from pathlib import Path
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "fuzz_hostcodec"
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-x", "c++",
           str(root / "tests" / "native" / "fuzz_hostcodec.cpp"),
           str(root / "sentinel2-super-resolution-poc_amd" / "csrc" / "hostcodec.hip"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe), "1500"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok 1500 cases" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    # the PNG encoder: every file parsed, inflated with zlib and un-filtered back to the pixels; exact-size buffers
    exe2 = tmp_path / "fuzz_pngenc"
    b = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-x", "c++",
                        str(root / "tests" / "native" / "fuzz_pngenc.cpp"),
                        str(root / "sentinel2-super-resolution-poc_amd" / "csrc" / "pngenc.hip"), "-lz", "-o", str(exe2)],
                       capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("zlib.h" in b.stderr or "-lz" in b.stderr):
        pytest.skip("zlib development files not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe2), "400"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok 400 cases" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
