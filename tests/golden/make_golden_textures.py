"""Writes tests/golden/texture_streams.npz: small JPEG streams ENCODED by Pillow from the synthetic images of tests/jpeg_model.py with
Pillow's DECODE of each, and hand-built PNG files (Pillow does not let a caller force a row filter) with Pillow's RGBA of each.  The
tests compare the numpy model (tests/texture_decode_model.py) and the library with these byte for byte; no test imports Pillow.
Run where Pillow is installed:  python tests/golden/make_golden_textures.py"""
import io
import os
import struct
import sys
import zlib

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_model as jm  # noqa: E402

SIZES = [(1, 1), (7, 5), (8, 8), (17, 9), (33, 17), (5, 4), (4, 9)]
SUBS = ["444", "422", "420", "grey"]
KINDS = ["smooth", "noise", "black_white", "checker", "constant"]


def pillow_jpeg(rgb, sub, quality, optimize, restart, **extra):
    im = Image.fromarray(rgb).convert("L") if sub == "grey" else Image.fromarray(rgb)
    buf = io.BytesIO()
    kw = dict(quality=quality, optimize=optimize, **extra)
    if sub != "grey":
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[sub]
    if restart:
        kw["restart_marker_blocks"] = restart
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_decode(stream):
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))


def png_file(w, h, color_type, rows, filters, palette=None, trns=None, interlace=0):
    """rows: h byte strings of unfiltered scanlines; filters: the filter type of each row."""
    bpp = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[color_type]
    raw, prev = bytearray(), bytes(len(rows[0]))
    for row, f in zip(rows, filters):
        out = bytearray([f])
        for i, x in enumerate(row):
            a = row[i - bpp] if i >= bpp else 0
            b, c = prev[i], (prev[i - bpp] if i >= bpp else 0)
            if f == 4:
                e = a + b - c
                pa, pb, pc = abs(e - a), abs(e - b), abs(e - c)
                pr = a if pa <= pb and pa <= pc else b if pb <= pc else c
            else:
                pr = (0, a, b, (a + b) >> 1)[f]
            out.append((x - pr) & 255)
        raw += out
        prev = row

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color_type, 0, 0, interlace))
    if palette is not None:
        out += chunk(b"PLTE", bytes(palette))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    data = zlib.compress(bytes(raw), 9)
    half = len(data) // 2  # (two IDAT chunks: a reader has to join them)
    return out + chunk(b"IDAT", data[:half]) + chunk(b"IDAT", data[half:]) + chunk(b"IEND", b"")


def main():
    out = {}
    k = 0
    for (w, h) in SIZES:
        for sub in SUBS:
            kind = KINDS[k % len(KINDS)]
            quality, optimize, restart = (25, 90)[k % 2], bool((k // 2) % 2), (0, 1, 5)[k % 3]
            rgb = np.ascontiguousarray(getattr(jm, kind)(w, h)[..., :3])
            name = "%dx%d_%s_q%d_%s_r%d_%s" % (w, h, sub, quality, "opt" if optimize else "std", restart, kind)
            s = pillow_jpeg(rgb, sub, quality, optimize, restart)
            out["jpg_" + name], out["dec_" + name] = np.frombuffer(s, np.uint8), pillow_decode(s)
            k += 1
    # a COM segment and an APP1 segment in front of the tables
    rgb = np.ascontiguousarray(jm.smooth(33, 17)[..., :3])
    s = pillow_jpeg(rgb, "420", 90, False, 5, comment=b"a comment segment", exif=b"Exif\x00\x00MM\x00\x2a\x00\x00\x00\x08\x00\x00\x00\x00\x00\x00")
    assert b"\xff\xfe" in s and b"\xff\xe1" in s
    out["jpg_33x17_420_com_app1"], out["dec_33x17_420_com_app1"] = np.frombuffer(s, np.uint8), pillow_decode(s)
    # forms the library refuses: a progressive stream, and a header that declares 4:4:0 (luma 1 x 2: Pillow writes none, so the
    # sampling byte of a 4:2:2 stream's frame header is edited; the refusal comes from the header alone)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=90, progressive=True)
    out["unsupported_progressive"] = np.frombuffer(buf.getvalue(), np.uint8)
    s = bytearray(pillow_jpeg(rgb, "422", 90, False, 0))
    i = s.index(b"\xff\xc0")
    assert s[i + 11] == 0x21
    s[i + 11] = 0x12
    out["unsupported_440"] = np.frombuffer(bytes(s), np.uint8)
    # PNG: the five colour types, the five filters in rotation (each forced at least once per file of five rows or more)
    rng = np.random.default_rng(11)
    for ct, (w, h) in ((0, (7, 5)), (2, (17, 9)), (3, (5, 6)), (4, (8, 8)), (6, (33, 17))):
        ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ct]
        px = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        if ct == 6:
            px[::3, ::2, 3] = 0
        palette = trns = None
        if ct == 3:
            px = (px % 6).astype(np.uint8)
            palette, trns = rng.integers(0, 256, 18, dtype=np.uint8).tolist(), [255, 0, 128, 7]
        f = png_file(w, h, ct, [px[y].tobytes() for y in range(h)], [(y + ct) % 5 for y in range(h)], palette, trns)
        name = "type%d_%dx%d" % (ct, w, h)
        out["png_" + name] = np.frombuffer(f, np.uint8)
        out["rgba_" + name] = np.asarray(Image.open(io.BytesIO(f)).convert("RGBA"))
    px = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
    out["png_interlaced"] = np.frombuffer(png_file(4, 4, 2, [px[y].tobytes() for y in range(4)], [0] * 4, interlace=1), np.uint8)
    out["versions"] = np.array(["Pillow " + Image.__version__, "libjpeg " + str(features.version("jpg")),
                                "libjpeg-turbo " + str(features.version_feature("libjpeg_turbo"))])
    path = os.path.join(HERE, "texture_streams.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
