"""Image files as texture sources (include/rfwhip.h, rfwhip_set_texture_sources): a JPEG stays encoded — the device decodes it —
and a PNG becomes RGBA8 pixels here (zlib and the row filters), which the device flips, linearises and mips.  What the reference's
rfw::texture does with FreeImage (texture.cpp of its system layer) on the host."""
import ctypes as C
import struct
import zlib

import numpy as np

from . import abi

PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _lib():
    from .context import load_library
    return load_library()


def image_info(data, lib=None):
    """The header of a JPEG stream as a dict: width, height, components, h_sampling, v_sampling, restart_interval, intervals,
    supported, reason.  Host only (rfwhip_image_info); a malformed stream raises RuntimeError."""
    lib = lib or _lib()
    src = np.frombuffer(bytes(data), np.uint8)
    info = abi.ImageInfo()
    lib.rfwhip_image_info.restype, lib.rfwhip_image_info.argtypes = C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(abi.ImageInfo)]
    if lib.rfwhip_image_info(src.ctypes.data, src.size, C.byref(info)) != 0:
        lib.rfwhip_last_error.restype = C.c_char_p
        raise RuntimeError((lib.rfwhip_last_error() or b"unknown error").decode(errors="replace"))
    out = {n: int(getattr(info, n)) for n, _ in abi.ImageInfo._fields_ if n != "reason"}
    out["supported"], out["reason"] = bool(out["supported"]), info.reason.decode(errors="replace")
    return out


def _unfilter(raw, h, row_bytes, bpp, lib):
    """h scanlines of a filter byte and row_bytes bytes -> h x row_bytes uint8.  None and Up as whole rows and Sub as a running sum
    when the file uses nothing else; files with Average or Paeth rows go through rfwhip_png_unfilter (a loop per byte)."""
    lines = np.frombuffer(raw, np.uint8).reshape(h, row_bytes + 1)
    types = lines[:, 0]
    if types.max(initial=0) > 4:
        raise ValueError("PNG: filter type %d" % int(types.max()))
    out = np.empty((h, row_bytes), np.uint8)
    if types.max(initial=0) <= 2:
        for y in range(h):
            row = lines[y, 1:]
            if types[y] == 1:  # Sub: the running sum per byte lane
                pad = (-row_bytes) % bpp
                lanes = np.concatenate([row, np.zeros(pad, np.uint8)]).reshape(-1, bpp)
                row = np.cumsum(lanes, axis=0, dtype=np.uint8).reshape(-1)[:row_bytes]
            elif types[y] == 2 and y:
                row = row + out[y - 1]
            out[y] = row
        return out
    lib = lib or _lib()
    src = np.ascontiguousarray(lines)
    lib.rfwhip_png_unfilter.restype = C.c_int
    lib.rfwhip_png_unfilter.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p]
    if lib.rfwhip_png_unfilter(src.ctypes.data, h, row_bytes, bpp, out.ctypes.data) != 0:
        raise ValueError("PNG: the rows could not be unfiltered")
    return out


def decode_png(data, lib=None):
    """A PNG file's bytes -> H x W x 4 uint8 in file order.  8-bit depth, colour types 0 (grey), 2 (RGB), 3 (palette, with tRNS), 4
    (grey + alpha), 6 (RGBA), not interlaced; anything else raises a ValueError naming the form."""
    data = bytes(data)
    if data[:8] != PNG_SIGNATURE:
        raise ValueError("not a PNG file (signature)")
    p, ihdr, palette, trns, idat = 8, None, None, None, []
    while p + 8 <= len(data):
        n, tag = struct.unpack(">I4s", data[p:p + 8])
        body = data[p + 8:p + 8 + n]
        if len(body) != n:
            raise ValueError("PNG: truncated inside chunk %r" % tag)
        p += 12 + n
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"PLTE":
            palette = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif tag == b"tRNS":
            trns = np.frombuffer(body, np.uint8)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
    if ihdr is None or not idat:
        raise ValueError("PNG: no IHDR or no IDAT chunk")
    w, h, depth, ct, _, _, interlace = ihdr
    if interlace:
        raise ValueError("PNG: interlaced (Adam7) files are not supported")
    if depth != 8:
        raise ValueError("PNG: bit depth %d is not supported (8 only)" % depth)
    if ct not in (0, 2, 3, 4, 6):
        raise ValueError("PNG: colour type %d" % ct)
    ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ct]
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != h * (w * ch + 1):
        raise ValueError("PNG: %d bytes of pixel data, %d expected" % (len(raw), h * (w * ch + 1)))
    px = _unfilter(raw, h, w * ch, ch, lib).reshape(h, w, ch)
    out = np.empty((h, w, 4), np.uint8)
    out[..., 3] = 255
    if ct == 0:
        out[..., :3] = px
    elif ct == 2:
        out[..., :3] = px
    elif ct == 3:
        if palette is None or int(px.max(initial=0)) >= len(palette):
            raise ValueError("PNG: a palette index without an entry")
        out[..., :3] = palette[px[..., 0]]
        if trns is not None:
            alpha = np.full(256, 255, np.uint8)
            alpha[:len(trns)] = trns
            out[..., 3] = alpha[px[..., 0]]
    elif ct == 4:
        out[..., :3], out[..., 3] = px[..., :1], px[..., 1]
    else:
        out[...] = px
    return out


def texture_from_bytes(data, flip=False, linearize=None, lib=None):
    """A texture source for set_textures from a file's bytes: a JPEG stays encoded ({"kind": "jpeg"}), a PNG becomes pixels
    ({"kind": "rgba8"}); both carry type, width and height as the finished textures' dicts do.  flip: texel row 0 is the image's bottom row; linearize: None | "reference" (c c >> 8) | "srgb"."""
    flags = (abi.TEXSRC_FLIP_ROWS if flip else 0) | {None: 0, "reference": abi.TEXSRC_LINEARIZE_REFERENCE, "srgb": abi.TEXSRC_LINEARIZE_SRGB}[linearize]
    data = bytes(data)
    if data[:2] == b"\xff\xd8":
        info = image_info(data, lib)
        if not info["supported"]:
            raise ValueError("JPEG: not a form the device decodes: " + info["reason"])
        return {"kind": "jpeg", "data": data, "flags": flags, "type": abi.TEX_UINT, "width": info["width"], "height": info["height"]}
    if data[:8] == PNG_SIGNATURE:
        px = decode_png(data, lib)
        return {"kind": "rgba8", "data": px, "flags": flags, "type": abi.TEX_UINT, "width": px.shape[1], "height": px.shape[0]}
    raise ValueError("neither a JPEG nor a PNG file")


def texture_from_file(path, flip=False, linearize=None, lib=None):
    with open(path, "rb") as f:
        return texture_from_bytes(f.read(), flip, linearize, lib)
