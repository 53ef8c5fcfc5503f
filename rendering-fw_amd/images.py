"""Image files as texture sources (include/rfwhip.h, rfwhip_set_texture_sources): a JPEG stays encoded — the device decodes it —
and a PNG becomes RGBA8 pixels here (zlib and the row filters), which the device flips, linearises and mips.  What the reference's
rfw::texture does with FreeImage (texture.cpp of its system layer) on the host.  Radiance .hdr files for the sky (rfwhip_set_sky_hdr)
stay encoded as well: load_hdr / hdr_info, and write_hdr, a numpy encoder."""
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


# ---- Radiance .hdr files (include/rfwhip.h, rfwhip_set_sky_hdr): the sky's loader, and an encoder for linear images ---------------
def hdr_info(data, lib=None):
    """The header of a Radiance .hdr file as a dict: width, height, exposure (the product of the EXPOSURE lines, not applied), rle,
    supported, reason.  Host only (rfwhip_hdr_info); a malformed file raises RuntimeError."""
    lib = lib or _lib()
    src = np.frombuffer(bytes(data), np.uint8)
    info = abi.HdrInfo()
    lib.rfwhip_hdr_info.restype, lib.rfwhip_hdr_info.argtypes = C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(abi.HdrInfo)]
    if lib.rfwhip_hdr_info(src.ctypes.data, src.size, C.byref(info)) != 0:
        lib.rfwhip_last_error.restype = C.c_char_p
        raise RuntimeError((lib.rfwhip_last_error() or b"unknown error").decode(errors="replace"))
    return dict(width=int(info.width), height=int(info.height), exposure=float(info.exposure), rle=bool(info.rle),
                supported=bool(info.supported), reason=info.reason.decode(errors="replace"))


def load_hdr(path, ctx, flip=False):
    """The file `path` becomes the sky of `ctx` (a RenderContext or a group): the device decodes it.  Returns hdr_info's dict."""
    with open(path, "rb") as f:
        data = f.read()
    info = hdr_info(data, getattr(ctx, "_lib", None))
    if not info["supported"]:
        raise ValueError("HDR: not a form the device decodes: " + info["reason"])
    ctx.set_sky_hdr(data, flip=flip)
    return info


def rgbe_from_float(rgb):
    """H x W x 3 linear floats -> H x W x 4 uint8 RGBE, Ward's float2rgbe: the shared exponent of the largest component, the
    mantissas truncated; a pixel whose largest component is below 1e-32 (or negative, or NaN) is 0 0 0 0."""
    rgb = np.asarray(rgb, np.float64)
    big = np.nan_to_num(rgb, nan=0.0, posinf=3.0e38).clip(0.0, 3.0e38)
    v = big.max(-1)
    m, e = np.frexp(v)  # v = m 2^e, m in [0.5, 1)
    scale = np.where(v < 1e-32, 0.0, np.ldexp(256.0, -e))
    out = np.zeros(rgb.shape[:2] + (4,), np.uint8)
    out[..., :3] = np.minimum(big * scale[..., None], 255.0).astype(np.uint8)
    out[..., 3] = np.where(v < 1e-32, 0, np.clip(e + 128, 0, 255)).astype(np.uint8)
    out[out[..., 3] == 0] = 0
    return out


def _rle_plane(row):
    """One component plane of a scanline -> its count bytes: runs of at least 4 equal bytes as (128 + n, value) with n <= 127,
    everything else as literals of at most 128 bytes."""
    out, n, i, lit = bytearray(), len(row), 0, 0
    row = bytes(row)

    def flush(upto):
        nonlocal lit
        while lit < upto:
            k = min(128, upto - lit)
            out.append(k)
            out.extend(row[lit:lit + k])
            lit += k
    while i < n:
        j = i + 1
        while j < n and row[j] == row[i] and j - i < 127:
            j += 1
        if j - i >= 4:
            flush(i)
            out.append(128 + (j - i))
            out.append(row[i])
            lit = j
        i = j
    flush(n)
    return bytes(out)


def encode_hdr(rgbe, rle=True, exposure=None):
    """H x W x 4 uint8 RGBE -> the bytes of a Radiance .hdr file (-Y H +X W).  rle: new-style run-length encoding where the format
    allows it (8 <= W <= 32767), flat quadruples otherwise."""
    rgbe = np.ascontiguousarray(rgbe, np.uint8)
    h, w = rgbe.shape[:2]
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n" + (b"EXPOSURE=%g\n" % exposure if exposure is not None else b"") + b"\n-Y %d +X %d\n" % (h, w)
    if not rle or w < 8 or w > 32767:
        # (a flat scanline that begins 2 2 hi<128 would read as an RLE header, a pixel 1 1 1 e as an old-style run)
        first = rgbe[:, 0]
        if (8 <= w <= 32767 and ((first[:, 0] == 2) & (first[:, 1] == 2) & (first[:, 2] < 128)).any()) or \
                ((rgbe[..., 0] == 1) & (rgbe[..., 1] == 1) & (rgbe[..., 2] == 1)).any():
            raise ValueError("HDR: these texels cannot be written flat (a scanline would read as run-length encoded): use rle=True")
        return head + rgbe.tobytes()
    body = bytearray()
    for y in range(h):
        body += bytes((2, 2, w >> 8, w & 255))
        for c in range(4):
            body += _rle_plane(rgbe[y, :, c])
    return head + bytes(body)


def write_hdr(path, rgb, rle=True):
    """Save H x W x 3 (or x 4: the fourth channel is dropped) linear floats as a Radiance .hdr file — a sky for load_hdr, or a linear
    render (framebuffer()[..., :3]).  Values are stored as RGBE: 8-bit mantissas under a shared exponent."""
    rgb = np.asarray(rgb)[..., :3]
    with open(path, "wb") as f:
        f.write(encode_hdr(rgbe_from_float(rgb), rle=rle))
