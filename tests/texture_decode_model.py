"""The image-texture decoder of include/rfwhip.h (rfwhip_set_texture_sources) in numpy: a general baseline marker walk (jpeg_model.walk
takes only the project's own header), Huffman decoding, the 13-bit "slow integer" inverse DCT in wrapping int32, the decoders' "fancy"
chroma upsampling, integer colour conversion, the modifiers and the reference's mip filter.  Nothing here calls the library.  Results
are cached per process (decode_cached), as display_jpeg_checks.model does."""
import numpy as np

import jpeg_model as jm

FLIP_ROWS, LINEARIZE_REFERENCE, LINEARIZE_SRGB = 1, 2, 4
MIP_LEVELS = 5


class Unsupported(ValueError):
    pass


class Invalid(ValueError):
    pass


def walk(stream):
    """-> dict(w, h, ncomp, hs, vs, ri, q {id: 64 in zigzag order}, huff {(class, id): {(len, code): symbol}}, tq, td, ta,
    intervals [the unstuffed entropy bytes of every restart interval])."""
    d = bytes(stream)
    if d[:2] != b"\xff\xd8":
        raise Invalid("no SOI")
    info = dict(q={}, huff={}, ri=0, hs=1, vs=1)
    p, adobe = 2, None
    while True:
        if p + 2 > len(d) or d[p] != 0xFF:
            raise Invalid("no marker at %d" % p)
        while p < len(d) and d[p] == 0xFF:
            p += 1
        m = d[p]
        p += 1
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        n = int.from_bytes(d[p:p + 2], "big")
        if n < 2 or p + n > len(d):
            raise Invalid("truncated segment")
        b = d[p + 2:p + n]
        p += n
        if m == 0xC2:
            raise Unsupported("progressive")
        if m in (0xC3, 0xC5, 0xC6, 0xC7) or 0xC9 <= m <= 0xCF:
            raise Unsupported("SOF%d" % (m - 0xC0))
        if m in (0xC0, 0xC1):
            if b[0] != 8:
                raise Unsupported("precision")
            info["h"], info["w"], info["ncomp"] = int.from_bytes(b[1:3], "big"), int.from_bytes(b[3:5], "big"), b[5]
            if info["ncomp"] not in (1, 3):
                raise Unsupported("components")
            comps = [(b[6 + 3 * i], b[7 + 3 * i], b[8 + 3 * i]) for i in range(info["ncomp"])]
            info["ids"], info["tq"] = [c[0] for c in comps], [c[2] for c in comps]
            if info["ncomp"] == 3:
                if comps[0][1] not in (0x11, 0x21, 0x22) or comps[1][1] != 0x11 or comps[2][1] != 0x11:
                    raise Unsupported("sampling")
                info["hs"], info["vs"] = comps[0][1] >> 4, comps[0][1] & 15
        elif m == 0xDB:
            while b:
                if b[0] >> 4:
                    raise Unsupported("16-bit DQT")
                info["q"][b[0] & 15] = np.array(list(b[1:65]), np.int32)
                b = b[65:]
        elif m == 0xC4:
            while b:
                bits = list(b[1:17])
                n_sym = sum(bits)
                table = jm.codes((bits, list(b[17:17 + n_sym])))
                info["huff"][(b[0] >> 4, b[0] & 15)] = {(length, code): sym for sym, (code, length) in table.items()}
                b = b[17 + n_sym:]
        elif m == 0xDD:
            info["ri"] = int.from_bytes(b, "big")
        elif m == 0xEE and b[:5] == b"Adobe":
            adobe = b[11]
        elif m == 0xDA:
            if b[0] != info["ncomp"]:
                raise Unsupported("non-interleaved")
            if info["ncomp"] == 3 and adobe not in (None, 1):
                raise Unsupported("APP14 transform")
            info["td"] = [b[2 + 2 * i] >> 4 for i in range(b[0])]
            info["ta"] = [b[2 + 2 * i] & 15 for i in range(b[0])]
            break
    intervals, cur, expect = [], bytearray(), 0
    while True:
        q = d.find(b"\xff", p)
        if q < 0 or q + 1 >= len(d):
            raise Invalid("no EOI")
        cur += d[p:q]
        nxt = d[q + 1]
        if nxt == 0:
            cur.append(0xFF)
            p = q + 2
        elif nxt == 0xFF:
            p = q + 1
        elif 0xD0 <= nxt <= 0xD7:
            if nxt - 0xD0 != expect:
                raise Invalid("RST out of sequence")
            expect = (expect + 1) & 7
            intervals.append(bytes(cur))
            cur = bytearray()
            p = q + 2
        elif nxt == 0xD9:
            intervals.append(bytes(cur))
            break
        else:
            raise Unsupported("marker %02X inside the scan" % nxt)
    info["intervals"] = intervals
    hs, vs = info["hs"], info["vs"]
    info["mw"], info["mh"] = -(-info["w"] // (8 * hs)), -(-info["h"] // (8 * vs))
    info["bpm"] = 1 if info["ncomp"] == 1 else hs * vs + 2
    return info


def decode_coefficients(info):
    """blocks x 64 int32 in zigzag order, in stream order (MCU by MCU: the luma blocks row by row, Cb, Cr)."""
    mcus, bpm, luma = info["mw"] * info["mh"], info["bpm"], info["bpm"] - (info["ncomp"] - 1)
    ri = info["ri"] or mcus
    out = np.zeros((mcus * bpm, 64), np.int32)
    blk = 0
    for data in info["intervals"]:
        n_mcu = min(ri, mcus - blk // bpm)
        total = 8 * len(data)
        acc, pos = int.from_bytes(data, "big"), 0

        def symbol(table):
            nonlocal pos
            for length in range(1, 17):
                code = (acc >> (total - pos - length)) & ((1 << length) - 1)
                if (length, code) in table:
                    pos += length
                    return table[(length, code)]
            raise Invalid("no code")

        def receive(s):
            nonlocal pos
            v = (acc >> (total - pos - s)) & ((1 << s) - 1)
            pos += s
            return v if v >= 1 << (s - 1) else v - (1 << s) + 1
        pred = [0, 0, 0]
        for _ in range(n_mcu):
            for k in range(bpm):
                c = 0 if k < luma else 1 + k - luma
                s = symbol(info["huff"][(0, info["td"][c])])
                if s:
                    pred[c] += receive(s)
                out[blk, 0] = pred[c]
                kk, ac = 1, info["huff"][(1, info["ta"][c])]
                while kk < 64:
                    rs = symbol(ac)
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        kk += 16
                        continue
                    kk += r
                    if kk > 63:
                        raise Invalid("run past 63")
                    out[blk, kk] = receive(s)
                    kk += 1
                blk += 1
        if pos > total:
            raise Invalid("truncated interval")
    return out


def _idct_1d(i):
    """Eight int32 arrays -> the eight sums before the descale (wrapping int32)."""
    z1 = (i[2] + i[6]) * 4433
    e2, e3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    e0, e1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]


def idct(zz, q):
    """N x 64 coefficients and a table, both in zigzag order -> N x 8 x 8 samples (uint8)."""
    with np.errstate(over="ignore"):
        nat = np.zeros(zz.shape, np.int32)
        nat[:, jm.ZZ] = zz.astype(np.int32) * q.astype(np.int32)
        F = nat.reshape(-1, 8, 8)
        ws = np.stack([(o + np.int32(1 << 10)) >> 11 for o in _idct_1d([F[:, u, :] for u in range(8)])], 1)  # [n, u, column]
        px = np.stack([(o + np.int32(1 << 17)) >> 18 for o in _idct_1d([ws[:, :, x] for x in range(8)])], 2)  # [n, row, x]
        return np.clip(px + 128, 0, 255).astype(np.uint8)


def _plane(blocks, bh, bw):
    """bh x bw blocks of 8 x 8 -> the plane."""
    return blocks.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _upsample_h2v1(c):
    c = c.astype(np.int64)
    lf, rt = np.hstack([c[:, :1], c[:, :-1]]), np.hstack([c[:, 1:], c[:, -1:]])
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * c + lf + 1) >> 2, (3 * c + rt + 2) >> 2
    return out


def upsample(c, hs, vs):
    """A chroma component at its own size -> the image's grid (at least the image's size)."""
    if hs == 1:
        return c.astype(np.int64)
    if c.shape[1] <= 2:  # the decoders' rule: no triangle filter on a component at most two columns wide
        return np.repeat(np.repeat(c, vs, 0), hs, 1).astype(np.int64)
    return jm._upsample_fancy(c) if vs == 2 else _upsample_h2v1(c)


def FIX(x):
    return int(x * 65536 + 0.5)


def planes(info, coef):
    """The components' planes (whole blocks) from the coefficients."""
    mh, mw, bpm, hs, vs = info["mh"], info["mw"], info["bpm"], info["hs"], info["vs"]
    z = coef.reshape(mh, mw, bpm, 64)
    luma = bpm - (info["ncomp"] - 1)
    ys = z[:, :, :luma].reshape(mh, mw, vs, hs, 64).transpose(0, 2, 1, 3, 4).reshape(-1, 64)
    out = [_plane(idct(ys, info["q"][info["tq"][0]]), mh * vs, mw * hs)]
    for c in range(1, info["ncomp"]):
        out.append(_plane(idct(z[:, :, luma + c - 1].reshape(-1, 64), info["q"][info["tq"][c]]), mh, mw))
    return out


def decode(stream, flags=0):
    """-> (H x W x 4 uint8 with alpha 255 and the modifiers applied, the coefficients as int16, the walk's info)."""
    info = walk(stream)
    coef = decode_coefficients(info)
    pl = planes(info, coef)
    h, w, hs, vs = info["h"], info["w"], info["hs"], info["vs"]
    Y = pl[0][:h, :w].astype(np.int64)
    if info["ncomp"] == 1:
        R = G = B = Y
    else:
        ch, cw = -(-h // vs), -(-w // hs)
        cb, cr = (upsample(p[:ch, :cw], hs, vs)[:h, :w] - 128 for p in pl[1:])
        R = Y + ((FIX(1.402) * cr + 32768) >> 16)
        B = Y + ((FIX(1.772) * cb + 32768) >> 16)
        G = Y + ((-FIX(0.34414) * cb + 32768 - FIX(0.71414) * cr) >> 16)
    rgba = np.stack([np.clip(R, 0, 255), np.clip(G, 0, 255), np.clip(B, 0, 255), np.full_like(Y, 255)], -1).astype(np.uint8)
    return modify(rgba, flags), coef.astype(np.int16), info


_CACHE = {}


def decode_cached(stream, flags=0):
    key = (bytes(stream), flags)
    if key not in _CACHE:
        _CACHE[key] = decode(stream, flags)
    return _CACHE[key]


def srgb_table():
    c = np.arange(256) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    return np.floor(lin * 255.0 + 0.5).astype(np.uint8)


def modify(rgba, flags):
    """H x W x 4 uint8 in file order -> the texels of level 0: flip, then the linearisation of the three colour bytes."""
    out = np.array(rgba[::-1] if flags & FLIP_ROWS else rgba, np.uint8)
    if flags & LINEARIZE_REFERENCE:
        c = out[..., :3].astype(np.uint32)
        out[..., :3] = (c * c) >> 8
    elif flags & LINEARIZE_SRGB:
        out[..., :3] = srgb_table()[out[..., :3]]
    return np.ascontiguousarray(out)


def chain(level0):
    """H x W x 4 uint8 -> the five levels back to back as uint32 texels (r | g << 8 | b << 16 | a << 24): colours the truncated quarter
    of the aligned 2 x 2 quad's sum, alpha its minimum; level i is (w >> i) x (h >> i)."""
    levels, cur = [np.ascontiguousarray(level0, np.uint8)], level0
    for _ in range(1, MIP_LEVELS):
        h, w = cur.shape[0] >> 1, cur.shape[1] >> 1
        q = cur[:2 * h, :2 * w].reshape(h, 2, w, 2, 4).astype(np.uint32)
        nxt = np.empty((h, w, 4), np.uint8)
        nxt[..., :3] = (q[..., :3].sum(axis=(1, 3)) >> 2)
        nxt[..., 3] = q[..., 3].min(axis=(1, 3)) if h and w else 0
        levels.append(nxt)
        cur = nxt
    return np.concatenate([np.ascontiguousarray(lv).view(np.uint32).reshape(-1) for lv in levels])


def chain_texels(w, h):
    return sum((w >> i) * (h >> i) for i in range(MIP_LEVELS))
