"""The baseline JPEG stream of include/rfwhip.h (rfwhip_read_display_jpeg) in numpy: an encoder that follows the definition to the
letter — every step is integer arithmetic, so the library has to agree with it byte for byte — and a decoder of its own (marker
walk, Huffman decode, dequantisation, float64 inverse DCT, upsampling, colour).  Nothing here calls the library."""
import math

import numpy as np

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# T.81 Annex K.1
QL = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
QC = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
# T.81 Annex K.3: (BITS, HUFFVAL)
DCL = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DCC = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
ACL = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
       [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
        0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
        0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
        0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
        0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
        0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
        0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
ACC = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
       [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
        0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
        0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
        0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
        0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
        0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
        0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HEADER_BYTES = 613
BLOCK_BYTES = 416  # the worst case of one block in the stream: 1658 bits -> 208 bytes, every one stuffed
K = np.array([[int(round(8192 * (math.sqrt(1 / 8) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16))) for x in range(8)]
              for u in range(8)], dtype=np.int64)
assert list(K[0]) == [2896] * 8 and list(K[1][:4]) == [4017, 3406, 2276, 799]


def codes(table):
    """symbol -> (code, length) of a (BITS, HUFFVAL) table."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def qtable(base, quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array(base, dtype=np.int64) * s + 50) // 100, 1, 255)


def geometry(w, h, sub, ri):
    m = 16 if sub == "420" else 8
    mw, mh = (w + m - 1) // m, (h + m - 1) // m
    bpm = 6 if sub == "420" else 3
    return dict(m=m, mw=mw, mh=mh, mcus=mw * mh, bpm=bpm, blocks=mw * mh * bpm, intervals=(mw * mh + ri - 1) // ri)


def bound(w, h, sub, ri):
    g = geometry(w, h, sub, ri)
    return HEADER_BYTES + BLOCK_BYTES * g["blocks"] + 2 * g["intervals"]


def planes(rgba, sub):
    """Y, Cb, Cr of the image extended to whole MCUs (int64)."""
    h, w = rgba.shape[:2]
    g = geometry(w, h, sub, 1)
    yi, xi = np.minimum(np.arange(g["mh"] * g["m"]), h - 1), np.minimum(np.arange(g["mw"] * g["m"]), w - 1)
    p = rgba[yi][:, xi].astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + 8421375) >> 16
    if sub == "420":
        def ds(c):
            return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
        Cb, Cr = ds(Cb), ds(Cr)
    return Y, Cb, Cr


def plane_blocks(plane, q):
    """Every 8 x 8 block of a plane -> bh x bw x 64 quantised coefficients in zigzag order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    X = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
    T = (np.einsum("uy,abyx->abux", K, X) + 512) >> 10
    S = np.einsum("abux,vx->abuv", T, K).reshape(bh, bw, 64)
    v = np.sign(S) * ((np.abs(S) + (q << 15)) // (q << 16))
    return v[..., ZZ]


def coefficients(rgba, quality=90, sub="420"):
    """blocks x 64 int16 in stream order (MCU by MCU; Y blocks, Cb, Cr)."""
    h, w = rgba.shape[:2]
    g = geometry(w, h, sub, 1)
    Y, Cb, Cr = planes(rgba, sub)
    ql, qc = qtable(QL, quality), qtable(QC, quality)
    by, bb, br = plane_blocks(Y, ql), plane_blocks(Cb, qc), plane_blocks(Cr, qc)
    mh, mw = g["mh"], g["mw"]
    if sub == "420":
        ys = by.reshape(mh, 2, mw, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mh, mw, 4, 64)
    else:
        ys = by.reshape(mh, mw, 1, 64)
    out = np.concatenate([ys, bb.reshape(mh, mw, 1, 64), br.reshape(mh, mw, 1, 64)], axis=2)
    return out.reshape(-1, 64).astype(np.int16)


def header(w, h, quality, sub, ri):
    out = bytearray(b"\xff\xd8")

    def seg(marker, body):
        out.extend(b"\xff" + bytes([marker]) + (len(body) + 2).to_bytes(2, "big") + body)
    seg(0xe0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    seg(0xdb, bytes([0]) + bytes(qtable(QL, quality)[ZZ].tolist()) + bytes([1]) + bytes(qtable(QC, quality)[ZZ].tolist()))
    seg(0xc0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 0x22 if sub == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    d = b""
    for cls, t in ((0x00, DCL), (0x10, ACL), (0x01, DCC), (0x11, ACC)):
        d += bytes([cls]) + bytes(t[0]) + bytes(t[1])
    seg(0xc4, d)
    seg(0xdd, ri.to_bytes(2, "big"))
    seg(0xda, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == HEADER_BYTES
    return bytes(out)


_HD, _HA = [codes(DCL), codes(DCC)], [codes(ACL), codes(ACC)]


def encode(rgba, quality=90, sub="420", ri=8):
    """-> (the stream, facts about it: what the tests' preconditions ask for)."""
    h, w = rgba.shape[:2]
    g = geometry(w, h, sub, ri)
    coef = coefficients(rgba, quality, sub)
    out = bytearray(header(w, h, quality, sub, ri))
    facts = dict(stuffed=0, dc_category=0, ac_category=0, zrl=0, block_bits=0, intervals=g["intervals"], mcus=g["mcus"], blocks=g["blocks"],
                 eob_free=0, interval_blocks=0, interval_bytes=0)
    bpm = g["bpm"]
    for i0 in range(0, g["mcus"], ri):
        acc, nb, pred, bs = 0, 0, [0, 0, 0], bytearray()
        bits = 0

        def put(c, length):
            nonlocal acc, nb, bits
            acc = (acc << length) | c
            nb += length
            bits += length
            while nb >= 8:
                b = (acc >> (nb - 8)) & 255
                bs.append(b)
                if b == 255:
                    bs.append(0)
                nb -= 8
            acc &= (1 << nb) - 1
        n_mcu = min(ri, g["mcus"] - i0)
        for b in range(i0 * bpm, (i0 + n_mcu) * bpm):
            k = b % bpm
            ci = (0 if k < bpm - 2 else k - (bpm - 3))
            ti = 0 if ci == 0 else 1
            v = coef[b].astype(np.int64)
            start = bits
            dd = int(v[0]) - pred[ci]
            pred[ci] = int(v[0])
            s = abs(dd).bit_length()
            facts["dc_category"] = max(facts["dc_category"], s)
            put(*_HD[ti][s])
            if s:
                put((dd if dd >= 0 else dd - 1) & ((1 << s) - 1), s)
            nz = np.nonzero(v[1:])[0]
            last = int(nz[-1]) + 1 if len(nz) else 0
            run = 0
            for kk in range(1, last + 1):
                a = int(v[kk])
                if a == 0:
                    run += 1
                    continue
                while run > 15:
                    put(*_HA[ti][0xf0])
                    run -= 16
                    facts["zrl"] += 1
                s = abs(a).bit_length()
                facts["ac_category"] = max(facts["ac_category"], s)
                put(*_HA[ti][run * 16 + s])
                put((a if a >= 0 else a - 1) & ((1 << s) - 1), s)
                run = 0
            if last < 63:
                put(*_HA[ti][0])
            else:
                facts["eob_free"] += 1
            facts["block_bits"] = max(facts["block_bits"], bits - start)
        if nb:
            pad = 8 - nb
            put((1 << pad) - 1, pad)
        facts["stuffed"] += bs.count(b"\xff\x00")
        facts["interval_blocks"] = max(facts["interval_blocks"], n_mcu * bpm)
        facts["interval_bytes"] = max(facts["interval_bytes"], len(bs))
        out += bs
        out += bytes([0xff, 0xd0 + ((i0 // ri) & 7)]) if i0 + ri < g["mcus"] else b"\xff\xd9"
    return bytes(out), facts


# ---- the decoder -----------------------------------------------------------------------------------------------------------
def walk(stream):
    """The marker walk: {"segments": [(marker, body)], "w", "h", "sub", "ri", "q": {id: 64 natural}, "huff": {(class, id): {(len, code): symbol}},
    "intervals": [the unstuffed entropy bytes of every restart interval], "markers": [the RSTn numbers in order]}.  Asserts the
    structure: SOI first, EOI last, every RSTn in sequence mod 8, no other marker inside the scan."""
    assert stream[:2] == b"\xff\xd8" and stream[-2:] == b"\xff\xd9"
    p, info = 2, dict(segments=[], q={}, huff={}, ri=0)
    while True:
        assert stream[p] == 0xFF
        marker, n = stream[p + 1], int.from_bytes(stream[p + 2:p + 4], "big")
        body = stream[p + 4:p + 2 + n]
        info["segments"].append((marker, body))
        p += 2 + n
        if marker == 0xDB:
            b = body
            while b:
                assert b[0] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZZ] = list(b[1:65])
                info["q"][b[0] & 15] = t
                b = b[65:]
        elif marker == 0xC0:
            assert body[0] == 8 and body[5] == 3
            info["h"], info["w"] = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            comps = [(body[6 + 3 * i], body[7 + 3 * i], body[8 + 3 * i]) for i in range(3)]
            assert [c[0] for c in comps] == [1, 2, 3] and comps[1][1] == comps[2][1] == 0x11 and comps[0][1] in (0x11, 0x22)
            info["sub"] = "420" if comps[0][1] == 0x22 else "444"
            info["qsel"] = [c[2] for c in comps]
        elif marker == 0xC4:
            b = body
            while b:
                bits = list(b[1:17])
                n_sym = sum(bits)
                table = codes((bits, list(b[17:17 + n_sym])))
                info["huff"][(b[0] >> 4, b[0] & 15)] = {(length, code): sym for sym, (code, length) in table.items()}
                b = b[17 + n_sym:]
        elif marker == 0xDD:
            info["ri"] = int.from_bytes(body, "big")
        elif marker == 0xDA:
            assert list(body) == [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]
            break
    intervals, markers, cur = [], [], bytearray()
    while True:
        b = stream[p]
        if b != 0xFF:
            cur.append(b)
            p += 1
            continue
        nxt = stream[p + 1]
        if nxt == 0:
            cur.append(0xFF)
            p += 2
        elif 0xD0 <= nxt <= 0xD7:
            markers.append(nxt - 0xD0)
            intervals.append(bytes(cur))
            cur = bytearray()
            p += 2
        else:
            assert nxt == 0xD9 and p + 2 == len(stream), "a marker inside the scan, or bytes behind EOI"
            intervals.append(bytes(cur))
            break
    assert markers == [i & 7 for i in range(len(markers))]
    info["intervals"], info["markers"] = intervals, markers
    return info


def decode_coefficients(info):
    """blocks x 64 (zigzag order) from the walked stream; asserts every interval's padding is 1-bits of less than a byte."""
    g = geometry(info["w"], info["h"], info["sub"], info["ri"] or 1 << 30)
    bpm, out = g["bpm"], []
    left = g["mcus"]
    for data in info["intervals"]:
        n_mcu = min(info["ri"] or left, left)
        left -= n_mcu
        bits = "".join(format(b, "08b") for b in data)
        pos, pred = 0, [0, 0, 0]

        def symbol(table):
            nonlocal pos
            code, length = 0, 0
            while True:
                code = (code << 1) | int(bits[pos])
                pos += 1
                length += 1
                if (length, code) in table:
                    return table[(length, code)]
                assert length < 16

        def receive(s):
            nonlocal pos
            if not s:
                return 0
            v = int(bits[pos:pos + s], 2)
            pos += s
            return v if v >= 1 << (s - 1) else v - (1 << s) + 1
        for m in range(n_mcu):
            for k in range(bpm):
                ci = 0 if k < bpm - 2 else k - (bpm - 3)
                ti = 0 if ci == 0 else 1
                z = np.zeros(64, np.int64)
                pred[ci] += receive(symbol(info["huff"][(0, ti)]))
                z[0] = pred[ci]
                kk = 1
                while kk < 64:
                    rs = symbol(info["huff"][(1, ti)])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        kk += 16
                        continue
                    kk += r
                    z[kk] = receive(s)
                    kk += 1
                out.append(z)
        assert len(bits) - pos < 8 and set(bits[pos:]) <= {"1"}
    assert left == 0
    return np.array(out)


def _upsample_fancy(c):
    """2 x 2 "triangle" upsampling of a chroma plane (9 : 3 : 3 : 1 with the edges replicated), in integers, rounding 8 / 7 in
    alternation — what the common decoders do for 4:2:0."""
    c = c.astype(np.int64)
    up, dn = np.vstack([c[:1], c[:-1]]), np.vstack([c[1:], c[-1:]])
    rows = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    rows[0::2], rows[1::2] = 3 * c + up, 3 * c + dn
    lf, rt = np.hstack([rows[:, :1], rows[:, :-1]]), np.hstack([rows[:, 1:], rows[:, -1:]])
    out = np.empty((rows.shape[0], 2 * rows.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * rows + lf + 8) >> 4, (3 * rows + rt + 7) >> 4
    return out


def decode(stream):
    """-> H x W x 3 uint8."""
    info = walk(stream)
    z = decode_coefficients(info)
    g = geometry(info["w"], info["h"], info["sub"], 1)
    mh, mw, bpm = g["mh"], g["mw"], g["bpm"]
    z = z.reshape(mh, mw, bpm, 64)
    Kf = np.array([[(math.sqrt(1 / 8) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)] for u in range(8)])

    def plane(zz, q):  # a x b x 64 zigzag -> the samples
        nat = np.zeros(zz.shape, np.float64)
        nat[..., ZZ] = zz
        F = (nat * q).reshape(zz.shape[0], zz.shape[1], 8, 8)
        px = np.einsum("uy,abuv,vx->abyx", Kf, F, Kf) + 128.0
        return np.clip(np.rint(px), 0, 255).transpose(0, 2, 1, 3).reshape(zz.shape[0] * 8, zz.shape[1] * 8)
    ql, qc = info["q"][info["qsel"][0]], info["q"][info["qsel"][1]]
    if info["sub"] == "420":
        ys = z[:, :, :4].reshape(mh, mw, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mh * 2, mw * 2, 64)
    else:
        ys = z[:, :, 0]
    Y, Cb, Cr = plane(ys, ql), plane(z[:, :, bpm - 2], qc), plane(z[:, :, bpm - 1], qc)
    if info["sub"] == "420":
        # (the decoders upsample the component at its own size, ceil(h / 2) x ceil(w / 2), its edge replicated: not the padding)
        ch, cw = (info["h"] + 1) // 2, (info["w"] + 1) // 2
        Cb, Cr = _upsample_fancy(Cb[:ch, :cw]), _upsample_fancy(Cr[:ch, :cw])
    Y, Cb, Cr = Y[:info["h"], :info["w"]], Cb[:info["h"], :info["w"]] - 128.0, Cr[:info["h"], :info["w"]] - 128.0
    rgb = np.stack([Y + 1.402 * Cr, Y - 0.344136 * Cb - 0.714136 * Cr, Y + 1.772 * Cb], -1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


# ---- the inputs of the tests (seeded; RGBA8 with a varying alpha, which the encoder must ignore) ----------------------------------
SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 9), (67, 35), (130, 70)]
SUBS = ["444", "420"]
QUALITIES = [1, 25, 90, 100]
RESTARTS = [1, 8, 11, 65535]


def _rgba(rgb, seed=7):
    rgb = np.asarray(rgb, np.uint8)
    a = np.random.default_rng(seed).integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, a], -1))


def constant(w, h):
    return _rgba(np.full((h, w, 3), (200, 30, 90), np.uint8))


def smooth(w, h, seed=1):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    im = np.stack([127 + 120 * np.sin(x / 9.) * np.cos(y / 7.), 127 + 100 * np.sin((x + y) / 13.), 127 + 110 * np.cos(x / 5. - y / 11.)], -1)
    return _rgba(np.clip(im + rng.normal(0, 6, im.shape), 0, 255).astype(np.uint8))


def noise(w, h, seed=2):
    return _rgba(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def black_white(w, h, seed=3):
    """8 x 8 blocks of pure black and white: DC differences of category 11 at quality 100."""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 2, ((h + 7) // 8, (w + 7) // 8, 1), dtype=np.uint8) * 255
    cells[0, :2, 0] = (0, 255)[:cells.shape[1]]
    return _rgba(np.kron(cells, np.ones((8, 8, 3), np.uint8))[:h, :w])


def checker(w, h):
    """Black and white pixel by pixel: the AC coefficient (7, 7) alone, of category 10 at quality 100."""
    y, x = np.mgrid[0:h, 0:w]
    return _rgba(np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1))


def cosine(w, h):
    """The highest-frequency cosine (7, 7) on a grey: below quality 100 a lone last coefficient behind 62 zeros -> three ZRL per
    luminance block and no EOB."""
    y, x = np.mgrid[0:h, 0:w]
    v = np.rint(128 + 60 * np.cos((2 * (x % 8) + 1) * 7 * math.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * math.pi / 16))
    return _rgba(np.repeat(v.astype(np.uint8)[..., None], 3, -1))


def worst_case(w, h, seed=5):
    """As close to the worst-case slot as the model can construct.  The bound of 1658 bits per block (every AC coefficient of
    category 10 behind a 16-bit code) is out of reach of 8-bit samples: by Parseval the squared coefficients of a block add up to
    at most 64 x 128^2, which 63 coefficients of 512 and more exceed sixteen times over.  What samples can give is every coefficient
    large at once: blocks whose 63 AC coefficients are +-260 with random signs, transformed back and clipped to 0 .. 255 — at
    quality 100 (every Q = 1) about 990 bits per luminance block, 60 % of the bound, against 780 for uniform noise."""
    rng = np.random.default_rng(seed)
    kf = np.array([[(math.sqrt(1 / 8) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)] for u in range(8)])
    out = np.zeros(((h + 7) // 8 * 8, (w + 7) // 8 * 8), np.float64)
    for by in range(0, out.shape[0], 8):
        for bx in range(0, out.shape[1], 8):
            c = 260.0 * rng.choice([-1.0, 1.0], (8, 8))
            c[0, 0] = 0.0
            out[by:by + 8, bx:bx + 8] = kf.T @ c @ kf + 128.0
    g = np.clip(np.rint(out[:h, :w]), 0, 255).astype(np.uint8)
    return _rgba(np.repeat(g[..., None], 3, -1))


_QUALITY_IMAGES = {}


def quality_image(name):
    """The six images the quality comparison with Pillow's encoder was specified on, drawn in this order from ONE generator
    (seed 1): uniform noise 130 x 70, smooth with noise 130 x 70 and 67 x 35, one pixel, smooth 7 x 5, black and white cells 72 x 40."""
    if not _QUALITY_IMAGES:
        rng = np.random.default_rng(1)

        def sm(h, w):
            y, x = np.mgrid[0:h, 0:w]
            im = np.stack([127 + 120 * np.sin(x / 9.) * np.cos(y / 7.), 127 + 100 * np.sin((x + y) / 13.), 127 + 110 * np.cos(x / 5. - y / 11.)], -1)
            return np.clip(im + rng.normal(0, 6, im.shape), 0, 255).astype(np.uint8)
        _QUALITY_IMAGES["q_noise130x70"] = _rgba(rng.integers(0, 256, (70, 130, 3), dtype=np.uint8))
        _QUALITY_IMAGES["q_smooth130x70"] = _rgba(sm(70, 130))
        _QUALITY_IMAGES["q_smooth67x35"] = _rgba(sm(35, 67))
        _QUALITY_IMAGES["q_one"] = _rgba(rng.integers(0, 256, (1, 1, 3), dtype=np.uint8))
        _QUALITY_IMAGES["q_7x5"] = _rgba(sm(5, 7))
        _QUALITY_IMAGES["q_bw"] = _rgba(np.kron(rng.integers(0, 2, (5, 9, 1), dtype=np.uint8) * 255, np.ones((8, 8, 3), np.uint8)))
    return _QUALITY_IMAGES[name]


for _n in ("q_noise130x70", "q_smooth130x70", "q_smooth67x35", "q_one", "q_7x5", "q_bw"):
    globals()[_n] = (lambda n: lambda w, h: quality_image(n))(_n)
