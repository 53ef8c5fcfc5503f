"""numpy model of the sky's loaders (csrc/sky_load.h; include/rfwhip.h, rfwhip_set_sky_hdr and sky_table=device): an encoder and a
decoder for Radiance .hdr files written from the format's description — the reference ships no .hdr file, so the model writes its
own — and the judging rules for an alias table: what every table must satisfy whoever built it, with bounds counted from the number
formats and the shapes of the sums, not from any implementation's results."""
import math

import numpy as np

FLIP_ROWS = 1
VALID, DEVICE = 1, 2
THREADS, ITEMS, B = 256, 4, 1024  # the table's shapes (sky_load.h: SKYTAB_*)


# ---- Radiance files ----------------------------------------------------------------------------------------------------------
def header(w, h, fmt="32-bit_rle_rgbe", res=None, magic=b"#?RADIANCE", extra=b"", blank=True):
    res = res if res is not None else b"-Y %d +X %d" % (h, w)
    return magic + b"\n# written by the model\n" + extra + b"FORMAT=" + fmt.encode() + b"\n" + (b"\n" if blank else b"") + res + b"\n"


def rle_plane(row):
    """One component plane -> count bytes: runs of three or more equal bytes as (128 + n, value), n <= 127 (a longer run splits),
    the bytes between them as literals of at most 128."""
    row = [int(x) for x in row]
    out, i, n, lit = bytearray(), 0, len(row), []

    def flush():
        while lit:
            k = min(128, len(lit))
            out.append(k)
            out.extend(lit[:k])
            del lit[:k]
    while i < n:
        j = i
        while j < n and row[j] == row[i]:
            j += 1
        if j - i >= 3:
            flush()
            left = j - i
            while left:
                k = min(127, left)
                out.extend((128 + k, row[i]))
                left -= k
        else:
            lit.extend(row[i:j])
        i = j
    flush()
    return bytes(out)


def rle_scanline(line):
    w = len(line)
    return bytes((2, 2, w >> 8, w & 255)) + b"".join(rle_plane(line[:, c]) for c in range(4))


def encode(rgbe, mode="rle", **head):
    """H x W x 4 uint8 -> a file.  mode: "rle", "flat", or "mixed" (even scanlines RLE, odd ones flat)."""
    h, w = rgbe.shape[:2]
    body = b""
    for y in range(h):
        flat = mode == "flat" or (mode == "mixed" and y % 2 == 1) or w < 8 or w > 32767
        body += rgbe[y].tobytes() if flat else rle_scanline(rgbe[y])
    return header(w, h, **head) + body


def rgbe_to_float(rgbe):
    """rgb = mantissa 2^(e - 136), all three 0 when e = 0; the fourth channel 0.  Exact in float32 (subnormal for small e)."""
    e = rgbe[..., 3].astype(np.int32)
    out = np.zeros(rgbe.shape[:2] + (4,), np.float32)
    out[..., :3] = np.ldexp(rgbe[..., :3].astype(np.float32), (e - 136)[..., None]).astype(np.float32)
    out[e == 0] = 0
    return out


def decode(data, flip=False):
    """A file's bytes -> H x W x 4 float32, row 0 the first scanline (the last with flip).  A plain reader of well-formed files."""
    data = bytes(data)
    p = data.index(b"\n\n") + 2
    q = data.index(b"\n", p)
    tok = data[p:q].split()
    assert tok[0] == b"-Y" and tok[2] == b"+X", tok
    h, w = int(tok[1]), int(tok[3])
    p = q + 1
    rgbe = np.zeros((h, w, 4), np.uint8)
    for y in range(h):
        if 8 <= w <= 32767 and data[p] == 2 and data[p + 1] == 2 and data[p + 2] < 128:
            assert (data[p + 2] << 8 | data[p + 3]) == w
            p += 4
            for c in range(4):
                x = 0
                while x < w:
                    n = data[p]
                    if n > 128:
                        rgbe[y, x:x + n - 128, c] = data[p + 1]
                        x, p = x + n - 128, p + 2
                    else:
                        rgbe[y, x:x + n, c] = np.frombuffer(data[p + 1:p + 1 + n], np.uint8)
                        x, p = x + n, p + 1 + n
                assert x == w
        else:
            rgbe[y] = np.frombuffer(data[p:p + 4 * w], np.uint8).reshape(w, 4)
            p += 4 * w
    out = rgbe_to_float(rgbe)
    return out[::-1].copy() if flip else out


def sample_rgbe(w, h, seed=1):
    """Texels that exercise the format: long runs (one longer than 127 where the width allows), literals, exponent 0 with non-zero
    mantissas, mantissa 0 under a non-zero exponent, exponents 1 and 255 — and no flat-form hazards (2 2 hi<128 at a scanline's start,
    1 1 1 e anywhere)."""
    rng = np.random.default_rng(seed + 977 * w + h)
    px = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    px[..., 3] = rng.integers(100, 150, (h, w))
    for y in range(h):
        x = 0
        while x < w:  # alternate noise and runs of random length
            n = int(rng.integers(1, 12))
            if rng.random() < 0.5:
                px[y, x:x + n] = px[y, x]
            x += n
    if w >= 130:
        px[0, 1:130, 0] = 77  # a run of 129: splits at 127
        px[h - 1, :, 3] = 128  # a run of the whole width in the exponent plane
    flat = px.reshape(-1, 4)
    if w < 130:  # (the special texels; at width 130 they would cut the long run, and widths 7, 8 and 33 carry them in every form)
        flat[0] = (9, 200, 31, 0)  # exponent 0: black whatever the mantissas
        flat[1] = (0, 0, 0, 140)  # mantissa 0
        flat[2] = (255, 1, 128, 1)  # exponent 1: subnormal floats
        flat[3] = (255, 128, 1, 255)  # exponent 255
        flat[4] = (0, 255, 0, 129)
    bad = (px[..., 0] == 1) & (px[..., 1] == 1) & (px[..., 2] == 1)
    px[bad, 0] = 3
    px[(px[:, 0, 0] == 2) & (px[:, 0, 1] == 2), 0, 0] = 5
    return px


# ---- the alias table -----------------------------------------------------------------------------------------------------------
def solid_angles(w, h):
    j = np.arange(h, dtype=np.float64)
    return (2.0 * np.pi / w) * (np.cos(np.pi * j / h) - np.cos(np.pi * (j + 1) / h))


def weights(px, w, h):
    """w_k = lum_k omega_row(k) in float64, lum 0 for a negative or NaN texel."""
    px = np.asarray(px, np.float32).reshape(h, w, -1).astype(np.float64)
    lum = 0.2126 * px[..., 0] + 0.7152 * px[..., 1] + 0.0722 * px[..., 2]
    lum = np.where(lum > 0, lum, 0.0)
    return (lum * solid_angles(w, h)[:, None]).reshape(-1)


def sum_depth(n):
    """Additions on the longest path of the device's sum of n weights: a thread's 3, the fold's 8, the strided chain over the
    partials, the fold's 8."""
    nb1 = -(-n // B)
    return (ITEMS - 1) + 8 + -(-nb1 // THREADS) + 8


def scan_depth(n):
    """Roundings on the longest path to one prefix value: a thread's chain, the chain over the 256 threads, over the 1024 blocks of a
    super-block, over the super-blocks, and the two additions of k_skytab_scan_apply plus the one of the block-local value."""
    nb1 = -(-n // B)
    nb2 = -(-nb1 // B)
    return (ITEMS - 1) + THREADS + min(nb1, B) + nb2 + 3


def implied(table, n):
    """The distribution a table describes: P_t = (keep_t + sum over k != t with alias_k = t of (1 - keep_k)) / n, and m_t, the number
    of those k."""
    keep, alias = table["keep"].astype(np.float64), table["alias"].astype(np.int64)
    other = alias != np.arange(n)
    p = keep + np.where(other, 0.0, 1.0 - keep)  # a bucket that names itself keeps everything
    p = p + np.bincount(alias[other], weights=(1.0 - keep)[other], minlength=n)
    m = np.bincount(alias[other], minlength=n)
    return p / n, m


def check_table(table, w, S, label, device=True):
    """What every alias table over the weights w with total S must satisfy.  device: the closed form's extra promises (every alias
    is a heavy texel; the host's Vose build may leave a rounding residue on a light one)."""
    n = len(w)
    assert len(table) == n, (label, len(table))
    keep, alias = table["keep"], table["alias"].astype(np.int64)
    assert (alias >= 0).all() and (alias < n).all(), label
    assert (keep >= 0).all() and (keep <= 1).all(), (label, float(keep.min()), float(keep.max()))
    zero = w == 0
    other = alias != np.arange(n)
    assert (keep[zero] == 0).all(), (label, "a texel of weight 0 keeps itself")
    assert not zero[alias[other]].any() and not zero[alias[zero]].any(), (label, "a texel of weight 0 is somebody's alias")
    mu = S / n
    if device:
        assert (w[alias[other]] > mu).all(), (label, "an alias that is not heavy")
    p, m = implied(table, n)
    # each of the m_t + 1 terms carries the rounding of one `keep` to float32: half an ulp of a number <= 1 is 2^-25; the issue's
    # factor of two makes it 2^-24.  The scan's term: the mass a heavy texel receives is a difference of prefix values (two ends in
    # D, one or two in E), each with a relative error of at most scan_depth roundings of 2^-53 on a value <= S, and mu = fl(S / n)
    # adds one more: 8 (depth + 1) 2^-53 in units of probability covers four such ends with a factor of two.
    bound = (m + 1) * 2.0 ** -24 / n + 8.0 * (scan_depth(n) + 1) * 2.0 ** -53
    err = np.abs(p - w / S)
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), (label, "texel %d: |P - w / S| = %.3e, bound %.3e, m = %d" % (worst, err[worst], bound[worst], m[worst]))
    return float((err / bound).max())


def check_record(rec, w, label):
    """The record of a device-built table against the float64 weights."""
    n = len(w)
    exact = math.fsum(w)
    if not (exact > 0 and math.isfinite(exact)):
        assert not rec["flags"] & VALID, (label, rec)
        return
    assert rec["flags"] == VALID | DEVICE, (label, rec)
    # non-negative terms: every addition on the path loses at most 2^-53 of the running sum, fsum itself rounds once
    assert abs(rec["S"] - exact) <= (sum_depth(n) + 1) * 2.0 ** -53 * exact, (label, rec["S"], exact, sum_depth(n))
    assert rec["heaviest"] == int(np.argmax(w)), (label, rec["heaviest"], int(np.argmax(w)))
    mu = rec["S"] / n
    assert rec["heavy"] == int((w > mu).sum()) and rec["light"] == n - rec["heavy"], (label, rec)


def weight_vectors(n, seed=3):
    """The vectors of the issue at size n: constant, a single spike, 70 % zeros, and one with a NaN and a negative entry."""
    rng = np.random.default_rng(seed + n)
    out = {"constant": np.full(n, 0.37), "uniform": rng.random(n)}
    spike = np.full(n, 1e-3)
    spike[(n * 2) // 3] = 50.0
    out["spike"] = spike
    sparse = rng.random(n) ** 3
    sparse[rng.random(n) < 0.7] = 0.0
    if not sparse.any():
        sparse[n // 2] = 1.0
    out["sparse"] = sparse
    odd = rng.lognormal(0.0, 2.0, n)
    odd[0] = np.nan
    odd[n - 1] = -4.0
    if n > 2:
        odd[n // 2] = 0.0
    out["nan_negative"] = odd
    return out


def sanitised(w):
    w = np.asarray(w, np.float64)
    return np.where(w > 0, w, 0.0)
