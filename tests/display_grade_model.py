"""A float64 numpy restatement of the display stage's colour grading and dither (csrc/display_grade.h; include/rfwhip.h,
rfwhip_set_display_lut) on top of tests/display_model.py, and the rule by which an image is judged against it.

Every function that restates a float32 step returns the value and a BOUND on |float32 result - float64 value|, counted term by
term with u = 2^-24 (half an ulp, relative) and propagated through what follows:

  exposure     x E: one rounding, u |x E|.  The sanitising clamp is exact and 1-Lipschitz.
  matrix       row i = fmaf(M_i2, c_b, fmaf(M_i1, c_g, M_i0 c_r)): three roundings of partial sums that are each at most
               S_i = sum_j |M_ij| |c_j|, and the host's double product rounded to float32 may land on the neighbouring float
               (another u S_i): 4 u S_i + sum_j |M_ij| err_j.
  CDL          t = fmaf(c, slope, offset): slope err_c + u |t|.  pow: the float64 power evaluated at both ends of [t - err_t, t + err_t]
               (the power is monotone; the lower end clamped at 0) plus POW_ULP = 2 ulp = 4 u of the result (HIP documents powf
               to 1 ulp, glibc's is below 1; one ulp of margin).  A channel whose power is 1 takes no powf: no such term.
  saturation   Y = three roundings of partial sums of at most W = 0.2126 |r| + 0.7152 |g| + 0.0722 |b|: 3 u W + sum_j w_j err_j;
               d = c - Y: err_c + err_Y + u |d|;  fmaf(sat, d, Y): sat err_d + err_Y + u |out|.
  tone map     the input error goes through M_in (non-negative), through the fitted curve by evaluating it at both ends (it is
               monotone on v >= 0) and through |M_out|; the stage's own float32 arithmetic adds TONE_U = 32 u: four roundings on
               the way to the curve's argument (relative; v f'(v) <= 0.37), the curve's numerator (three roundings of at most 1.05),
               denominator (four, relative) and quotient — about 10 u of a value of at most 1.02 — times |M_out|'s row sum 2.21, and
               three more roundings of that row.
  LUT          p = v (n - 1) is rounded (u (n - 1)) and carries (n - 1) err_v; the error of the fraction along axis a moves output channel k by
               at most D_ak, the largest difference of that channel between neighbours along that axis: (n - 1) sum_a D_ak (err_v_a + u); the three weight
               differences and the four-term fmaf chain are seven roundings of terms of at most Lmax: + 8 u Lmax.  The stage clamps
               the result to [0, 1] (a LUT may overshoot), which is exact and 1-Lipschitz.
  sRGB         the OETF's slope at the value (12.92 below the knee, else 1.055 / 2.4 (c - err)^(1 / 2.4 - 1)) times the error, + 16 u for
               its own powf and two more roundings.
  byte         255 v: without dither the kernel's rintf(v * 255.0f) rounds the product first, u 255 = 1.5e-5 of a byte step; with
               dither v 255 + d - 0.5 is decided exactly (dg_byte), so only v's own bound counts.
Where a bound decides a byte — 255 v (+ d - 0.5) within 255 times the bound of a half-integer — the byte may differ by one.  judge()
asserts BY THE MODEL ALONE that at most MAX_NEAR = 1 % of an image's colour channel values are such values, then holds the rest to the
exact byte.

FXAA (display.h) is judged in two steps, each against the model: the graded texels t of an image are what the stage returns with
display_fxaa = 0 as RGBA32F, held to graded_texels() within its bound; the FXAA result is held to display_model's fxaa() ON THOSE
float32 texels under display_model's own rule (TOL, the branch margin) — the situation that rule was made for.  A bound on FXAA's
output in terms of an error of its input does not exist in a useful form: the tap positions divide by a gradient."""
import numpy as np

import display_model as dm

U = 2.0 ** -24
POW_ULP = 2
TONE_U = 32 * U
MAX_NEAR = 0.01
LUMA709 = np.array([0.2126, 0.7152, 0.0722])

BRADFORD = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]])
RGB2XYZ = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]])


def white(T):
    T = float(T)
    if T <= 4000.0:
        x = -0.2661239e9 / T ** 3 - 0.2343589e6 / T ** 2 + 0.8776956e3 / T + 0.179910
    else:
        x = -3.0258469e9 / T ** 3 + 2.1070379e6 / T ** 2 + 0.2226347e3 / T + 0.240390
    if T <= 2222.0:
        y = -1.1063814 * x ** 3 - 1.34811020 * x ** 2 + 2.18555832 * x - 0.20219683
    elif T <= 4000.0:
        y = -0.9549476 * x ** 3 - 1.37418593 * x ** 2 + 2.09137015 * x - 0.16748867
    else:
        y = 3.0817580 * x ** 3 - 5.87338670 * x ** 2 + 3.75112997 * x - 0.37001483
    return np.array([x / y, 1.0, (1.0 - x - y) / y])


def wb_matrix(T):
    """M_wb of T kelvin as the host stores it: float64 arithmetic, float32 entries (returned as float64)."""
    scale = (BRADFORD @ white(6500.0)) / (BRADFORD @ white(T))
    M = np.linalg.inv(RGB2XYZ) @ np.linalg.inv(BRADFORD) @ np.diag(scale) @ BRADFORD @ RGB2XYZ
    return M.astype(np.float32).astype(np.float64)


class Grade:
    """The settings of one test case, with the float32 values the context holds."""

    def __init__(self, temperature=6500.0, slope=1.0, offset=0.0, power=1.0, saturation=1.0, lut=None, dither=0):
        self.temperature = float(np.float32(temperature))
        f3 = lambda v: np.broadcast_to(np.asarray(v, np.float32), (3,)).astype(np.float64)
        self.slope, self.offset, self.power = f3(slope), f3(offset), f3(power)
        self.saturation = float(np.float32(saturation))
        self.lut = None if lut is None else np.asarray(lut, np.float32)
        self.dither = int(dither)

    def settings(self):
        j = lambda v: " ".join("%.9g" % x for x in v)
        return {"display_wb_temperature": "%.9g" % self.temperature, "display_grade_slope": j(self.slope),
                "display_grade_offset": j(self.offset), "display_grade_power": j(self.power),
                "display_grade_saturation": "%.9g" % self.saturation, "display_dither": self.dither}

    def apply(self, c):
        for k, v in self.settings().items():
            c.set_setting(k, v)
        c.set_display_lut(self.lut)

    @property
    def wb_on(self):
        return self.temperature != 6500.0

    def cdl_on(self, i):
        return not (self.slope[i] == 1.0 and self.offset[i] == 0.0 and self.power[i] == 1.0)

    @property
    def linear_on(self):
        return self.wb_on or any(self.cdl_on(i) for i in range(3)) or self.saturation != 1.0


def linear(c, err, g):
    """The LINEAR block on colours c (... x 3, float64, with the bound err on what float32 holds): (value, bound)."""
    with np.errstate(invalid="ignore"):
        c = np.minimum(dm._fmax(c, 0.0), 65504.0)
    err = np.where(np.isfinite(err), err, 0.0)  # (a NaN or an infinity is sanitised exactly)
    if g.wb_on:
        M = wb_matrix(g.temperature)
        S = np.abs(c) @ np.abs(M).T
        c, err = c @ M.T, err @ np.abs(M).T + 4 * U * S
    c, err = c.copy(), err.copy()
    for i in range(3):
        if g.cdl_on(i):
            t = c[..., i] * g.slope[i] + g.offset[i]
            et = g.slope[i] * err[..., i] + U * np.abs(t)
            lo, hi = np.maximum(t - et, 0.0) ** g.power[i], np.maximum(t + et, 0.0) ** g.power[i]
            r = np.maximum(t, 0.0) ** g.power[i]
            pw = 0.0 if g.power[i] == 1.0 else POW_ULP * 2 * U * r  # (power 1: the clamped value itself, no powf)
            c[..., i], err[..., i] = r, np.maximum(hi - r, r - lo) + pw
    if g.saturation != 1.0:
        Y = c @ LUMA709
        eY = err @ LUMA709 + 3 * U * (np.abs(c) @ LUMA709)
        d = c - Y[..., None]
        ed = err + eY[..., None] + U * np.abs(d)
        out = Y[..., None] + g.saturation * d
        c, err = out, g.saturation * ed + eY[..., None] + U * np.abs(out)
    return c, err


def _curve(v):
    return (v * (v + 0.0245786) - 0.000090537) / (v * (0.983729 * v + 0.432951) + 0.238081)


def tone(c, err, brightness, contrast, tonemap):
    """display.h's tone step on float64 colours with an input bound: (v in [0, 1], bound)."""
    off = -0.5 * np.float64(np.float32(contrast)) + 0.5 + np.float64(np.float32(brightness))
    with np.errstate(invalid="ignore"):
        v = np.minimum(dm._fmax(c + off, 0.0), 65504.0)
    err = np.where(np.isfinite(err), err, 0.0)
    if tonemap == "none":
        return np.minimum(v, 1.0), err + TONE_U
    w, ew = v @ dm.M_IN.T, err @ dm.M_IN.T
    f = _curve(w)
    ef = np.maximum(np.abs(_curve(w + ew) - f), np.abs(f - _curve(np.maximum(w - ew, 0.0))))
    return np.clip(f @ dm.M_OUT.T, 0.0, 1.0), ef @ np.abs(dm.M_OUT).T + TONE_U


def lut_spread(lut):
    """(D, Lmax): D[a][k] = the largest difference of output channel k between neighbours along input axis a (0 = red), and the
    LUT's largest magnitude."""
    L = np.asarray(lut, np.float64)
    D = np.array([np.abs(np.diff(L, axis=2 - a)).reshape(-1, 3).max(0) for a in range(3)])
    return D, np.abs(L).max()


def tetra(lut, v):
    """tetra(L, v) in float64 for v (... x 3) in [0, 1]; lut is n x n x n x 3 indexed [b][g][r]."""
    L = np.asarray(lut, np.float64)
    n = L.shape[0]
    p = np.asarray(v, np.float64) * (n - 1)
    i = np.minimum(p.astype(np.int64), n - 2)
    f = p - i
    order = np.argsort(-f, axis=-1, kind="stable")  # descending, ties in channel order
    fs = np.take_along_axis(f, order, -1)
    idx = i.copy()

    def at(ix):
        return L[ix[..., 2], ix[..., 1], ix[..., 0]]
    V0 = at(idx)
    step = np.zeros_like(idx)
    np.put_along_axis(step, order[..., :1], 1, -1)
    V1 = at(idx + step)
    np.put_along_axis(step, order[..., 1:2], 1, -1)
    V2 = at(idx + step)
    V3 = at(idx + 1)
    w = np.stack([1.0 - fs[..., 0], fs[..., 0] - fs[..., 1], fs[..., 1] - fs[..., 2], fs[..., 2]], -1)
    return w[..., 0:1] * V0 + w[..., 1:2] * V1 + w[..., 2:3] * V2 + w[..., 3:4] * V3


def tetra_bound(lut, ev):
    D, Lmax = lut_spread(lut)
    n = np.asarray(lut).shape[0]
    return (n - 1) * ((ev + U) @ D) + 8 * U * Lmax


def graded_texels(rgba, g, E=None, brightness=0.05, contrast=1.0, tonemap="aces"):
    """What the LDS tile holds: (t H x W x 3 in float64, bound H x W x 3, alpha H x W)."""
    x = np.asarray(rgba, np.float32).astype(np.float64)
    c, a = x[..., :3], x[..., 3]
    err = np.zeros_like(c)
    with np.errstate(invalid="ignore", over="ignore"):
        if E is not None:
            c = c * np.float64(np.float32(E))
            err = U * np.abs(c)
        if g.linear_on:
            c, err = linear(c, err, g)
        t, et = tone(c, err, brightness, contrast, tonemap)
        a = np.minimum(dm._fmax(a, 0.0), 1.0)
    if g.lut is not None:
        t, et = np.clip(tetra(g.lut, t), 0.0, 1.0), tetra_bound(g.lut, et)  # (the stage clamps the LUT's result: 1-Lipschitz)
    return t, et, a


def srgb(c, err):
    knee = c - err < 0.0031308
    slope = np.where(knee, 12.92, 1.055 / 2.4 * np.maximum(c - err, 0.0031308) ** (1.0 / 2.4 - 1.0))
    return dm.srgb(c), slope * err + 16 * U


def bayer(w, h):
    """B(x, y) as an h x w array."""
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    q = xs ^ ys
    B = np.zeros_like(xs)
    for b in range(4):
        B |= (((q >> b) & 1) << (2 * (3 - b) + 1)) | (((ys >> b) & 1) << (2 * (3 - b)))
    return B


def byte_target(v, dither, w, h):
    """s with byte = rint(s), and the stage's own rounding of it in byte units."""
    if dither:
        return 255.0 * v + ((bayer(w, h) - 127.5) / 256.0)[..., None], 0.0
    return 255.0 * v, 255.0 * U


def judge_pointwise(got, rgba, g, E=None, brightness=0.05, contrast=1.0, tonemap="aces", srgb_on=False, label="", texels=None):
    """display_fxaa = 0: `got` (H x W x 4, float32 or uint8) against the model within the counted bound.  Returns the largest
    deviation as a fraction of the bound (float) or the share of byte values near a boundary (uint8)."""
    h, w = got.shape[:2]
    t, et, a = texels if texels is not None else graded_texels(rgba, g, E, brightness, contrast, tonemap)  # (texels: computed once)
    if srgb_on:
        t, et = srgb(t, et)
    if got.dtype == np.float32:
        d = np.abs(got[..., :3].astype(np.float64) - t)
        assert (d <= et).all(), "%s: float deviation %.3g of the bound at %s" % (label, (d / et).max(), np.unravel_index((d / et).argmax(), d.shape))
        assert np.abs(got[..., 3] - a).max() <= 1e-7, label
        return float((d / et).max())
    assert got.dtype == np.uint8
    s, own = byte_target(np.clip(t, 0.0, 1.0) if g.dither else t, g.dither, w, h)
    tol = 255.0 * et + own
    near = np.abs(s - np.floor(s) - 0.5) <= tol
    assert near.mean() <= MAX_NEAR, "%s: %.2f %% of the channel values lie within the bound of a byte boundary" % (label, 100 * near.mean())
    want = np.clip(np.rint(s), 0, 255)
    diff = np.abs(got[..., :3].astype(np.float64) - want)
    bad = ~((diff == 0) | (near & (diff <= 1)))
    assert not bad.any(), "%s: %d byte values differ; first at %s: got %s, want %s" % (
        label, int(bad.sum()), np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0][:2])], want[tuple(np.argwhere(bad)[0][:2])])
    assert np.array_equal(got[..., 3], np.rint(255.0 * np.float32(a).astype(np.float64)).astype(np.uint8)) or \
        np.abs(got[..., 3].astype(np.float64) - 255.0 * a).max() <= 0.5 + 1e-4, label + " alpha"
    return float(near.mean())


def judge_fxaa(got, texels, alpha, g, srgb_on=False, label=""):
    """display_fxaa = 1: `got` against display_model's FXAA of the float32 graded texels (H x W x 3, the stage's own RGBA32F output with
    display_fxaa = 0 and display_srgb = 0), under display_model's rule; a dithered byte image by the same rule on the dithered target."""
    t = np.asarray(texels, np.float32).astype(np.float64)
    h, w = t.shape[:2]
    A, B, take_a, margin = dm.fxaa(t)
    split = np.abs(A - B).max(-1)
    if srgb_on:
        A, B = dm.srgb(A), dm.srgb(B)
    tol = dm.TOL * (dm.SRGB_SLOPE if srgb_on else 1.0)
    take = take_a[..., None]
    out, other = np.where(take, A, B), np.where(take, B, A)
    if got.dtype == np.float32:
        d = got[..., :3].astype(np.float64)
        ok_out, ok_other = (np.abs(d - out) <= tol).all(-1), (np.abs(d - other) <= tol).all(-1)
        near_share = 0.0
    else:
        def ok(want):
            s, own = byte_target(np.clip(want, 0.0, 1.0) if g.dither else want, g.dither, w, h)
            near = np.abs(s - np.floor(s) - 0.5) <= 255.0 * tol + own
            diff = np.abs(got[..., :3].astype(np.float64) - np.clip(np.rint(s), 0, 255))
            return ((diff == 0) | (near & (diff <= 1))).all(-1), near
        ok_out, near = ok(out)
        ok_other, _ = ok(other)
        near_share = float(near.mean())
        assert near_share <= MAX_NEAR, "%s: %.2f %% of the channel values lie within the bound of a byte boundary" % (label, 100 * near_share)
    via_other = ~ok_out & ok_other & (margin <= dm.BAND)
    bad = ~(ok_out | via_other)
    assert not bad.any(), "%s: %d of %d pixels fail; first %s" % (label, int(bad.sum()), bad.size, np.argwhere(bad)[0])
    excused = int((via_other & (split > tol)).sum())
    assert excused <= dm.MAX_EXCUSED * bad.size, "%s: %d pixels excused" % (label, excused)
    return near_share


# ---- the inputs of the tests, all seeded -----------------------------------------------------------------------------------
SIZES = ((1, 1), (7, 5), (65, 17), (130, 35))


def image(w, h, seed=11):
    """Seeded HDR noise: gamma-distributed colours, a tenth of the pixels highlights of up to 1e4, then — where there is room — one
    NaN, one +inf and one negative channel."""
    rng = np.random.default_rng(seed + 977 * w + h)
    img = np.empty((h, w, 4), np.float32)
    img[..., :3] = rng.gamma(0.7, 0.6, (h, w, 3))
    hot = rng.uniform(size=(h, w)) < 0.1
    img[hot, :3] *= (10.0 ** rng.uniform(0.0, 4.0, int(hot.sum())))[:, None].astype(np.float32)
    np.minimum(img[..., :3], 1e4, out=img[..., :3])
    img[..., 3] = rng.uniform(-0.2, 1.2, (h, w))
    if w * h >= 4:
        flat = img.reshape(-1, 4)
        k = rng.choice(w * h, 3, replace=False)
        flat[k[0], 0], flat[k[1], 1], flat[k[2], 2] = np.nan, np.inf, -2.5
    return img


def look_lut(n):
    """A smooth look: a mild S-curve per channel and a little cross-talk (neighbours differ by about 1.3 / (n - 1))."""
    g = np.linspace(0.0, 1.0, n)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    s = lambda x: x * x * (3.0 - 2.0 * x)
    R, G, B = 0.6 * s(r) + 0.4 * r, 0.5 * s(gg) + 0.5 * gg, 0.7 * s(b) + 0.3 * b
    return np.stack([0.92 * R + 0.05 * G + 0.03 * B, 0.04 * R + 0.93 * G + 0.03 * B, 0.02 * R + 0.06 * G + 0.92 * B], -1).astype(np.float32)


def overshoot_lut(n):
    """A look with undershoot and overshoot, as grading tools export them: a contrast stretch about mid grey, entries in
    [-0.08, 1.08], and some cross-talk."""
    g = np.linspace(0.0, 1.0, n)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    s = lambda x: 0.5 + 1.16 * (x - 0.5)
    return np.stack([0.95 * s(r) + 0.05 * s(gg), 0.03 * s(r) + 0.97 * s(gg), 0.04 * s(gg) + 0.96 * s(b)], -1).astype(np.float32)


def random_lut(n, seed=5):
    return np.random.default_rng(seed + n).uniform(0.0, 1.0, (n, n, n, 3)).astype(np.float32)


CASES = {
    "wb_warm": dict(temperature=3200.0),
    "wb_cool": dict(temperature=9000.0),
    "slope": dict(slope=(1.2, 1.0, 0.8)),
    "offset": dict(offset=(0.02, -0.03, 0.0)),
    "power": dict(power=(0.9, 1.1, 1.0)),
    "saturation": dict(saturation=1.4),
    "lut": dict(lut="look17"),
    "dither": dict(dither=1),
    "all": dict(temperature=5200.0, slope=(1.1, 0.95, 1.05), offset=(0.01, 0.0, -0.02), power=(0.95, 1.0, 1.08), saturation=0.8, lut="look17", dither=1),
}


# what the stage tests run: every case unexposed, two of them under a manual exposure of 2^ev
VARIANTS = [(name, 0) for name in CASES] + [("all", 1), ("lut", -2)]


def near_share(img, g, E, srgb_on):
    """By the model alone: the share of an image's colour channel values whose byte the counted bound leaves open (FXAA off)."""
    h, w = img.shape[:2]
    t, et, _ = graded_texels(img, g, E)
    if srgb_on:
        t, et = srgb(t, et)
    s, own = byte_target(np.clip(t, 0.0, 1.0) if g.dither else t, g.dither, w, h)
    return float((np.abs(s - np.floor(s) - 0.5) <= 255.0 * et + own).mean())


_chosen = {}


def test_image(w, h):
    """The seeded image of a size: the first seed from 11 on under which every variant stays inside MAX_NEAR — chosen by the model,
    before any code under test runs (a 1 x 1 image has three channel values: none of them may sit on a boundary)."""
    if (w, h) not in _chosen:
        for seed in range(11, 75):
            img = image(w, h, seed)
            if all(near_share(img, case(name), None if ev == 0 else 2.0 ** ev, srgb_on) <= MAX_NEAR
                   for name, ev in VARIANTS for srgb_on in (False, True)):
                _chosen[(w, h)] = img
                break
        else:
            raise AssertionError("no seed keeps a %d x %d image inside the cap" % (w, h))
    return _chosen[(w, h)].copy()


def case(name):
    kw = dict(CASES[name])
    if kw.get("lut") == "look17":
        kw["lut"] = look_lut(17)
    return Grade(**kw)
