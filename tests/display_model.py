"""A float64 numpy restatement of the display stage (csrc/display.h; include/rfwhip.h, rfwhip_read_display): tone map, FXAA,
encoding — and the rule by which an image is judged against it.

FXAA ends in a branch (A when luma(B) leaves [lumaMin, lumaMax], else B), so the model returns, per pixel, the chosen result,
both candidates and the branch margin min(|luma(B) - lumaMin|, |luma(B) - lumaMax|): a float32 implementation whose luma(B) lies
within rounding of a bound may take the other branch and is then held to the other candidate."""
import numpy as np

BAND = 1e-5        # margin below which a pixel may take the other branch
MAX_EXCUSED = 0.01  # a cap against hiding failures, not a measurement
TOL = 1e-5         # on the [0, 1] values before encoding (must stay <= 3.9e-5 = 0.01 of an 8-bit step)
SRGB_SLOPE = 12.92  # the OETF's largest slope: tolerance of encoded values

M_IN = np.array([[0.59719, 0.35458, 0.04823], [0.07600, 0.90834, 0.01566], [0.02840, 0.13383, 0.83777]])
M_OUT = np.array([[1.60475, -0.53108, -0.07367], [-0.10208, 1.10813, -0.00605], [-0.00327, -0.07276, 1.07602]])
LUMA = np.array([0.299, 0.587, 0.114])


def _fmax(a, b):
    """fmaxf: the other operand when one is NaN."""
    return np.where(np.isnan(a), b, np.maximum(a, b))


def tone(rgba, brightness, contrast, tonemap="aces"):
    """Step 1: H x W x 3 tone-mapped colour and H x W alpha, float64."""
    x = np.asarray(rgba, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = np.minimum(_fmax(x[..., :3] - 0.5 * np.float64(np.float32(contrast)) + 0.5 + np.float64(np.float32(brightness)), 0.0), 65504.0)
        a = np.minimum(_fmax(x[..., 3], 0.0), 1.0)
    if tonemap == "none":
        return np.minimum(v, 1.0), a
    v = v @ M_IN.T
    v = (v * (v + 0.0245786) - 0.000090537) / (v * (0.983729 * v + 0.432951) + 0.238081)
    return np.clip(v @ M_OUT.T, 0.0, 1.0), a


def _tap(t, qx, qy):
    h, w = t.shape[:2]
    ux, uy = qx - 0.5, qy - 0.5
    ix, iy = np.floor(ux), np.floor(uy)
    fx, fy = (ux - ix)[..., None], (uy - iy)[..., None]
    ix, iy = ix.astype(np.int64), iy.astype(np.int64)
    x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    return (1 - fy) * ((1 - fx) * t[y0, x0] + fx * t[y0, x1]) + fy * ((1 - fx) * t[y1, x0] + fx * t[y1, x1])


def fxaa(t):
    """Step 2 on the tone-mapped H x W x 3 image: (A, B, take_a, margin); the chosen result is A where take_a, else B."""
    h, w = t.shape[:2]
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    cx, cy = xs + 0.5, ys + 0.5
    nw, ne = _tap(t, cx - 0.75, cy - 0.75) @ LUMA, _tap(t, cx + 0.25, cy - 0.75) @ LUMA
    sw, se = _tap(t, cx - 0.75, cy + 0.25) @ LUMA, _tap(t, cx + 0.25, cy + 0.25) @ LUMA
    m = t @ LUMA
    lmin = np.minimum.reduce([m, nw, ne, sw, se])
    lmax = np.maximum.reduce([m, nw, ne, sw, se])
    dx, dy = -((nw + ne) - (sw + se)), (nw + sw) - (ne + se)
    reduce = np.maximum((nw + ne + sw + se) * (0.25 / 8.0), 1.0 / 64.0)
    rcp = 1.0 / (np.minimum(np.abs(dx), np.abs(dy)) + reduce)
    dx, dy = np.clip(dx * rcp, -8.0, 8.0), np.clip(dy * rcp, -8.0, 8.0)
    A = 0.5 * (_tap(t, cx - dx / 6.0, cy - dy / 6.0) + _tap(t, cx + dx / 6.0, cy + dy / 6.0))
    B = 0.5 * A + 0.25 * (_tap(t, cx - dx / 2.0, cy - dy / 2.0) + _tap(t, cx + dx / 2.0, cy + dy / 2.0))
    lb = B @ LUMA
    take_a = (lb < lmin) | (lb > lmax)
    margin = np.minimum(np.abs(lb - lmin), np.abs(lb - lmax))
    return A, B, take_a, margin


def srgb(c):
    return np.where(c < 0.0031308, 12.92 * c, 1.055 * np.power(np.maximum(c, 0.0), 1.0 / 2.4) - 0.055)


def display(rgba, brightness=0.05, contrast=1.0, tonemap="aces", fxaa_on=True, srgb_on=False):
    """The whole stage in float64, H x W x 4 each (colour encoded when srgb_on, alpha appended): {"out": the chosen result,
    "other": the candidate not chosen, "A", "B": both candidates (all four the tone-mapped texel without FXAA), "margin": H x W
    branch margin (inf without FXAA), "split": H x W max|A - B| before the encoding}."""
    t, a = tone(rgba, brightness, contrast, tonemap)
    if fxaa_on:
        A, B, take_a, margin = fxaa(t)
        split = np.abs(A - B).max(-1)
    else:
        A, B, take_a, margin, split = t, t, np.zeros(t.shape[:2], bool), np.full(t.shape[:2], np.inf), np.zeros(t.shape[:2])
    if srgb_on:
        A, B = srgb(A), srgb(B)
    A, B = np.concatenate([A, a[..., None]], -1), np.concatenate([B, a[..., None]], -1)
    take_a = take_a[..., None]
    return {"out": np.where(take_a, A, B), "other": np.where(take_a, B, A), "A": A, "B": B, "margin": margin, "split": split}


def _byte_ok(got, want, tol255):
    """A byte may differ from rint(255 want) by at most 1, and only where 255 want lies within tol255 of a half-integer."""
    s = 255.0 * want
    exact = got == np.rint(s)
    frac = s - np.floor(s)
    near = (np.abs(frac - 0.5) <= tol255) & (np.abs(got - np.rint(s)) <= 1)
    return exact | near


def judge(got, model, srgb_on=False, tol=TOL, label=""):
    """Assert that `got` (H x W x 4 float32, or uint8) passes the judging rule against display()'s result.  Returns the number
    of excused pixels (other branch taken within BAND of the branch, where the two candidates differ by more than tol)."""
    enc_tol = tol * (SRGB_SLOPE if srgb_on else 1.0)
    g = got.astype(np.float64)
    if got.dtype == np.uint8:
        ok_out = _byte_ok(g, model["out"], 255.0 * enc_tol).all(-1)
        ok_other = _byte_ok(g, model["other"], 255.0 * enc_tol).all(-1)
    else:
        assert got.dtype == np.float32
        ok_out = (np.abs(g - model["out"]) <= enc_tol).all(-1)
        ok_other = (np.abs(g - model["other"]) <= enc_tol).all(-1)
    via_other = ~ok_out & ok_other & (model["margin"] <= BAND)
    bad = ~(ok_out | via_other)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d pixels fail; first (%d, %d): got %s, model %s, other %s, margin %.3g" % (
            label, int(bad.sum()), bad.size, x, y, got[y, x], model["out"][y, x], model["other"][y, x], model["margin"][y, x]))
    excused = int((via_other & (model["split"] > tol)).sum())
    assert excused <= MAX_EXCUSED * bad.size, "%s: %d of %d pixels excused" % (label, excused, bad.size)
    return excused


# ---- the inputs of the tests, all seeded ---------------------------------------------------------------------------------
def image(kind, w, h, seed=7):
    rng = np.random.default_rng(seed + 131 * w + h)
    img = np.empty((h, w, 4), np.float32)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    if kind in ("noise", "nonfinite"):  # (a), (e): gamma-distributed HDR noise
        img[..., :3] = rng.gamma(0.5, 2.0, (h, w, 3))
    elif kind == "stripes":  # (b): diagonal stripes between 3.0 and 0.02, green halved, times 1 + 0.05 uniform per pixel
        s = np.where(np.mod(0.37 * xs + 0.93 * ys, 17.0) < 8.0, 3.0, 0.02)
        img[..., :3] = s[..., None] * np.array([1.0, 0.5, 1.0]) * (1.0 + 0.05 * rng.uniform(size=(h, w, 1)))
    elif kind == "lines":  # (c): flat 0.3 with one bright row and one black column
        img[..., :3] = 0.3
        img[h // 2, :, :3] = 4.0
        img[:, w // 3, :3] = 0.0
    elif kind == "ramp":  # (d): a horizontal ramp from 0 to 2
        img[..., :3] = (2.0 * xs / max(w - 1, 1))[..., None]
    else:
        raise ValueError(kind)
    img[..., 3] = rng.uniform(-0.2, 1.2, (h, w))
    if kind == "nonfinite":
        n = max(1, (w * h) // 40)
        for value in (np.nan, np.inf, -np.inf, -3.5):
            ys_, xs_, cs_ = rng.integers(0, h, n), rng.integers(0, w, n), rng.integers(0, 4, n)
            img[ys_, xs_, cs_] = value
    return img


KINDS = ("noise", "stripes", "lines", "ramp", "nonfinite")
SIZES = ((1, 1), (5, 3), (37, 23), (130, 70))
