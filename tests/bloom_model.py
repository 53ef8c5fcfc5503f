"""A float64 numpy restatement of the display stage's bloom (csrc/bloom.h; include/rfwhip.h, rfwhip_bloom_image): sanitise, prefilter,
the Karis-weighted first down pass, the plain down passes, the up passes and the apply pass — and the bound by which a float32
implementation is judged against it.

THE BOUND.  u = 2^-24 is the unit roundoff of float32, M the largest sanitised input channel of the image, T = threshold, K = knee T,
E > 0 the exposure, R = T / E.  Every quantity below is non-negative and every stage is a convex combination, so nothing exceeds M
(0 <= g <= 1: s2 <= soft / 2 <= br / 2 because soft <= 2 K and br >= soft when K <= T; br - T <= br).  First-order terms are
counted; one further u M at the end pays for the products of two of them.
  p = c g      br = E max(c) (1 rounding), d = br - T (1): |err d| <= u br + u d.
               g = d / max(br, 1e-4) (d >= s2, so br >= T): |err g| <= u + 3 u g; with c <= 2 R where g < 1/2, and the rounding of
               the product: |err p| <= 6 u p + 2 u R.
               g = s2 / max(br, 1e-4) (br < T + K <= 2 T): soft = clamp(d + K, 0, 2 K) with K rounded once: |err soft| <= 8 u T;
               s2 = soft^2 / (4 K + 1e-4) (4 roundings, soft <= 2 K): |err s2| <= 8 u T + 4 u s2; |err g| <= 8 u T / max(br, 1e-4)
               + 6 u g, and c / max(br, 1e-4) <= 1 / E: |err p| <= 7 u p + 8 u R.
               max() is 1-Lipschitz: both cases obey |err p| <= 7 u p + 8 u R.
  k            Y = nz_luma(p) (3 roundings, coefficients adding up to 1): |err Y| <= 10 u Y + 8 u R; k = 1 / (1 + Y) (2 roundings),
               k Y < 1, k <= 1: relative error of k <= 12 u + 8 u R.
  k p          |err| <= (20 + 8 R) u (k p) + 8 u R k.
  D_1          16 taps, weights exact, one rounding per product and 15 additions of non-negative terms: each sum carries 16 u
               relative; the quotient one more: |err D_1| <= (65 + 16 R) u M + 8 u R.
  D_{k+1}      |err| <= err(D_k) + 16 u M.
  U_k          up(): 4 products, 3 additions: 4 u M; the difference, the product with scatter and the sum: 3 u M; the errors of D_k and
               U_{k+1} enter with the weights 1 - scatter and scatter: |err U_k| <= max(err D_k, err U_{k+1}) + 7 u M.
  With L levels: |err U_k| <= (65 + 16 R + 23 (L - 1) + 1) u M + 8 u R for every k  (bound_level)
  out          up(U_1) (4 u M), the product with intensity I and the sum:
               |err out| <= I (err U_1 + 5 u M) + (1 + I) u M                        (bound_out)
The model's own float64 roundings are 2^-29 of these.  Nothing here was chosen by looking at an implementation's error."""
import numpy as np

U32 = 2.0 ** -24
MAX_IN = 65504.0
EPS = float(np.float32(1e-4))  # the float32 literal of bloom.h
COEF = np.array([np.float32(0.2126), np.float32(0.7152), np.float32(0.0722)], np.float64)  # the float32 literals of nz_luma
H4 = np.array([1.0, 3.0, 3.0, 1.0]) / 8.0
MAX_LEVELS = 8

DEFAULTS = {"display_bloom": "0", "display_bloom_intensity": "0.2", "display_bloom_threshold": "1", "display_bloom_knee": "0.5",
            "display_bloom_scatter": "0.7", "display_bloom_levels": "6"}


def params(**kw):
    """The five parameters as the kernels see them (float32 values, held in float64); keys without the display_bloom_ prefix."""
    p = {k[len("display_bloom_"):]: v for k, v in DEFAULTS.items() if k != "display_bloom"}
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    out = {k: float(np.float32(float(p[k]))) for k in ("intensity", "threshold", "knee", "scatter")}
    out["levels"] = int(p["levels"])
    return out


def sanitise(rgba):
    """H x W x 3 float64: min(max(x, 0), 65504) with a NaN channel at 0."""
    x = np.asarray(rgba, np.float32).astype(np.float64)[..., :3]
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), 0.0, np.minimum(np.maximum(x, 0.0), MAX_IN))


def gain(c, E, P):
    T = P["threshold"]
    K = P["knee"] * T
    br = E * c.max(-1)
    soft = np.clip(br - T + K, 0.0, 2.0 * K)
    s2 = soft * soft / (4.0 * K + EPS)
    return np.maximum(s2, br - T) / np.maximum(br, EPS)


def prefilter(c, E, P):
    return c * gain(c, E, P)[..., None]


def half(n):
    return (n + 1) >> 1


def level_count(w, h, levels):
    k = 0
    while k < levels and (w > 1 or h > 1):
        w, h, k = half(w), half(h), k + 1
    return max(k, 1)


def _taps(img):
    """The 4 x 4 taps with h (x) h of every texel of the next level: H x W x C -> half(H) x half(W) x C."""
    H, W = img.shape[:2]
    i, j = np.arange(half(W)), np.arange(half(H))
    acc = np.zeros((half(H), half(W)) + img.shape[2:])
    for b in range(4):
        ys = np.clip(2 * j - 1 + b, 0, H - 1)
        for a in range(4):
            xs = np.clip(2 * i - 1 + a, 0, W - 1)
            acc += H4[b] * H4[a] * img[ys][:, xs]
    return acc


def down0(p):
    k = 1.0 / (1.0 + p @ COEF)
    return _taps(k[..., None] * p) / _taps(k[..., None])


def down(d):
    return _taps(d)


def up(u, w, h):
    """up(u) at the w x h texels of the finer level."""
    Hn, Wn = u.shape[:2]
    x, y = np.arange(w), np.arange(h)
    xa, ya = (x - 1) >> 1, (y - 1) >> 1
    x0, x1, y0, y1 = np.clip(xa, 0, Wn - 1), np.clip(xa + 1, 0, Wn - 1), np.clip(ya, 0, Hn - 1), np.clip(ya + 1, 0, Hn - 1)
    wx0, wy0 = np.where(x & 1, 0.75, 0.25)[None, :, None], np.where(y & 1, 0.75, 0.25)[:, None, None]
    top = wx0 * u[y0][:, x0] + (1.0 - wx0) * u[y0][:, x1]
    bottom = wx0 * u[y1][:, x0] + (1.0 - wx0) * u[y1][:, x1]
    return wy0 * top + (1.0 - wy0) * bottom


def chain(rgba, E=1.0, **kw):
    """{"levels": L, "U": {k: h_k x w_k x 3 for k = 1 .. L}, "D": likewise before the way up, "c": the sanitised input,
    "out": H x W x 3, "M": the largest sanitised channel, "params": the parameters, "E": E}."""
    P = params(**kw)
    E = float(np.float32(E))
    c = sanitise(rgba)
    h, w = c.shape[:2]
    L = level_count(w, h, P["levels"])
    D = {1: down0(prefilter(c, E, P))}
    for k in range(2, L + 1):
        D[k] = down(D[k - 1])
    U = {L: D[L]}
    for k in range(L - 1, 0, -1):
        U[k] = D[k] + P["scatter"] * (up(U[k + 1], D[k].shape[1], D[k].shape[0]) - D[k])
    out = c + P["intensity"] * up(U[1], w, h)
    return {"levels": L, "U": U, "D": D, "c": c, "out": out, "M": float(c.max()), "params": P, "E": E}


def bound_level(m):
    """|U_k - model| for every level of chain() result m."""
    R = m["params"]["threshold"] / m["E"]
    return (65.0 + 16.0 * R + 23.0 * (m["levels"] - 1) + 1.0) * U32 * m["M"] + 8.0 * U32 * R


def bound_out(m):
    I = m["params"]["intensity"]
    return I * (bound_level(m) + 5.0 * U32 * m["M"]) + (1.0 + I) * U32 * m["M"]


def judge(got_out, got_levels, m, rgba, label=""):
    """Assert that the output image (H x W x 4 float32) and the levels ({k: h x w x 4 float32}) are chain() result m within the
    bounds, and that alpha is the input's bit for bit.  Returns the largest error / bound ratio."""
    rgba = np.asarray(rgba, np.float32)
    assert got_out.dtype == np.float32 and got_out.shape == rgba.shape, label
    assert np.array_equal(got_out[..., 3].view(np.uint32), rgba[..., 3].view(np.uint32)), "%s: alpha is not the input's" % label
    assert np.isfinite(got_out[..., :3]).all(), "%s: the output is not finite" % label
    worst = 0.0
    bl, bo = bound_level(m), bound_out(m)
    assert sorted(got_levels) == list(range(1, m["levels"] + 1)), "%s: levels %s, model %d" % (label, sorted(got_levels), m["levels"])
    for k, g in got_levels.items():
        assert g.shape[:2] == m["U"][k].shape[:2], "%s: level %d is %s, model %s" % (label, k, g.shape, m["U"][k].shape)
        e = float(np.abs(g[..., :3].astype(np.float64) - m["U"][k]).max())
        assert e <= bl, "%s: U_%d off by %.3g, bound %.3g" % (label, k, e, bl)
        worst = max(worst, e / bl if bl > 0 else 0.0)
    e = float(np.abs(got_out[..., :3].astype(np.float64) - m["out"]).max())
    assert e <= bo, "%s: out off by %.3g, bound %.3g" % (label, e, bo)
    return max(worst, e / bo if bo > 0 else 0.0)


# ---- the model's own images ------------------------------------------------------------------------------------------------
def constant(w, h, rgb=(0.8, 0.35, 2.5)):
    img = np.empty((h, w, 4), np.float32)
    img[...] = tuple(rgb) + (0.6,)
    return img


def impulse(w, h, x, y, value=(40.0, 25.0, 10.0), floor=0.05):
    """One bright pixel on a dim grey; alpha varies."""
    img = np.full((h, w, 4), floor, np.float32)
    img[..., 3] = np.linspace(-0.5, 1.5, w * h, dtype=np.float32).reshape(h, w)
    img[y, x, :3] = value
    return img


def lognormal(w, h, seed=5, sigma_octaves=3.0):
    """HDR noise, log2 of every channel normal with sigma = 3 octaves around 2^-2."""
    rng = np.random.default_rng(seed + 977 * w + h)
    img = np.empty((h, w, 4), np.float32)
    img[..., :3] = 2.0 ** (sigma_octaves * rng.standard_normal((h, w, 3)) - 2.0)
    img[..., 3] = rng.uniform(-0.2, 1.2, (h, w))
    return img


def nonfinite(w, h, seed=9):
    """Noise with NaN, +inf, -inf and negative channels sprinkled in (alpha too: it is copied, never read)."""
    rng = np.random.default_rng(seed + 31 * w + h)
    img = lognormal(w, h, seed)
    n = max(1, (w * h) // 30)
    for value in (np.nan, np.inf, -np.inf, -3.5):
        ys, xs, cs = rng.integers(0, h, n), rng.integers(0, w, n), rng.integers(0, 4, n)
        img[ys, xs, cs] = value
    return img


def impulse_positions(w, h):
    """An even/even and an odd/odd interior position and the four corners (fewer on images too small to have them)."""
    pos = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    if w > 4 and h > 4:
        pos += [((w // 2) & ~1, (h // 2) & ~1), ((w // 2) | 1, (h // 2) | 1)]
    return sorted({(min(x, w - 1), min(y, h - 1)) for x, y in pos})


SIZES = ((1, 1), (2, 2), (3, 5), (63, 17), (130, 70))
# the defaults, and one deviation from them each
PARAM_SETS = ({}, {"threshold": 0}, {"knee": 0}, {"scatter": 0}, {"scatter": 1}, {"levels": 1}, {"levels": 2}, {"levels": 3}, {"levels": 8})
EXPOSURES = (0.25, 4.0)
