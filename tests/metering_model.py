"""A float64 numpy restatement of the exposure meter (csrc/metering.h; include/rfwhip.h, rfwhip_get_meter): luminance, bin,
histogram, the windowed mean and the adapted exposure — and the rules by which a histogram and a record are judged against it.

HISTOGRAM.  The device computes Y = fmaf(0.0722, b, fmaf(0.7152, g, 0.2126 r)) in float32: three roundings of non-negative
terms, so |Y32 - Y| <= gamma(3) Y with gamma(n) = n u / (1 - n u), u = 2^-24 (the bound noise_model.py counts for the same
expression).  A pixel whose Y (1 - gamma3) and Y (1 + gamma3) fall into different bins is AMBIGUOUS between those two.  A histogram
passes when its total and `excluded` are exact, every bin lies between its certain count and certain + ambiguous, and the
ambiguous share of the image is at most MAX_AMBIGUOUS — a cap against hiding failures, not a measurement (the 0.01 of
display_model.MAX_EXCUSED).  Validity is taken from the float64 Y: the images here keep away from float32 underflow and overflow
of Y itself (their smallest positive channel is far above 1e-38, their largest finite one far below 1e38).

REDUCE.  Judged as a function of the histogram it was given.  Bounds, counted from the roundings (u = 2^-24, U = 2^-53):
  lambda   the device adds 256 terms w_b lambda_b with one double rounding each (fma) and 256 terms w_b likewise, divides, and
           rounds ONCE to float32: |err| <= ulp32(lambda) / 2 + 520 U max|lambda_b| (the second term covers both double sums, the
           quotient and this model's own double sum: 2 x 256 + a few roundings of values of magnitude <= 16).
  l_target (log2_key - lambda) + ev, two float32 roundings, then a clamp (which does not grow an error):
           |err| <= err(lambda) + u |log2_key - lambda| + u |l_target before the clamp|.
  l        first step: l_target.  Else fmaf(speed, l_target - l_prev, l_prev) with l_prev the DEVICE's previous l (an input,
           exact): one rounding of the difference d, one of the fma: |err| <= speed (err(l_target) + u |d|) + u |l|.
  E        exp2f(l).  The host's exp2f (glibc) documents < 1 ulp; the device's math library follows the OpenCL full-profile
           bound for exp2, <= 3 ulp.  An ulp is at most 2^-23 of the value, so |E - 2^l_device| <= EXP2_ULPS 2^-23 2^l_device
           for the device's own l, and against the model's l the error of l adds ln 2 err(l) relative.
Nothing here was chosen by looking at an implementation's error."""
import numpy as np

BINS = 256
U32, U64 = 2.0 ** -24, 2.0 ** -53
GAMMA3 = 3 * U32 / (1 - 3 * U32)
MAX_AMBIGUOUS = 0.01
EXP2_ULPS = 3.0
COEF = np.array([np.float32(0.2126), np.float32(0.7152), np.float32(0.0722)], np.float64)  # the float32 literals of nz_luma
T = np.array([np.float32(np.log2(1.0 + (s + 0.5) / 8.0)) for s in range(8)], np.float64)   # metering.h: MT_T
LAMBDA = np.array([(b >> 3) - 16 + T[b & 7] for b in range(BINS)], np.float64)

DEFAULTS = {"display_exposure": "manual", "display_exposure_ev": "0", "display_exposure_key": "0.18", "display_exposure_low": "0.1",
            "display_exposure_high": "0.9", "display_exposure_speed": "1", "display_exposure_min_ev": "-16",
            "display_exposure_max_ev": "16"}


def luminance(rgba):
    """H x W float64: Y of max(rgb, 0) with a NaN channel at 0."""
    x = np.asarray(rgba, np.float32).astype(np.float64)[..., :3]
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(x), 0.0, np.maximum(x, 0.0))
        return c @ COEF  # (inf * coefficient = inf; no NaN can arise: every term is >= 0)


def bin_of(Y):
    """The bin of positive finite float64 values: 8 per octave over [2^-16, 2^16), clamped."""
    m, ex = np.frexp(Y)  # Y = m 2^ex, m in [0.5, 1)
    k = 8 * (ex - 1 + 16) + np.floor((2.0 * m - 1.0) * 8.0).astype(np.int64)
    return np.clip(k, 0, BINS - 1)


def bin_of_float32(y):
    """The bin of ONE float32 value by the integer rule of metering.h, or -1 where it is not valid (RFWHIP_KAT_METER_BIN)."""
    y = np.float32(y)
    if not (y > 0 and np.isfinite(y)):
        return -1
    return int(np.clip((int(y.view(np.uint32)) >> 20) - ((127 - 16) << 3), 0, BINS - 1))


def histogram(rgba):
    """{"certain": 256 counts, "ambiguous": 256 counts (pixels that MAY be in the bin), "valid", "excluded", "n_ambiguous"}."""
    Y = luminance(rgba).ravel()
    valid = (Y > 0.0) & np.isfinite(Y)
    Yv = Y[valid]
    lo, hi = bin_of(Yv * (1.0 - GAMMA3)), bin_of(Yv * (1.0 + GAMMA3))
    amb = lo != hi
    certain = np.bincount(lo[~amb], minlength=BINS)
    ambiguous = np.bincount(lo[amb], minlength=BINS) + np.bincount(hi[amb], minlength=BINS)
    return {"certain": certain, "ambiguous": ambiguous, "valid": int(valid.sum()), "excluded": int((~valid).sum()),
            "n_ambiguous": int(amb.sum()), "pixels": int(Y.size)}


def judge_histogram(bins, excluded, model, label=""):
    bins = np.asarray(bins, np.int64)
    assert bins.shape == (BINS,), label
    assert int(bins.sum()) == model["valid"], "%s: %d pixels in the histogram, %d valid" % (label, int(bins.sum()), model["valid"])
    assert int(excluded) == model["excluded"], "%s: excluded %d, model %d" % (label, excluded, model["excluded"])
    low, high = model["certain"], model["certain"] + model["ambiguous"]
    bad = np.flatnonzero((bins < low) | (bins > high))
    assert bad.size == 0, "%s: bin %d holds %d, model [%d, %d]" % (label, bad[0], bins[bad[0]], low[bad[0]], high[bad[0]])
    assert model["n_ambiguous"] <= MAX_AMBIGUOUS * model["pixels"], "%s: %d of %d pixels ambiguous" % (
        label, model["n_ambiguous"], model["pixels"])
    return model["n_ambiguous"]


def _f32(v):
    return np.float64(np.float32(float(v)))


def reduce(bins, settings=None, prev=None):
    """The step on a histogram in float64.  settings: display_exposure_* values (strings or numbers; DEFAULTS where absent);
    prev: the record before the step (dict with "steps", "log2_exposure") or None for a fresh meter.  Returns None for no
    step, else {"lambda", "target", "target_unclamped", "first_term", "l", "d", "E", "speed", "first"}."""
    s = dict(DEFAULTS, **{k: str(v) for k, v in (settings or {}).items()})
    h = np.asarray(bins, np.float64)
    N = h.sum()
    C = np.concatenate([[0.0], np.cumsum(h)])
    lo, hi = _f32(s["display_exposure_low"]) * N, _f32(s["display_exposure_high"]) * N
    w = np.maximum(0.0, np.minimum(C[1:], hi) - np.maximum(C[:-1], lo))
    den = w.sum()
    if not den > 0.0:
        return None
    lam = float((w * LAMBDA).sum() / den)
    log2_key = _f32(np.log2(_f32(s["display_exposure_key"])))
    ev, lo_ev, hi_ev = _f32(s["display_exposure_ev"]), _f32(s["display_exposure_min_ev"]), _f32(s["display_exposure_max_ev"])
    speed = _f32(s["display_exposure_speed"])
    t1 = log2_key - lam
    t = t1 + ev
    target = min(max(t, lo_ev), hi_ev)
    first = prev is None or int(prev["steps"]) == 0
    lp = 0.0 if first else float(prev["log2_exposure"])
    d = target - lp
    l = target if first else lp + speed * d
    return {"lambda": lam, "target": target, "target_unclamped": t, "first_term": t1, "l": l, "d": 0.0 if first else d,
            "E": 2.0 ** l, "speed": speed, "first": first}


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v)))) if v != 0 else 2.0 ** -149


def bounds(m):
    """The error bounds of the docstring for a reduce() result: {"lambda", "target", "l", "E_rel"}."""
    e_lam = 0.5 * _ulp32(m["lambda"]) + 520 * U64 * 16.0
    e_t = e_lam + U32 * abs(m["first_term"]) + U32 * abs(m["target_unclamped"])
    e_l = e_t if m["first"] else m["speed"] * (e_t + U32 * abs(m["d"])) + U32 * abs(m["l"])
    return {"lambda": e_lam, "target": e_t, "l": e_l, "E_rel": EXP2_ULPS * 2.0 ** -23 + np.log(2.0) * e_l}


def judge_record(rec, bins, settings=None, prev=None, label=""):
    """Assert that the record `rec` (CoreBinding.meter() dict) is the step on `bins` from `prev`.  Returns the largest
    error / bound ratio observed (lambda, target, l, E against the model, E against the device's own l)."""
    m = reduce(bins, settings, prev)
    steps0 = 0 if prev is None else int(prev["steps"])
    if m is None:
        assert rec["steps"] == steps0, "%s: no valid pixel, yet a step was taken" % label
        if prev is not None:
            assert rec["exposure"] == prev["exposure"] and rec["log2_exposure"] == prev["log2_exposure"], label
        else:
            assert rec["exposure"] == 1.0, label
        return 0.0
    assert rec["steps"] == steps0 + 1, "%s: steps %d, expected %d" % (label, rec["steps"], steps0 + 1)
    b = bounds(m)
    ratios = {"lambda": abs(rec["log2_luminance"] - m["lambda"]) / b["lambda"],
              "target": abs(rec["log2_target"] - m["target"]) / b["target"],
              "l": abs(rec["log2_exposure"] - m["l"]) / b["l"],
              "E": abs(rec["exposure"] - m["E"]) / (b["E_rel"] * m["E"]),
              "E|l": abs(rec["exposure"] - 2.0 ** float(rec["log2_exposure"])) / (EXP2_ULPS * 2.0 ** -23 * 2.0 ** float(rec["log2_exposure"]))}
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0, "%s: %s is %.3g of its bound (record %s, model %s)" % (label, worst, ratios[worst], rec, m)
    return ratios[worst]


# ---- the model's own images ------------------------------------------------------------------------------------------------
def bin_centres(w, h, seed=3):
    """Greys at bin centres 2^e (1 + (s + 0.5) / 8), exactly representable: (image, the exact histogram).  A grey's Y lies
    within gamma3 of the grey (the three coefficients add up to 1 within 1e-7); a centre is 3 % from its bin's edges."""
    rng = np.random.default_rng(seed + 17 * w + h)
    b = rng.integers(0, BINS, (h, w))
    g = (2.0 ** ((b >> 3) - 16) * (1.0 + ((b & 7) + 0.5) / 8.0)).astype(np.float32)
    img = np.empty((h, w, 4), np.float32)
    img[..., :3] = g[..., None]
    img[..., 3] = rng.uniform(-1.0, 2.0, (h, w))
    return img, np.bincount(b.ravel(), minlength=BINS)


def constant(w, h, rgb=(0.8, 0.35, 2.5)):
    img = np.empty((h, w, 4), np.float32)
    img[...] = tuple(rgb) + (0.6,)
    return img


def all_excluded(w, h, seed=5):
    """Zeros, negatives, NaN, +inf and -inf mixed: no pixel is valid."""
    rng = np.random.default_rng(seed + 13 * w + h)
    kinds = np.array([[0.0, 0.0, 0.0], [-1.0, -0.0, -3.5], [np.nan, np.nan, np.nan], [np.nan, -2.0, 0.0], [np.inf, 0.5, 0.1],
                      [0.2, np.inf, np.nan], [-np.inf, -np.inf, 0.0], [np.inf, np.inf, np.inf]], np.float32)
    img = np.empty((h, w, 4), np.float32)
    img[..., :3] = kinds[rng.integers(0, len(kinds), (h, w))]
    img[..., 3] = 1.0
    return img


KINDS = ("noise", "stripes", "nonfinite")  # display_model.image kinds with no grey on a bin edge
# 130 x 70 = 9100 pixels is five workgroup ranges of 2048 (the last partial), 37 x 23 one ragged range, 1 x 1 and 5 x 3 less than a wave
SIZES = ((1, 1), (5, 3), (37, 23), (130, 70))
