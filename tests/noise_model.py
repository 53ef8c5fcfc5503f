"""A float64 model of the noise estimate (csrc/noise.h), the bounds both builds are held to, and the
checks the CPU and the GPU tier share.  Not the product's algorithm restated: the variance is TWO-PASS over all samples (no
shift, no merge), the tile sums are numpy sums (no butterfly, no order).

Counted bounds, u = 2^-24 (float32 round to nearest), gamma(k) = k u / (1 - k u):

Y of a sample: three roundings (a product, two fmaf) of non-negative terms           |Y32 - Y| <= gamma(3) Y =: eY

sumY: a call adds its S values in order (S - 1 additions) and the sum to the old one (1 addition)
      E_sum' = E_sum + sum eY + gamma(S - 1) sum Y + u sumY'

M2, one call of S samples on top of n_a (moment_bounds below follows this line by line):
  K      the device's shift.  n_a > 0: K = fl(sumY32 / n_a), |K - mean_a| <= E_sum / n_a + u |K| =: eK.  n_a = 0: K = Y32 of sample 0.
  d_s    = fl(Y32_s - K); against d^_s = Y_s - K (real arithmetic, the device's K):    |d_s - d^_s| <= eY_s + u |d_s| =: ed_s
         with |d^_s| <= D_s = |Y_s - mean_a| + eK  (n_a = 0: |Y_s - Y_0| + eY_0)
  b      S fused multiply-adds:         eb = sum (2 D ed + ed^2) + gamma(S + 1) sum (D + ed)^2
  a      S - 1 additions:               ea = sum ed + gamma(S - 1) sum (D + ed)
  M2_b   = b - a^2 / S (a product, a division, a subtraction); in real arithmetic b^ - a^^2 / S IS the step's two-pass M2 whatever K:
                                        eM2b = eb + (2 A ea + ea^2) / S + gamma(2) (A + ea)^2 / S + u (M2_b + eb),   A >= |a^|
  T      = (a / S)^2 (n_a S / (n_a + S)): five roundings; and Chan's term wants mean_b - mean_a = a^ / S + (K - mean_a):
                                        eT = gamma(5) T + (2 A ea + ea^2) w / S^2 + (2 (A / S) eK + eK^2) w,   w = n_a S / (n_a + S)
  M2'    two additions:                 E_M2' = E_M2 + eM2b + eT + 2 u M2'
The eK term is the price of keeping the mean in float32: it is what limits a pixel of mean 100 and spread 1e-3 (eK grows to
1.5e-4 over 50 calls against the spread of 1e-3: the bound comes to 0.2 - 0.5 M2), where sum Y^2 - (sum Y)^2 / n has an error of
n 1e4 u ~ 6e-4 n against M2 = 1e-6 n.
The bounds are multiplied by 1 + 1e-3 for the products of two error terms left out above.

e of a pixel from GIVEN float32 moments: sumY / n, M2 / (n - 1), / n, sqrt, mean + floor, the division: six operations; the
square root halves what comes before it, and the device's sqrt and division are allowed one ulp (2 u) where u would do:
                                        |e32 - e| <= 8 u e =: E_REL e
A tile's sum_e: at most 255 additions of non-negative terms in any order, each term off by E_REL:   gamma(255) + E_REL, relative.
The totals are sums of the tile sums in double: nothing to add at this scale.
converged: a pixel may fall on the other side of the threshold only where |e - threshold| <= E_REL e (plus, for rendered moments,
what the moments' own bounds move e by); at most 1 % of an input's pixels may."""
import numpy as np

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
WR, WG, WB = (float(np.float32(w)) for w in (0.2126, 0.7152, 0.0722))
TILE_X, TILE_Y = 32, 8
E_REL = 8 * U
SLACK = 1.0 + 1e-3
SIZES = [(1, 1), (31, 7), (33, 9), (130, 70)]
FLOOR, THRESHOLD = 0.01, 0.05  # the settings' defaults


def gamma(k):
    return k * U / (1.0 - k * U)


def luma(c):
    c = np.asarray(c, np.float64)
    return WR * c[..., 0] + WG * c[..., 1] + WB * c[..., 2]


def two_pass(Y):
    """Y: P x n -> (sum, M2)."""
    Y = np.asarray(Y, np.float64)
    return Y.sum(1), ((Y - Y.mean(1, keepdims=True)) ** 2).sum(1)


def moment_bounds(steps, y_err=None):
    """steps: the calls' sample luminances, P x S_k float64 arrays in call order (Y >= 0 up to y_err); y_err: per call, what
    the given Y may be off by beyond the device's own roundings.  -> (sumY, M2, E_sum, E_M2) after the last call."""
    P = steps[0].shape[0]
    E_sum, E_m2, n_a = np.zeros(P), np.zeros(P), 0
    for k, Y in enumerate(steps):
        Y = np.asarray(Y, np.float64)
        S = Y.shape[1]
        eY = gamma(3) * np.abs(Y) + (0.0 if y_err is None else y_err[k])
        if n_a:
            prev = np.concatenate(steps[:k], 1)
            mean_a = prev.mean(1)
            eK = E_sum / n_a + U * (np.abs(mean_a) + E_sum / n_a)
            D = np.abs(Y - mean_a[:, None]) + eK[:, None]
            A = np.abs(Y.sum(1) - S * mean_a) + S * eK
        else:
            eK = np.zeros(P)
            D = np.abs(Y - Y[:, :1]) + eY[:, :1]
            A = np.abs((Y - Y[:, :1]).sum(1)) + S * eY[:, 0]
        ed = eY + U * (D + eY)
        eb = (2 * D * ed + ed ** 2).sum(1) + gamma(S + 1) * ((D + ed) ** 2).sum(1)
        ea = ed.sum(1) + gamma(max(S - 1, 1)) * (D + ed).sum(1)
        m2b = two_pass(Y)[1]
        eM2b = eb + (2 * A * ea + ea ** 2) / S + gamma(2) * (A + ea) ** 2 / S + U * (m2b + eb)
        eT = 0.0
        if n_a:
            w = n_a * S / (n_a + S)
            eT = gamma(5) * ((A + ea) / S) ** 2 * w + (2 * A * ea + ea ** 2) * w / S ** 2 + (2 * (A / S) * eK + eK ** 2) * w
        n_a += S
        sum_now, m2_now = two_pass(np.concatenate(steps[:k + 1], 1))
        E_m2 = (E_m2 + eM2b + eT) * (1 + 2 * U) + 2 * U * m2_now
        E_sum = (E_sum + eY.sum(1) + gamma(max(S - 1, 1)) * np.abs(Y).sum(1)) * (1 + U) + U * np.abs(sum_now)
    return sum_now, m2_now, E_sum * SLACK + 1e-37, E_m2 * SLACK + 1e-37


def error(sumY, m2, n, floor=FLOOR):
    """The per-pixel error in float64 from given moments (float32 values as they are)."""
    s, m = np.asarray(sumY, np.float64), np.asarray(m2, np.float64)
    fl = float(np.float32(floor))
    with np.errstate(all="ignore"):
        e = np.sqrt(m / (n - 1) / n) / (s / n + fl)
    bad = ~np.isfinite(s) | ~np.isfinite(m) | ~(e >= 0) | ~(e <= FLT_MAX)
    return np.where(bad, FLT_MAX, e)


def tiles(e, threshold=THRESHOLD):
    """e: H x W -> dict of tiles_y x tiles_x arrays: sum_e (at most FLT_MAX), max_e, pixels, converged."""
    h, w = e.shape
    ty, tx = -(-h // TILE_Y), -(-w // TILE_X)
    thr = float(np.float32(threshold))
    out = {k: np.zeros((ty, tx), np.float64 if k.endswith("_e") else np.int64) for k in ("sum_e", "max_e", "pixels", "converged")}
    for j in range(ty):
        for i in range(tx):
            t = e[j * TILE_Y:(j + 1) * TILE_Y, i * TILE_X:(i + 1) * TILE_X]
            out["sum_e"][j, i], out["max_e"][j, i] = min(t.sum(), FLT_MAX), t.max()
            out["pixels"][j, i], out["converged"][j, i] = t.size, int((t <= thr).sum())
    return out


def near_threshold(e, threshold, e_tol=None):
    """Pixels whose comparison with the threshold the bound does not decide."""
    thr = float(np.float32(threshold))
    tol = E_REL * e if e_tol is None else e_tol
    return np.abs(e - thr) <= tol


# ---- inputs of the metric: (n, sumY, M2) of a W x H image ---------------------------------------------------------
KINDS = ("zero", "uniform", "hot", "nonfinite", "straddle")


def metric_input(kind, w, h, n=16, floor=FLOOR, threshold=THRESHOLD):
    rng = np.random.default_rng(1234 + 7 * w + h)
    s, m = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    if kind == "uniform":
        s[:], m[:] = 0.5 * n, 0.02 * (n - 1)
    elif kind == "hot":  # one hot pixel at each corner of a tile and of the image, on a quiet ground
        s[:], m[:] = 0.5 * n, 1e-4 * (n - 1)
        for y in {0, min(TILE_Y - 1, h - 1), min(TILE_Y, h - 1), h - 1}:
            for x in {0, min(TILE_X - 1, w - 1), min(TILE_X, w - 1), w - 1}:
                m[y, x] = (50.0 + x + 3 * y) * (n - 1)
    elif kind == "nonfinite":
        s[:], m[:] = 0.5 * n, 0.02 * (n - 1)
        s[h // 2, w // 2] = np.nan
        m[h - 1, w - 1] = np.inf
        if w > TILE_X:
            m[0, TILE_X] = np.nan
    elif kind == "straddle":  # e from 0.5 to 1.5 thresholds, every pixel another value
        mean = rng.uniform(0.05, 2.0, (h, w))
        e = threshold * rng.uniform(0.5, 1.5, (h, w))
        s[:], m[:] = mean * n, (e * (mean + floor)) ** 2 * n * (n - 1)
    return n, s, m


def check_metric(c, kind, w, h, floor=FLOOR, threshold=THRESHOLD):
    """rfwhip_noise_image against the model: the map, every tile record, the stats, and two calls byte-equal."""
    n, s, m = metric_input(kind, w, h, floor=floor, threshold=threshold)
    c.set_setting("noise_floor", repr(floor))
    c.set_setting("noise_threshold", repr(threshold))
    st, e, t = c.noise_image(n, s, m)
    st2, e2, t2 = c.noise_image(n, s, m)
    assert st == st2 and e.tobytes() == e2.tobytes() and t.tobytes() == t2.tobytes(), "two calls differ"
    want = error(s, m, n, floor)
    big = want == FLT_MAX
    assert np.array_equal(e[big], np.full(int(big.sum()), FLT_MAX, np.float32))
    err = np.abs(e.astype(np.float64) - want)[~big]
    print("%s %dx%d: map max rel err %.3g u" % (kind, w, h, float((err / np.maximum(want[~big], 1e-300)).max() / U) if err.size else 0.0))
    assert (err <= E_REL * want[~big]).all()
    near = near_threshold(want, threshold)
    assert near.sum() <= 0.01 * w * h, "the input leaves more than 1 % of its pixels to the rounding"
    thr = float(np.float32(threshold))
    flipped = (e <= np.float32(threshold)) != (want <= thr)
    assert not (flipped & ~near).any() and flipped.sum() <= 0.01 * w * h
    wt = tiles(want, threshold)
    assert t.shape == wt["pixels"].shape
    assert np.array_equal(t["pixels"], wt["pixels"]) and int(t["pixels"].sum()) == w * h
    got_conv = tiles(e.astype(np.float64), threshold)["converged"]  # (the device's own map decides its own counts)
    assert np.array_equal(t["converged"], got_conv)
    assert np.abs(t["converged"].astype(np.int64) - wt["converged"]).sum() <= flipped.sum()
    tol_sum = (gamma(TILE_X * TILE_Y - 1) + E_REL) * SLACK
    assert (np.abs(t["sum_e"] - wt["sum_e"]) <= tol_sum * wt["sum_e"]).all()
    assert (np.abs(t["max_e"] - wt["max_e"]) <= E_REL * wt["max_e"]).all()
    assert st["samples"] == n and st["pixels"] == w * h and st["converged"] == int(t["converged"].sum())
    assert st["threshold"] == np.float32(threshold)
    want_mean = wt["sum_e"].sum() / (w * h)
    assert abs(st["mean_error"] - want_mean) <= tol_sum * want_mean
    assert st["max_error"] == t["max_e"].max() and abs(st["max_error"] - want.max()) <= E_REL * want.max()
    # the stats are the tile records folded in double
    assert abs(st["mean_error"] - t["sum_e"].astype(np.float64).sum() / (w * h)) <= 1e-12 * want_mean
    return st


# ---- the step update on given samples ----------------------------------------------------------------------------
def run_merges(c, steps_rgb):
    """steps_rgb: P x S_k x 3 float32 arrays; the calls one after the other through rfwhip_noise_merge -> (sumY, M2)."""
    P = steps_rgb[0].shape[0]
    s, m, n = np.zeros(P, np.float32), np.zeros(P, np.float32), 0
    for rgb in steps_rgb:
        s, m = c.noise_merge(n, s, m, rgb)
        n += rgb.shape[1]
    return s, m


def check_merges(c, steps_rgb, label):
    s, m = run_merges(c, steps_rgb)
    ws, wm, es, em = moment_bounds([luma(r) for r in steps_rgb])
    ds, dm_ = np.abs(s - ws), np.abs(m - wm)
    print("%s: sumY err / bound %.3g, M2 err / bound %.3g, M2 bound / M2 %.3g" %
          (label, float((ds / es).max()), float((dm_ / em).max()), float((em / np.maximum(wm, 1e-300)).max())))
    assert (ds <= es).all() and (dm_ <= em).all()
    return s, m, wm, em


def merge_cases(c):
    rng = np.random.default_rng(99)
    P = 300  # more than one workgroup
    # constant samples: M2 is exactly 0 — from nothing for every S, and on top of earlier samples wherever the running mean is
    # exact (1 + 1 + 2 samples: Y, 2 Y, 4 Y are exact sums)
    const = rng.uniform(0.0, 4.0, (P, 1, 3)).astype(np.float32)
    for S in (1, 3, 64):
        s, m = run_merges(c, [np.repeat(const, S, 1)])
        assert (m == 0).all() and np.isfinite(s).all(), S
    s, m = run_merges(c, [const, const, np.repeat(const, 2, 1)])
    assert (m == 0).all()
    check_merges(c, [np.repeat(const, 3, 1), np.repeat(const, 64, 1), const], "constant 3 + 64 + 1")
    # n_a = 0 and n_a > 0, S = 1, 3 and 64, in both orders
    for sizes in ((1,), (3,), (64,), (1, 1, 1, 3, 64), (64, 3, 1, 1)):
        steps = [rng.gamma(0.7, 1.0, (P, S, 3)).astype(np.float32) for S in sizes]
        check_merges(c, steps, "gamma " + "+".join(map(str, sizes)))
    # mean 100, spread 1e-3, 50 merged calls: the case sum Y^2 - (sum Y)^2 / n loses
    for S in (1, 3):
        steps = [(100.0 + 1e-3 * rng.standard_normal((P, S, 1))).repeat(3, 2).astype(np.float32) for _ in range(50)]
        s, m, wm, em = check_merges(c, steps, "mean 100 spread 1e-3, 50 x %d" % S)
        Y = np.concatenate([luma(r) for r in steps], 1)
        naive = np.abs((Y.astype(np.float32) ** 2).sum(1, dtype=np.float32) - Y.sum(1, dtype=np.float32) ** 2 / np.float32(Y.shape[1]) - wm)
        print("   sum Y^2 form in float32 would be off by %.3g M2 (median); the bound allows %.3g M2" %
              (float(np.median(naive / wm)), float(np.median(em / wm))))
        assert np.median(em / wm) < 1.0 < np.median(naive / wm)
    # a NaN sample: the moments are not finite from then on
    steps = [rng.gamma(0.7, 1.0, (P, 3, 3)).astype(np.float32) for _ in range(3)]
    steps[1][5, 1, 2] = np.nan
    steps[1][7, 0, 0] = np.inf
    s, m = run_merges(c, steps)
    assert not np.isfinite(s[5]) and not np.isfinite(m[5]) and not np.isfinite(s[7])
    ok = np.ones(P, bool)
    ok[[5, 7]] = False
    assert np.isfinite(s[ok]).all() and np.isfinite(m[ok]).all()
