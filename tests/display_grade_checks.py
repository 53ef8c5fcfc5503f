"""The known answers of the display stage's colour grading, as functions of a context: tests/test_display_grade.py runs them on the
host emulation, tests/test_display_grade_gpu.py on the HIP kernels — each held to the float64 model (display_grade_model.py), never
to the other."""
import itertools

import numpy as np

import display_grade_model as gm

DEFAULTS = {"display_grade": 0, "display_fxaa": 1, "display_srgb": 0, "display_tonemap": "aces", "display_exposure": "manual",
            "display_exposure_ev": 0, "display_exposure_speed": 1, "display_bloom": 0}


def reset(c):
    for k, v in DEFAULTS.items():
        c.set_setting(k, v)
    gm.Grade().apply(c)


def defaults_are_the_ungraded_bytes(c, w, h):
    """display_grade = 1 with every parameter at its default against display_grade = 0, bit for bit."""
    img = gm.image(w, h)
    assert np.isnan(img).any() and np.isinf(img).any() and (img[..., :3] < 0).any()
    reset(c)
    for fmt, fxaa, (mode, ev), bloom in itertools.product(("rgba8", "rgba32f"), (1, 0), (("manual", 0), ("manual", 1.3), ("auto", 0)), (0, 1)):
        for k, v in (("display_fxaa", fxaa), ("display_exposure", mode), ("display_exposure_ev", ev), ("display_bloom", bloom)):
            c.set_setting(k, v)
        out = []
        for grade in (0, 1):
            c.set_setting("display_grade", grade)
            c.meter_reset()
            out.append(c.display_image(img, 0.05, 1.0, fmt))
        word = np.uint32 if fmt == "rgba32f" else np.uint8
        assert np.array_equal(out[0].view(word), out[1].view(word)), (fmt, fxaa, mode, ev, bloom)
    reset(c)


def stage_matches_the_model(c, w, h, name, ev=0):
    """One case of display_grade_model.CASES on the seeded image of w x h: FXAA off against the counted bound, both formats, sRGB off
    and on; FXAA on (the two larger sizes) against display_model's FXAA of the stage's own graded texels."""
    img, g = gm.test_image(w, h), gm.case(name)
    reset(c)
    c.set_setting("display_grade", 1)
    c.set_setting("display_exposure_ev", ev)
    g.apply(c)
    E = None if ev == 0 else c_exposure(ev)
    label = "%s %dx%d ev=%g" % (name, w, h, ev)
    c.set_setting("display_fxaa", 0)
    texels = None
    for srgb in (0, 1):
        c.set_setting("display_srgb", srgb)
        f = c.display_image(img, 0.05, 1.0, "rgba32f")
        share = gm.judge_pointwise(f, img, g, E, srgb_on=bool(srgb), label=label + " srgb=%d rgba32f" % srgb)
        near = gm.judge_pointwise(c.display_image(img, 0.05, 1.0, "rgba8"), img, g, E, srgb_on=bool(srgb), label=label + " srgb=%d rgba8" % srgb)
        print("%s srgb=%d: largest float deviation %.3f of the bound, %.3f %% of the bytes near a boundary" % (label, srgb, share, 100 * near))
        if not srgb:
            texels = f
    if w >= 65:
        c.set_setting("display_fxaa", 1)
        c.set_setting("display_srgb", 0)
        a = np.minimum(np.maximum(np.nan_to_num(img[..., 3], nan=0.0), 0.0), 1.0)
        gm.judge_fxaa(c.display_image(img, 0.05, 1.0, "rgba32f"), texels[..., :3], a, g, label=label + " fxaa rgba32f")
        gm.judge_fxaa(c.display_image(img, 0.05, 1.0, "rgba8"), texels[..., :3], a, g, label=label + " fxaa rgba8")
    reset(c)


def c_exposure(ev):
    """E of display_exposure_ev = ev in manual mode: exp2f on the host; the tests use whole ev, where it is exact."""
    assert float(ev) == int(ev)
    return float(np.float32(2.0 ** ev))


def linear_known_answers(c):
    """rfwhip_grade_colors(0): the grey axis under the white balance, saturation 0, a negative offset."""
    reset(c)
    grey = np.repeat(np.float32([0.0, 1e-3, 0.18, 1.0, 7.5, 1e4])[:, None], 3, 1)
    for T in (1667, 2222, 4000, 6500, 25000):
        g = gm.Grade(temperature=T)
        g.apply(c)
        out = c.grade_colors(0, grey).astype(np.float64)
        want, err = gm.linear(grey.astype(np.float64), np.zeros((len(grey), 3)), g)
        assert (np.abs(out - want) <= err).all(), T
        if T == 6500:
            assert np.array_equal(out, grey)  # the identity: skipped, grey stays grey bit for bit
        else:
            # the axis stays a straight line through black: g M (1, 1, 1), the adapted white
            M = gm.wb_matrix(T)
            assert (np.abs(out - grey.astype(np.float64) * M.sum(1)) <= err).all(), T
            assert (M.sum(1)[0] < M.sum(1)[2]) == (T < 6500)  # a warmer light: towards blue
    rng = np.random.default_rng(3)
    cols = rng.gamma(0.7, 0.8, (257, 3)).astype(np.float32)
    g = gm.Grade(saturation=0.0)
    g.apply(c)
    out = c.grade_colors(0, cols).astype(np.float64)
    want, err = gm.linear(cols.astype(np.float64), np.zeros(cols.shape), g)
    assert (np.abs(out - want) <= err).all()
    assert (np.abs(out - (cols.astype(np.float64) @ gm.LUMA709)[:, None]) <= err).all()
    assert (out[:, 0] == out[:, 1]).all() and (out[:, 1] == out[:, 2]).all()  # Y in all three channels
    g = gm.Grade(offset=(-0.5, -0.5, 0.0), power=(0.5, 2.0, 1.0))
    g.apply(c)
    low = np.float32([[0.25, 0.4, 0.3], [0.5, 0.5, 0.5], [0.0, 0.1, 0.0]])
    out = c.grade_colors(0, low)
    assert (out[:, :2] == 0.0).all() and np.array_equal(out[:, 2], low[:, 2])  # clamped at 0 in front of the pow, never a NaN
    cols[3] = (np.nan, np.inf, -1.0)
    g = gm.Grade(temperature=3000, slope=(1.3, 1.0, 0.7), offset=(0.01, -0.02, 0.0), power=(0.8, 1.2, 1.0), saturation=1.5)
    g.apply(c)
    out = c.grade_colors(0, cols).astype(np.float64)
    want, err = gm.linear(cols.astype(np.float64), np.zeros(cols.shape), g)
    assert (np.abs(out - want) <= err).all()
    print("linear: largest deviation %.3f of the bound" % float((np.abs(out - want) / np.maximum(err, 1e-300)).max()))
    reset(c)


def lut_known_answers(c, n):
    """rfwhip_grade_colors(1) with LUTs of size n: lattice colours, the orderings and ties of the fractions, a random LUT, an identity."""
    reset(c)
    L = gm.random_lut(n)
    c.set_display_lut(L)
    assert int(c.get_setting("display_lut")) == n
    k = np.arange(n, dtype=np.float64) / (n - 1)
    b, g, r = np.meshgrid(k, k, k, indexing="ij")
    lattice = np.stack([r, g, b], -1).reshape(-1, 3).astype(np.float32)  # (1.0 and 0 are among them)
    assert np.array_equal(c.grade_colors(1, lattice).view(np.uint32), L.reshape(-1, 3).view(np.uint32))
    # the six orderings, the three pair ties and the triple tie of the fractions, in the first and the last cell
    fr = [p for p in itertools.permutations((0.25, 0.5, 0.75))] + [(0.5, 0.5, 0.25), (0.25, 0.5, 0.5), (0.5, 0.25, 0.5), (0.75, 0.25, 0.75), (0.5, 0.5, 0.5)]
    cols = np.float32([[(cell + f) / (n - 1) for f in p] for p in fr for cell in (0, n - 2)])
    rng = np.random.default_rng(n)
    cols = np.concatenate([cols, rng.uniform(0.0, 1.0, (500, 3)).astype(np.float32), np.float32([[1.0, 0.0, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])])
    out = c.grade_colors(1, cols).astype(np.float64)
    want = gm.tetra(L, cols.astype(np.float64))
    err = gm.tetra_bound(L, np.zeros(cols.shape))
    assert (np.abs(out - want) <= err).all(), (n, float((np.abs(out - want) / err).max()))
    I = np.stack([r, g, b], -1).astype(np.float32)
    c.set_display_lut(I)
    out = c.grade_colors(1, cols).astype(np.float64)
    assert (np.abs(out - cols) <= gm.tetra_bound(I, np.zeros(cols.shape))).all(), n
    c.set_display_lut(None)
    assert np.array_equal(c.grade_colors(1, cols), cols)
    reset(c)


def lut_outside_the_unit_cube(c, w, h):
    """A LUT with entries below 0 and above 1: the stage clamps what the LUT step hands on, so every byte is a byte of its own channel
    (no carry into a neighbour, no 255 from a negative value) — RGBA8 with dither off and on, sRGB off and on, FXAA off and on."""
    L = gm.overshoot_lut(9)
    assert L.min() < -0.05 and L.max() > 1.05
    g0, g1 = gm.Grade(lut=L), gm.Grade(lut=L, dither=1)
    # a ramp through black, mid grey and far above white in every channel, alpha 0.25: the LUT's corners are reached
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    img = np.empty((h, w, 4), np.float32)
    img[..., 0], img[..., 1], img[..., 2], img[..., 3] = 4.0 * xs / max(w - 1, 1), 4.0 * ys / max(h - 1, 1), 4.0 * (w - 1 - xs) / max(w - 1, 1), 0.25
    reset(c)
    c.set_setting("display_grade", 1)
    c.set_setting("display_tonemap", "none")
    t, _, _ = gm.graded_texels(img, g0, None, 0.0, 1.0, "none")
    raw = gm.tetra(L, np.minimum(img[..., :3].astype(np.float64), 1.0))
    assert (raw < -0.01).any() and (raw > 1.01).any() and t.min() == 0.0 and t.max() == 1.0  # the clamp has work to do
    for g in (g0, g1):
        g.apply(c)
        for srgb, fxaa in ((0, 0), (1, 0), (0, 1), (1, 1)):
            c.set_setting("display_srgb", srgb)
            c.set_setting("display_fxaa", fxaa)
            u8 = c.display_image(img, 0.0, 1.0, "rgba8")
            f32 = c.display_image(img, 0.0, 1.0, "rgba32f")
            assert (u8[..., 3] == 64).all(), (g.dither, srgb, fxaa)  # rint(0.25 x 255): nothing spilled into alpha
            assert f32[..., :3].min() >= 0.0 and f32[..., :3].max() <= 1.0 + 1e-6, (g.dither, srgb, fxaa)
            if not fxaa:
                gm.judge_pointwise(f32, img, g, None, 0.0, 1.0, "none", bool(srgb), "overshoot rgba32f")
                gm.judge_pointwise(u8, img, g, None, 0.0, 1.0, "none", bool(srgb), "overshoot rgba8 dither=%d srgb=%d" % (g.dither, srgb))
                over, under = (raw > 1.0 + 1e-4).all(-1), (raw < -1e-4).all(-1)
                assert over.any() and (u8[over][:, :3] == 255).all() and ((u8[under][:, :3] == 0).all() if under.any() else True)
            elif not srgb:
                c.set_setting("display_fxaa", 0)
                texels = c.display_image(img, 0.0, 1.0, "rgba32f")
                gm.judge_fxaa(f32, texels[..., :3], None, g, label="overshoot fxaa rgba32f")
                if not g.dither:  # (dithered, the saturated texels of this ramp sit 1 / 512 from a threshold for 2 of the 256 Bayer
                    # values, inside display_model's FXAA tolerance: the byte comparison of that case is the pointwise one above)
                    gm.judge_fxaa(u8, texels[..., :3], None, g, label="overshoot fxaa rgba8")
    reset(c)


def white_balance_maps_white_to_white(c):
    """An answer that does not come from the model's matrix: the white of T on the Planckian locus, as linear Rec.709, goes to the
    white of 6500 K.  Only temperatures whose white lies inside the Rec.709 gamut can be fed in (the block clamps negative channels)."""
    reset(c)
    to_rgb = np.linalg.inv(gm.RGB2XYZ)
    target = to_rgb @ gm.white(6500.0)
    tested = 0
    for T in (2222, 3000, 4000, 5000, 8000, 12000, 25000):
        src = to_rgb @ gm.white(T)
        if src.min() < 0.0:
            continue
        gm.Grade(temperature=T).apply(c)
        src32 = src.astype(np.float32)
        out = c.grade_colors(0, src32[None])[0].astype(np.float64)
        # the input's rounding to float32 (u per channel through |M|) and the row's arithmetic, as counted in the model; the host's
        # entries are float32 roundings of the double product
        M = np.abs(gm.wb_matrix(T))
        bound = 6 * gm.U * (M @ np.abs(src))
        assert (np.abs(out - target) <= bound).all(), (T, out, target, bound)
        tested += 1
    assert tested >= 4
    reset(c)


def dither_known_answers(c):
    """Constant images on a 48 x 32 target: the mean byte of every aligned 16 x 16 block, equal reads, RGBA32F and alpha untouched.

    rint(255 c + (B - 127.5) / 256) over the 256 values of B: with 255 c = m + phi, 0 <= phi < 1, the byte is m + 1 for the B with
    B > 255.5 - 256 phi and m for the others, so K = floor(256 phi + 0.5) of the 256 bytes are m + 1 (a B exactly on the threshold goes
    either way) and the mean is m + K / 256: within 1 / 512 of m + phi = 255 c."""
    reset(c)
    c.set_setting("display_grade", 1)
    c.set_setting("display_fxaa", 0)
    c.set_setting("display_tonemap", "none")
    w, h = c.width, c.height
    assert w % 16 == 0 and h % 16 == 0
    img = np.empty((h, w, 4), np.float32)
    for k, j in ((0, 0), (0, 1), (0, 5), (17, 3), (100, 7), (127, 5), (128, 9), (200, 1), (254, 9), (254, 10), (255, 0)):
        value = np.float32(k / 255.0 + j / 2560.0)
        img[...] = (value, value, value, 0.37)
        # brightness 0, contrast 1: the tone step adds nothing; display_tonemap = none: v = min(c, 1)
        c.set_setting("display_dither", 0)
        plain8, plain32 = c.display_image(img, 0.0, 1.0, "rgba8"), c.display_image(img, 0.0, 1.0, "rgba32f")
        c.set_setting("display_dither", 1)
        d8, d32 = c.display_image(img, 0.0, 1.0, "rgba8"), c.display_image(img, 0.0, 1.0, "rgba32f")
        assert np.array_equal(d8, c.display_image(img, 0.0, 1.0, "rgba8"))
        assert np.array_equal(d32.view(np.uint32), plain32.view(np.uint32))
        assert np.array_equal(d8[..., 3], plain8[..., 3]) and (d8[..., 3] == d8[0, 0, 3]).all()
        target = 255.0 * min(float(value), 1.0)
        blocks = d8[..., :3].astype(np.float64).reshape(h // 16, 16, w // 16, 16, 3).mean((1, 3))
        print("dither k=%d j=%d: block means within %.6f of 255 c (1 / 512 = %.6f)" % (k, j, np.abs(blocks - target).max(), 1 / 512))
        assert np.abs(blocks - target).max() <= 1.0 / 512.0, (k, j)
        assert (d8[..., 0] == d8[..., 1]).all() and (d8[..., 1] == d8[..., 2]).all()  # one pattern for the three channels
    assert np.array_equal(gm.bayer(2, 2) >> 6, [[0, 2], [3, 1]])
    reset(c)
