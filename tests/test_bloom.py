"""Bloom in front of the tone map (include/rfwhip.h, rfwhip_bloom_image; csrc/bloom.h), CPU tier: the host-emulation build runs the
same work items as the HIP kernels.  Held to the float64 model of tests/bloom_model.py within the bound counted there
(bound_level, bound_out: relative to the largest sanitised input of the image), to known answers that need no model, to the settings
contract, and to the single context for groups."""
import ctypes

import numpy as np
import pytest

import bloom_model as bm
import display_model as dm

KEYS = ("intensity", "threshold", "knee", "scatter", "levels")


def _set(c, **kw):
    """The display_bloom_* settings at their defaults, then `kw` (keys without the prefix)."""
    for k in KEYS:
        c.set_setting("display_bloom_" + k, bm.DEFAULTS["display_bloom_" + k])
    for k, v in kw.items():
        c.set_setting("display_bloom_" + k, v)


def _levels(c, n):
    return {k: c.read_bloom_level(k) for k in range(1, n + 1)}


def inputs(w, h):
    out = [("constant", bm.constant(w, h))]
    out += [("impulse at (%d, %d)" % p, bm.impulse(w, h, *p)) for p in bm.impulse_positions(w, h)]
    out += [("lognormal", bm.lognormal(w, h)), ("nonfinite", bm.nonfinite(w, h))]
    return out


def check_against_model(c, images, label=""):
    """Every image under every parameter set at E = 1 and under the defaults at E = 0.25 and 4: the output and every level within
    the counted bound.  Returns the largest error / bound ratio."""
    worst = 0.0
    for name, img in images:
        for kw, E in [(kw, 1.0) for kw in bm.PARAM_SETS] + [({}, E) for E in bm.EXPOSURES]:
            _set(c, **kw)
            out = c.bloom_image(img, E)
            m = bm.chain(img, E, **kw)
            worst = max(worst, bm.judge(out, _levels(c, m["levels"]), m, img, "%s %s %s E=%g" % (label, name, kw, E)))
    return worst


@pytest.mark.parametrize("size", bm.SIZES, ids=lambda s: "%dx%d" % s)
def test_chain_matches_the_model(make_emu, size):
    w, h = size
    c = make_emu()
    c.init(w, h)
    print("%dx%d: largest error / bound %.3g" % (w, h, check_against_model(c, inputs(w, h), "%dx%d" % (w, h))))


def _render(pkg, c, w=96, h=64, spp=4):
    scene = pkg.scenes.cornell(w, h, geometric_emitter=True)
    scene.camera.brightness, scene.camera.contrast = 0.1, 0.9
    c.init(w, h)
    scene.upload(c)
    c.set_setting("integrator", "pt")
    c.set_setting("spp", spp)
    c.render_frame(scene.camera, pkg.RESET)
    return scene


def test_rendered_frame_matches_the_model(pkg, make_emu):
    c = make_emu()
    _render(pkg, c)
    fb = c.framebuffer()
    assert fb[..., :3].max() > 2.0  # (the emitter is far above display white: there is something to bloom)
    print("cornell: largest error / bound %.3g" % check_against_model(c, [("cornell", fb)], "96x64"))


def check_known_answers(c, w, h):
    # a constant image above the 1e-4 floor with threshold 0: g = 1, every level is the constant, out = c (1 + intensity)
    img = bm.constant(w, h)
    _set(c, threshold=0)
    out = c.bloom_image(img, 1.0)
    col = img[0, 0, :3].astype(np.float64)
    L = bm.level_count(w, h, 6)
    m = {"params": bm.params(threshold=0), "E": 1.0, "levels": L, "M": float(col.max())}
    for k in range(1, L + 1):
        lv = c.read_bloom_level(k)
        assert np.abs(lv[..., :3] - col).max() <= bm.bound_level(m), k
    assert np.abs(out[..., :3] - col * (1.0 + bm.params()["intensity"])).max() <= bm.bound_out(m)
    # levels = 1, scatter = 0: U_1 = D_1 of an interior impulse on black at (2 a, 2 b) is the 2 x 2 footprint of h (x) h with the
    # Karis weight k of the impulse: texel (a - 1 + s, b - 1 + t) holds w k p / (1 - w + w k), w = h[3 - 2 s] h[3 - 2 t]
    _set(c, threshold=0, levels=1, scatter=0)
    x, y = (w // 2) & ~1, (h // 2) & ~1
    p = np.array([40.0, 25.0, 10.0])
    img = bm.impulse(w, h, x, y, tuple(p), floor=0.0)
    c.bloom_image(img, 1.0)
    lv = c.read_bloom_level(1)[..., :3].astype(np.float64)
    k = 1.0 / (1.0 + p @ bm.COEF)
    want = np.zeros_like(lv)
    for t in (0, 1):
        for s in (0, 1):
            wgt = bm.H4[3 - 2 * t] * bm.H4[3 - 2 * s]
            want[y // 2 - 1 + t, x // 2 - 1 + s] = wgt * k * p / (1.0 - wgt + wgt * k)
    m = {"params": bm.params(threshold=0, levels=1, scatter=0), "E": 1.0, "levels": 1, "M": 40.0}
    assert np.abs(lv - want).max() <= bm.bound_level(m)
    assert np.count_nonzero(lv.max(-1)) == 4  # exactly the footprint: every other texel is 0


def test_known_answers_without_the_model(make_emu):
    c = make_emu()
    c.init(63, 17)
    check_known_answers(c, 63, 17)


def check_invariants(c, w, h):
    img = bm.nonfinite(w, h)
    _set(c)
    a = c.bloom_image(img, 1.0)
    b = c.bloom_image(img, 1.0)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))  # two runs, identical bits
    assert np.array_equal(a[..., 3].view(np.uint32), img[..., 3].view(np.uint32))  # alpha bit for bit (NaN and inf among them)
    assert not np.isfinite(img[..., :3]).all() and np.isfinite(a[..., :3]).all()
    _set(c, intensity=0)
    z = c.bloom_image(img, 1.0)
    assert np.array_equal(z[..., :3], bm.sanitise(img).astype(np.float32))  # by value: c + 0 * glow
    assert np.array_equal(z[..., 3].view(np.uint32), img[..., 3].view(np.uint32))


def test_invariants(make_emu):
    c = make_emu()
    c.init(63, 17)
    check_invariants(c, 63, 17)


def test_off_means_off(pkg, make_emu):
    c, d = make_emu(), make_emu()
    for x in (c, d):
        _render(pkg, x, 48, 32, 1)
        x.set_setting("stage_timing", 1)
    d.set_setting("display_bloom", 1)
    _set(d, intensity=3, threshold=0.25, knee=1, scatter=0.2, levels=2)
    d.set_setting("display_bloom", 0)
    for fmt in ("rgba8", "rgba32f"):
        assert np.array_equal(c.display(fmt), d.display(fmt))
    img = dm.image("noise", 48, 32)
    assert np.array_equal(c.display_image(img, 0.05, 1.0, "rgba8"), d.display_image(img, 0.05, 1.0, "rgba8"))
    assert c.get_kernel_time("bloom")[1] == 0 and d.get_kernel_time("bloom")[1] == 0
    # ... and on is on: the same read now differs and counts 2 launches per level of the chain
    d.set_setting("display_bloom", 1)
    assert not np.array_equal(c.display("rgba8"), d.display("rgba8"))
    assert d.get_kernel_time("bloom")[1] == 2 * 2


def tone_slope():
    """An upper bound of |d tone / d x| in the infinity norm: 1 without a tone map; with ACES the two matrices' norms times the
    largest slope of the fitted rational on [0, 65504], taken from its derivative on a dense grid (+ 1 %)."""
    v = np.concatenate([[0.0], np.logspace(-7, np.log10(65504.0), 400001)])
    a, b = v * (v + 0.0245786) - 0.000090537, v * (0.983729 * v + 0.432951) + 0.238081
    da, db = 2.0 * v + 0.0245786, 2.0 * 0.983729 * v + 0.432951
    return 1.01 * np.abs(dm.M_OUT).sum(1).max() * np.abs((da * b - a * db) / (b * b)).max() * np.abs(dm.M_IN).sum(1).max()


def judge_display(fb, E, b, k, got8, got32, label):
    """read_display's images against display_model on the bloom model's output under the exposure E.  The tolerance on the
    tone-mapped values: display_model's own plus what the bloom bound, the rounding of x E on the device and the model's cast of
    its input to float32 (2 u E max(out)) can move them."""
    m = bm.chain(fb, E)
    x = np.concatenate([m["out"] * E, fb[..., 3:].astype(np.float64)], -1)
    moved = E * bm.bound_out(m) + 2.0 * bm.U32 * E * float(m["out"].max())
    tol = dm.TOL + tone_slope() * moved
    model = dm.display(x, b, k)
    model["out"][..., 3] = model["other"][..., 3] = model["A"][..., 3] = model["B"][..., 3] = np.clip(fb[..., 3].astype(np.float64), 0.0, 1.0)
    if got32 is not None:
        dm.judge(got32, model, tol=tol, label=label + " rgba32f")
    dm.judge(got8, model, tol=tol, label=label + " rgba8")
    return tol


def check_display_routes(pkg, c, fresh):
    """read_display with bloom on: manual exposure one stop up (E = 2), then auto (E from the meter, whose histogram is the
    unbloomed image's — `fresh` is a context that meters the same framebuffer without bloom)."""
    scene = _render(pkg, c)
    b, k = scene.camera.brightness, scene.camera.contrast
    fb = c.framebuffer()
    plain = c.display("rgba8")
    c.set_setting("display_bloom", 1)
    c.set_setting("display_exposure_ev", 1)
    got8, got32 = c.display("rgba8"), c.display("rgba32f")
    assert not np.array_equal(got8, plain)
    tol = judge_display(fb, 2.0, b, k, got8, got32, "cornell ev=1")
    c.set_setting("display_exposure_ev", 0)
    c.set_setting("display_exposure", "auto")
    got8 = c.display("rgba8")
    rec = c.meter()
    got32 = c.display("rgba32f")
    assert c.meter() == rec and rec["steps"] == 1
    bins, excluded = c.meter_histogram()
    fresh.init(c.width, c.height)
    fresh.set_setting("display_exposure", "auto")
    frec, fbins = fresh.meter_image(fb)
    assert np.array_equal(bins, fbins) and excluded == frec["excluded"]  # the meter saw the unbloomed image
    tol = max(tol, judge_display(fb, rec["exposure"], b, k, got8, got32, "cornell auto"))
    assert np.array_equal(c.framebuffer().view(np.uint32), fb.view(np.uint32))  # the chain leaves the framebuffer alone
    return tol


def test_display_routes(pkg, make_emu):
    print("cornell: tolerance on the displayed values %.3g" % check_display_routes(pkg, make_emu(), make_emu()))


def group_sequence(pkg, lib, n, frames=4):
    """(the single context's display images over `frames` frames, the group's through read_display, the group's through the present
    slots with three frames in flight), bloom on under auto exposure."""
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    settings = {"max_depth": 2, "integrator": "pt", "spp": 4, "display_exposure": "auto", "display_exposure_speed": 0.5,
                "display_bloom": 1, "display_bloom_threshold": 0.5}

    def start(c):
        c.init(70, 51)
        scene.upload(c)
        for k, v in settings.items():
            c.set_setting(k, v)
    one = pkg._binding.CoreBinding(lib, "rfwhip_", 0, 0, 1)
    start(one)
    want = []
    for k in range(frames):
        one.render_frame(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
        want.append(one.display("rgba8"))
    one.set_setting("display_bloom", 0)
    differs = not np.array_equal(one.display("rgba8"), want[-1])
    out = []
    for flight in (False, True):
        g = pkg._binding.RenderGroup(lib, "rfwhip_", [0] * n, "peer")
        start(g)
        got = []
        if not flight:
            for k in range(frames):
                g.render_frame(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
                got.append(g.display("rgba8"))
        else:
            slots = 3
            for k in range(frames):
                g.render_async(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
                if k >= slots:
                    got.append(np.array(g.present_display_wait(k % slots)))
                g.present_display_async(k % slots, "rgba8")
            for k in range(max(frames - slots, 0), frames):
                got.append(np.array(g.present_display_wait(k % slots)))
        g.destroy()
        out.append(got)
    return want, out[0], out[1], differs


def check_group(pkg, lib, n):
    want, read, flight, differs = group_sequence(pkg, lib, n)
    assert differs  # (bloom does something to this scene)
    for k, img in enumerate(want):
        assert np.array_equal(read[k], img), k
        assert np.array_equal(flight[k], img), k


@pytest.mark.parametrize("n", [2, 3])
def test_group_equals_the_single_context(pkg, emu_lib, n):
    check_group(pkg, emu_lib, n)


def test_settings_and_refusals(make_emu):
    c = make_emu()
    for k, v in bm.DEFAULTS.items():
        assert c.get_setting(k) == v, k
    for key, values in (("display_bloom", ("1", "0")), ("display_bloom_intensity", ("0", "16", "0.2")),
                        ("display_bloom_threshold", ("0", "2.5", "1")), ("display_bloom_knee", ("0", "1", "0.5")),
                        ("display_bloom_scatter", ("0", "1", "0.7")), ("display_bloom_levels", ("1", "8", "6"))):
        for v in values:
            c.set_setting(key, v)
            assert c.get_setting(key) == v
    refused = (("display_bloom", "2", 'display_bloom must be "0" or "1"'), ("display_bloom", "on", 'display_bloom must be "0" or "1"'),
               ("display_bloom", "", 'display_bloom must be "0" or "1"'),
               ("display_bloom_intensity", "-0.1", "display_bloom_intensity must be in [0, 16]"),
               ("display_bloom_intensity", "16.5", "display_bloom_intensity must be in [0, 16]"),
               ("display_bloom_intensity", "nan", "display_bloom_intensity must be in [0, 16]"),
               ("display_bloom_intensity", "bright", "display_bloom_intensity must be in [0, 16]"),
               ("display_bloom_threshold", "-1", "display_bloom_threshold must be a finite number >= 0"),
               ("display_bloom_threshold", "inf", "display_bloom_threshold must be a finite number >= 0"),
               ("display_bloom_threshold", "", "display_bloom_threshold must be a finite number >= 0"),
               ("display_bloom_knee", "1.5", "display_bloom_knee must be in [0, 1]"),
               ("display_bloom_knee", "-0.5", "display_bloom_knee must be in [0, 1]"),
               ("display_bloom_knee", "x", "display_bloom_knee must be in [0, 1]"),
               ("display_bloom_scatter", "1.01", "display_bloom_scatter must be in [0, 1]"),
               ("display_bloom_scatter", "-1", "display_bloom_scatter must be in [0, 1]"),
               ("display_bloom_scatter", "nan", "display_bloom_scatter must be in [0, 1]"),
               ("display_bloom_levels", "0", "display_bloom_levels must be a whole number in [1, 8]"),
               ("display_bloom_levels", "9", "display_bloom_levels must be a whole number in [1, 8]"),
               ("display_bloom_levels", "2.5", "display_bloom_levels must be a whole number in [1, 8]"),
               ("display_bloom_levels", "", "display_bloom_levels must be a whole number in [1, 8]"))
    for key, value, text in refused:
        before = {k: c.get_setting(k) for k in bm.DEFAULTS}
        with pytest.raises(RuntimeError) as e:
            c.set_setting(key, value)
        assert text in str(e.value), (key, value, str(e.value))
        assert {k: c.get_setting(k) for k in bm.DEFAULTS} == before
    keys = c.get_settings()
    assert len(keys) == 31 and not any(k.startswith("display") for k in keys)


def test_errors(make_emu, emu_lib):
    lib = emu_lib
    lib.rfwhip_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    lib.rfwhip_bloom_image.restype, lib.rfwhip_bloom_image.argtypes = ctypes.c_int, [vp, vp, ctypes.c_float, vp]
    lib.rfwhip_read_bloom_level.restype, lib.rfwhip_read_bloom_level.argtypes = ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_size_t, vp, vp]
    c = make_emu()
    img, out = np.ones((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float32)
    assert lib.rfwhip_bloom_image(c._ctx, img.ctypes.data, 1.0, out.ctypes.data) != 0 and b"no render target" in lib.rfwhip_last_error()
    c.init(4, 4)
    with pytest.raises(RuntimeError, match="no bloom chain has run"):
        c.read_bloom_level(1)
    assert lib.rfwhip_bloom_image(c._ctx, None, 1.0, out.ctypes.data) != 0 and lib.rfwhip_bloom_image(c._ctx, img.ctypes.data, 1.0, None) != 0
    assert lib.rfwhip_bloom_image(None, img.ctypes.data, 1.0, out.ctypes.data) != 0
    for bad in (-1.0, float("nan"), float("inf")):
        assert lib.rfwhip_bloom_image(c._ctx, img.ctypes.data, bad, out.ctypes.data) != 0 and b"finite number >= 0" in lib.rfwhip_last_error()
    assert lib.rfwhip_bloom_image(c._ctx, img.ctypes.data, 1.0, out.ctypes.data) == 0
    # 4 x 4 reaches 1 x 1 at level 2: the default six levels run as two
    assert c.read_bloom_level(1).shape == (2, 2, 4) and c.read_bloom_level(2).shape == (1, 1, 4)
    for level in (0, 3):
        with pytest.raises(RuntimeError, match="the last chain ran levels 1 .. 2"):
            c.read_bloom_level(level)
    small = np.zeros(15, np.float32)
    assert lib.rfwhip_read_bloom_level(c._ctx, 1, small.ctypes.data, small.size, None, None) != 0 and b"room for 15 floats" in lib.rfwhip_last_error()
    # rfwhip_init frees the pyramid: no chain to read
    c.init(4, 4)
    with pytest.raises(RuntimeError, match="no bloom chain has run"):
        c.read_bloom_level(1)
