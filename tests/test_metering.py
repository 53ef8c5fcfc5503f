"""The exposure meter (include/rfwhip.h, rfwhip_get_meter; csrc/metering.h), CPU tier: the host-emulation build runs the same work
items as the HIP kernels.  Held to the float64 model of tests/metering_model.py by its judging rules, to the settings contract,
and to the single context for groups."""
import ctypes

import numpy as np
import pytest

import display_model as dm
import metering_model as mm


def _auto(c, **settings):
    c.set_setting("display_exposure", "auto")
    for k, v in settings.items():
        c.set_setting("display_exposure_" + k, v)


def edge_values():
    """Every one of the 257 edges 2^e (1 + s / 8) and the floats one ulp below and above, and the special values."""
    edges = np.array([2.0 ** ((b >> 3) - 16) * (1.0 + (b & 7) / 8.0) for b in range(mm.BINS + 1)], np.float32)
    below, above = np.nextafter(edges, np.float32(0)), np.nextafter(edges, np.float32(np.inf))
    special = np.array([0.0, -0.0, 1e-41, 2.0 ** -126, np.finfo(np.float32).max, np.inf, -1.0, -np.inf, np.nan, 1.0, 0.18], np.float32)
    return np.concatenate([edges, below, above, special])


def check_meter_bin(c):
    y = edge_values()
    pad = (-len(y)) % 8
    rec = np.zeros(((len(y) + pad) // 8, 24), np.float32)
    rec[:, :8] = np.concatenate([y, np.ones(pad, np.float32)]).reshape(-1, 8)
    got = c.kat("meter_bin", rec).view(np.int32).ravel()[:len(y)]
    want = np.array([mm.bin_of_float32(v) for v in y], np.int32)
    assert np.array_equal(got, want), "first mismatch at Y = %r" % y[np.flatnonzero(got != want)[0]]
    # the edges themselves: edge b opens bin b (the last one is 2^16: bin 255 with everything above it)
    assert np.array_equal(got[:mm.BINS + 1], np.minimum(np.arange(mm.BINS + 1), mm.BINS - 1))
    # one ulp below edge b lies in bin b - 1 (below the first edge: bin 0)
    assert np.array_equal(got[mm.BINS + 1:2 * mm.BINS + 2], np.maximum(np.arange(mm.BINS + 1) - 1, 0))
    assert list(got[-11:-2]) == [-1, -1, 0, 0, 255, -1, -1, -1, -1]


def test_meter_bin_known_answers(make_emu):
    c = make_emu()
    c.init(4, 4)
    check_meter_bin(c)


def check_histograms(c, w, h):
    """The histogram of every image kind at one size against the model; returns the largest ambiguous count."""
    worst = 0
    for kind in mm.KINDS:
        img = dm.image(kind, w, h)
        rec, bins = c.meter_image(img)
        model = mm.histogram(img)
        worst = max(worst, mm.judge_histogram(bins, rec["excluded"], model, "%s %dx%d" % (kind, w, h)))
        assert rec["valid"] == model["valid"]
        b2, ex2 = c.meter_histogram()
        assert np.array_equal(b2, bins) and ex2 == rec["excluded"]
    img, exact = mm.bin_centres(w, h)
    rec, bins = c.meter_image(img)
    assert np.array_equal(bins, exact) and rec["excluded"] == 0 and rec["valid"] == w * h
    rec, bins = c.meter_image(mm.constant(w, h))
    assert bins.max() == w * h and int(bins.sum()) == w * h and rec["excluded"] == 0
    return worst


@pytest.mark.parametrize("size", mm.SIZES, ids=lambda s: "%dx%d" % s)
def test_histogram_matches_the_model(make_emu, size):
    w, h = size
    c = make_emu()
    c.init(w, h)
    _auto(c)
    print("%dx%d: at most %d ambiguous pixels" % (w, h, check_histograms(c, w, h)))


def test_all_excluded_image_is_no_step(make_emu):
    w, h = 37, 23
    c = make_emu()
    c.init(w, h)
    img = mm.all_excluded(w, h)
    manual = c.display_image(img, 0.05, 1.0, "rgba8")
    _auto(c)
    rec, bins = c.meter_image(img)
    assert (rec["valid"], rec["excluded"], rec["steps"], rec["exposure"]) == (0, w * h, 0, 1.0) and not bins.any()
    assert np.array_equal(c.display_image(img, 0.05, 1.0, "rgba8"), manual)
    assert c.meter()["steps"] == 0
    # ... and after a step the state stays
    before, _ = c.meter_image(dm.image("noise", w, h))
    after, _ = c.meter_image(img)
    assert before["steps"] == after["steps"] == 1 and after["exposure"] == before["exposure"]
    assert after["log2_exposure"] == before["log2_exposure"] and (after["valid"], after["excluded"]) == (0, w * h)


def posed_histograms():
    """(label, bins, settings) of the reduce's known answers."""
    def one(b, n=1000):
        h = np.zeros(mm.BINS, np.uint32)
        h[b] = n
        return h
    two = np.zeros(mm.BINS, np.uint32)
    two[100], two[140] = 300, 700  # lo = 100, hi = 900: both ends fall inside a bin
    rng = np.random.default_rng(11)
    spread = rng.integers(0, 5000, mm.BINS).astype(np.uint32)
    big = np.zeros(mm.BINS, np.uint32)
    big[7], big[128], big[250] = 2 ** 31, 2 ** 31 - 5, 4  # sums to 2^32 - 1
    return [("one bin", one(93), {}), ("two bins", two, {}), ("plain mean", spread, {"low": 0, "high": 1}),
            ("window inside one bin", two, {"low": 0.4, "high": 0.6}), ("near 2^32", big, {}),
            ("clamp at max_ev", one(3), {"max_ev": 4}), ("clamp at min_ev", one(250), {"min_ev": -3}),
            ("key and compensation", spread, {"key": 0.5, "ev": -1.25})]


def check_posed(c):
    worst = 0.0
    for label, bins, settings in posed_histograms():
        for k, v in mm.DEFAULTS.items():
            c.set_setting(k, v)
        _auto(c, **settings)
        c.meter_reset()
        rec = c.meter_from_histogram(bins, 5)
        s = {"display_exposure_" + k: v for k, v in settings.items()}
        worst = max(worst, mm.judge_record(rec, bins, s, None, label))
        assert rec["excluded"] == 5 and rec["valid"] == int(bins.astype(np.uint64).sum())
        if label == "one bin":
            assert rec["log2_luminance"] == np.float32(mm.LAMBDA[93])
        if label.startswith("clamp"):
            assert rec["log2_target"] == (4.0 if "max" in label else -3.0) == rec["log2_exposure"]
    # N = 0: no step
    c.meter_reset()
    rec = c.meter_from_histogram(np.zeros(mm.BINS, np.uint32), 77)
    assert (rec["steps"], rec["exposure"], rec["valid"], rec["excluded"]) == (0, 1.0, 0, 77)
    return worst


def test_reduce_on_posed_histograms(make_emu):
    c = make_emu()
    c.init(8, 8)
    print("posed histograms: largest error / bound %.3g" % check_posed(c))
    with pytest.raises(RuntimeError, match="more than 2\\^32 - 1"):
        c.meter_from_histogram(np.full(mm.BINS, 2 ** 25, np.uint32))
    with pytest.raises(ValueError, match="256 bins"):
        c.meter_from_histogram(np.zeros(255, np.uint32))


def check_adaptation(c, w, h):
    """Images A, B, B, B at speed 0.5: l follows the recurrence; a reset makes the next step a first step; speed 1 is idempotent."""
    a, b = dm.image("noise", w, h), 8.0 * dm.image("stripes", w, h)
    s = {"display_exposure_speed": "0.5"}
    _auto(c, speed=0.5)
    c.meter_reset()
    prev, worst, ls = None, 0.0, []
    for k, img in enumerate((a, b, b, b)):
        rec, bins = c.meter_image(img)
        worst = max(worst, mm.judge_record(rec, bins, s, prev, "step %d" % k))
        prev = rec
        ls.append(rec["log2_exposure"])
    assert prev["steps"] == 4 and ls[0] != ls[1] and abs(ls[3] - prev["log2_target"]) < abs(ls[1] - prev["log2_target"])
    c.meter_reset()
    assert c.meter()["steps"] == 0 and c.meter()["exposure"] == 1.0
    rec, bins = c.meter_image(b)
    assert rec["steps"] == 1 and rec["log2_exposure"] == rec["log2_target"]
    worst = max(worst, mm.judge_record(rec, bins, s, None, "after reset"))
    _auto(c, speed=1)
    r1, _ = c.meter_image(a)
    r2, _ = c.meter_image(a)
    assert r2["steps"] == r1["steps"] + 1 and {k: v for k, v in r1.items() if k != "steps"} == {k: v for k, v in r2.items() if k != "steps"}
    return worst


def test_adaptation(make_emu):
    c = make_emu()
    c.init(37, 23)
    print("adaptation: largest error / bound %.3g" % check_adaptation(c, 37, 23))


def _render(pkg, c, scene, w, h, spp=4, **settings):
    c.init(w, h)
    scene.upload(c)
    c.set_setting("integrator", "pt")
    c.set_setting("spp", spp)
    for k, v in settings.items():
        c.set_setting(k, v)
    c.render_frame(scene.camera, pkg.RESET)
    return c


def check_rendered_frame(pkg, c):
    """A Cornell frame under auto exposure: the step rule, and the display held to the model on its own framebuffer."""
    scene = pkg.scenes.cornell(96, 64)
    scene.camera.brightness, scene.camera.contrast = 0.1, 0.9
    _render(pkg, c, scene, 96, 64)
    _auto(c)
    fb = c.framebuffer()
    u8 = c.display("rgba8")
    rec = c.meter()
    f32 = c.display("rgba32f")
    assert c.meter() == rec and rec["steps"] == 1  # one step per render call
    assert np.array_equal(c.display("rgba8"), u8) and np.array_equal(c.display("rgba32f"), f32)
    assert np.array_equal(c.framebuffer().view(np.uint32), fb.view(np.uint32))
    bins, excluded = c.meter_histogram()
    mm.judge_histogram(bins, excluded, mm.histogram(fb), "cornell")
    worst = mm.judge_record(rec, bins, None, None, "cornell")
    m = dm.display(fb * np.float32(rec["exposure"]), 0.1, 0.9)
    m["out"][..., 3] = m["other"][..., 3] = m["A"][..., 3] = m["B"][..., 3] = np.clip(fb[..., 3].astype(np.float64), 0.0, 1.0)
    dm.judge(f32, m, label="cornell auto rgba32f")
    dm.judge(u8, m, label="cornell auto rgba8")
    # another render: another step; a changed setting meters the same frame again
    c.render_frame(scene.camera, pkg.CONVERGE)
    c.display("rgba8")
    assert c.meter()["steps"] == 2
    c.display("rgba8")
    r2 = c.meter()
    assert r2["steps"] == 2
    c.set_setting("display_exposure_key", 0.36)
    c.display("rgba8")
    r3 = c.meter()
    assert r3["steps"] == 3 and r3["log2_target"] > r2["log2_target"] + 0.9  # (twice the key: one stop up)
    worst = max(worst, mm.judge_record(r3, c.meter_histogram()[0], {"display_exposure_key": "0.36"}, r2, "cornell, key 0.36"))
    # display_image is a step every call
    c.display_image(fb, 0.1, 0.9, "rgba8")
    c.display_image(fb, 0.1, 0.9, "rgba8")
    assert c.meter()["steps"] == 5
    return worst


def test_rendered_frame_and_the_step_rule(pkg, make_emu):
    print("cornell: largest error / bound %.3g" % check_rendered_frame(pkg, make_emu()))


def _exposed_model(img, E, b, k, tonemap, fxaa):
    x = np.array(img, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x[..., :3] = x[..., :3] * np.float32(E)
    m = dm.display(x, b, k, tonemap, bool(fxaa), False)
    return m


def check_displayed_image(c, w, h):
    for kind in ("noise", "stripes", "nonfinite"):
        img = dm.image(kind, w, h)
        for tonemap in ("aces", "none"):
            for fxaa in (1, 0):
                c.set_setting("display_tonemap", tonemap)
                c.set_setting("display_fxaa", fxaa)
                _auto(c, ev=0)
                for fmt in ("rgba32f", "rgba8"):
                    got = c.display_image(img, 0.05, 1.0, fmt)
                    E = c.meter()["exposure"]
                    dm.judge(got, _exposed_model(img, E, 0.05, 1.0, tonemap, fxaa), label="%s auto %s fxaa=%d %s" % (kind, tonemap, fxaa, fmt))
                # manual, one stop up: the model at 2 x the image
                c.set_setting("display_exposure", "manual")
                c.set_setting("display_exposure_ev", 1)
                for fmt in ("rgba32f", "rgba8"):
                    got = c.display_image(img, 0.05, 1.0, fmt)
                    dm.judge(got, _exposed_model(img, 2.0, 0.05, 1.0, tonemap, fxaa), label="%s ev=1 %s fxaa=%d %s" % (kind, tonemap, fxaa, fmt))
                assert c.meter()["exposure"] == 2.0
                c.set_setting("display_exposure_ev", 0)
    c.set_setting("display_tonemap", "aces")
    c.set_setting("display_fxaa", 1)


@pytest.mark.parametrize("size", [(37, 23), (130, 70)], ids=lambda s: "%dx%d" % s)
def test_displayed_image_matches_the_model(make_emu, size):
    w, h = size
    c = make_emu()
    c.init(w, h)
    check_displayed_image(c, w, h)


def test_manual_ev_zero_is_the_unexposed_stage(make_emu):
    c, d = make_emu(), make_emu()
    c.init(37, 23), d.init(37, 23)
    img = dm.image("noise", 37, 23)
    d.set_setting("display_exposure_ev", 1)
    d.set_setting("display_exposure_ev", 0)
    for fmt in ("rgba8", "rgba32f"):
        assert np.array_equal(c.display_image(img, 0.05, 1.0, fmt), d.display_image(img, 0.05, 1.0, fmt))
    assert d.meter()["steps"] == 0 and d.meter()["exposure"] == 1.0


def test_settings(make_emu):
    c = make_emu()
    for k, v in mm.DEFAULTS.items():
        assert c.get_setting(k) == v, k
    for key, values in (("display_exposure", ("auto", "manual")), ("display_exposure_ev", ("-2.5", "32", "0")),
                        ("display_exposure_key", ("0.5", "0.18")), ("display_exposure_low", ("0", "0.25")),
                        ("display_exposure_high", ("1", "0.75")), ("display_exposure_speed", ("0.125", "1")),
                        ("display_exposure_min_ev", ("-64", "-8")), ("display_exposure_max_ev", ("64", "8"))):
        for v in values:
            c.set_setting(key, v)
            assert c.get_setting(key) == v
    refused = (("display_exposure", "on", 'display_exposure must be "manual" or "auto"'),
               ("display_exposure", "", 'display_exposure must be "manual" or "auto"'),
               ("display_exposure_ev", "33", "display_exposure_ev must be a finite number in [-32, 32]"),
               ("display_exposure_ev", "nan", "display_exposure_ev must be a finite number in [-32, 32]"),
               ("display_exposure_ev", "", "display_exposure_ev must be a finite number in [-32, 32]"),
               ("display_exposure_key", "0", "display_exposure_key must be a finite number > 0"),
               ("display_exposure_key", "inf", "display_exposure_key must be a finite number > 0"),
               ("display_exposure_key", "-1", "display_exposure_key must be a finite number > 0"),
               ("display_exposure_low", "0.75", "display_exposure_low must be in [0, 1] and below display_exposure_high"),
               ("display_exposure_low", "0.9", "display_exposure_low must be in [0, 1] and below display_exposure_high"),
               ("display_exposure_low", "-0.1", "display_exposure_low must be in [0, 1] and below display_exposure_high"),
               ("display_exposure_high", "0.25", "display_exposure_high must be in [0, 1] and above display_exposure_low"),
               ("display_exposure_high", "0.1", "display_exposure_high must be in [0, 1] and above display_exposure_low"),
               ("display_exposure_high", "1.5", "display_exposure_high must be in [0, 1] and above display_exposure_low"),
               ("display_exposure_speed", "0", "display_exposure_speed must be in (0, 1]"),
               ("display_exposure_speed", "1.5", "display_exposure_speed must be in (0, 1]"),
               ("display_exposure_min_ev", "9", "display_exposure_min_ev must be a finite number in [-64, 64], at most display_exposure_max_ev"),
               ("display_exposure_max_ev", "-9", "display_exposure_max_ev must be a finite number in [-64, 64], at least display_exposure_min_ev"),
               ("display_exposure_max_ev", "65", "display_exposure_max_ev must be a finite number in [-64, 64], at least display_exposure_min_ev"))
    for key, value, text in refused:
        before = {k: c.get_setting(k) for k in mm.DEFAULTS}
        with pytest.raises(RuntimeError) as e:
            c.set_setting(key, value)
        assert text in str(e.value), (key, value, str(e.value))
        assert {k: c.get_setting(k) for k in mm.DEFAULTS} == before  # a refused set leaves every value (both ends of a pair) unchanged
    keys = c.get_settings()
    assert len(keys) == 31 and not any(k.startswith("display") for k in keys)


def group_sequence(pkg, lib, n, frames=4):
    """(single context's display images and records over `frames` frames, the group's through read_display, the group's through the
    present slots with frames in flight): auto exposure at speed 0.5."""
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    settings = {"max_depth": 2, "integrator": "pt", "spp": 4, "display_exposure": "auto", "display_exposure_speed": 0.5}

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
        want.append((one.display("rgba8"), one.meter()))
    out = []
    for flight in (False, True):
        g = pkg._binding.RenderGroup(lib, "rfwhip_", [0] * n, "peer")
        start(g)
        got = []
        if not flight:
            for k in range(frames):
                g.render_frame(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
                got.append((g.display("rgba8"), g.meter()))
        else:
            slots = 3
            for k in range(frames):
                g.render_async(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
                if k >= slots:
                    got.append((np.array(g.present_display_wait(k % slots)), None))
                g.present_display_async(k % slots, "rgba8")
            for k in range(max(frames - slots, 0), frames):
                got.append((np.array(g.present_display_wait(k % slots)), None))
            got[-1] = (got[-1][0], g.meter())
        g.destroy()
        out.append(got)
    return want, out[0], out[1]


def check_group(pkg, lib, n):
    want, read, flight = group_sequence(pkg, lib, n)
    assert want[-1][1]["steps"] == len(want) and len({w[1]["log2_exposure"] for w in want}) > 1  # the exposure is adapting
    for k, (img, rec) in enumerate(want):
        assert np.array_equal(read[k][0], img), k
        assert read[k][1] == rec, (k, read[k][1], rec)
        assert np.array_equal(flight[k][0], img), k
    assert flight[-1][1] == want[-1][1]


@pytest.mark.parametrize("n", [2, 3])
def test_group_equals_the_single_context(pkg, emu_lib, n):
    check_group(pkg, emu_lib, n)


def test_errors(make_emu, emu_lib):
    lib = emu_lib
    lib.rfwhip_last_error.restype = ctypes.c_char_p
    c = make_emu()
    st = (ctypes.c_uint32 * 8)()
    bins = (ctypes.c_uint32 * 256)()
    img = np.zeros((4, 4, 4), np.float32)
    vp = ctypes.c_void_p
    for name, args in (("rfwhip_get_meter", [vp, vp]), ("rfwhip_read_meter_histogram", [vp, vp, vp]), ("rfwhip_meter_reset", [vp]),
                       ("rfwhip_meter_image", [vp, vp, vp, vp]), ("rfwhip_meter_histogram", [vp, vp, ctypes.c_uint32, vp]),
                       ("rfwhip_group_get_meter", [vp, vp])):
        f = getattr(lib, name)
        f.restype, f.argtypes = ctypes.c_int, args
    # before init
    assert lib.rfwhip_get_meter(c._ctx, st) != 0 and b"no render target" in lib.rfwhip_last_error()
    with pytest.raises(RuntimeError, match="no render target"):
        c.meter_reset()
    with pytest.raises(RuntimeError, match="no render target"):
        c.meter_from_histogram(np.zeros(256, np.uint32))
    c.init(4, 4)
    assert lib.rfwhip_get_meter(c._ctx, st) == 0
    # null pointers
    assert lib.rfwhip_get_meter(c._ctx, None) != 0 and lib.rfwhip_get_meter(None, st) != 0
    assert lib.rfwhip_read_meter_histogram(c._ctx, None, None) != 0 and lib.rfwhip_read_meter_histogram(c._ctx, bins, None) == 0
    assert lib.rfwhip_meter_image(c._ctx, None, st, None) != 0 and lib.rfwhip_meter_image(c._ctx, img.ctypes.data, None, None) != 0
    assert lib.rfwhip_meter_image(c._ctx, img.ctypes.data, st, None) == 0
    assert lib.rfwhip_meter_histogram(c._ctx, None, 0, st) != 0 and lib.rfwhip_meter_histogram(c._ctx, bins, 0, None) != 0
    assert lib.rfwhip_meter_reset(None) != 0 and lib.rfwhip_group_get_meter(None, st) != 0
    # a rank of a larger world owns strips: no display of its own, in auto mode either
    r = make_emu(1, 2)
    r.init(8, 8)
    r.set_setting("display_exposure", "auto")
    with pytest.raises(RuntimeError, match="owns 1/2"):
        r.display()
    with pytest.raises(ValueError):
        c.meter_from_histogram(np.zeros(257, np.uint32))
    with pytest.raises(KeyError):
        c.kat("meter_bins", np.zeros((1, 24), np.float32))
