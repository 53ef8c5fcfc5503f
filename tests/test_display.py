"""The display stage (include/rfwhip.h, rfwhip_read_display; csrc/display.h), CPU tier: the host-emulation build runs the same
work item as the HIP kernel, with a direct fetch in place of the LDS tile.  Held to the float64 model of tests/display_model.py
by its judging rule, to the settings contract, and to the single context for groups."""
import ctypes
import itertools

import numpy as np
import pytest

import display_model as dm

COMBOS = list(itertools.product(("aces", "none"), (1, 0), (0, 1)))  # tone map, FXAA, sRGB


def _set(c, tonemap="aces", fxaa=1, srgb=0):
    c.set_setting("display_tonemap", tonemap)
    c.set_setting("display_fxaa", fxaa)
    c.set_setting("display_srgb", srgb)


def _judge_both(c, img, b, k, tonemap, fxaa, srgb, label):
    m = dm.display(img, b, k, tonemap, bool(fxaa), bool(srgb))
    f = c.display_image(img, b, k, "rgba32f")
    assert f.dtype == np.float32 and f.shape == img.shape
    print("%s: float max |err| %.3g" % (label, float(np.abs(f - m["out"]).max())))
    dm.judge(f, m, bool(srgb), label=label + " rgba32f")
    u = c.display_image(img, b, k, "rgba8")
    assert u.dtype == np.uint8 and u.shape == img.shape
    dm.judge(u, m, bool(srgb), label=label + " rgba8")


@pytest.mark.parametrize("size", dm.SIZES, ids=lambda s: "%dx%d" % s)
def test_display_image_matches_the_model(make_emu, size):
    w, h = size
    c = make_emu()
    c.init(w, h)
    for kind in dm.KINDS:
        img = dm.image(kind, w, h)
        for tonemap, fxaa, srgb in COMBOS:
            _set(c, tonemap, fxaa, srgb)
            _judge_both(c, img, 0.05, 1.0, tonemap, fxaa, srgb, "%s %dx%d %s fxaa=%d srgb=%d" % (kind, w, h, tonemap, fxaa, srgb))
    # another brightness / contrast goes through too
    _set(c)
    _judge_both(c, dm.image("noise", w, h), 0.2, 0.7, "aces", 1, 0, "noise b=0.2 c=0.7")


def test_settings(make_emu):
    c = make_emu()
    assert (c.get_setting("display_tonemap"), c.get_setting("display_fxaa"), c.get_setting("display_srgb")) == ("aces", "1", "0")
    for key, values in (("display_tonemap", ("none", "aces")), ("display_fxaa", ("0", "1")), ("display_srgb", ("1", "0"))):
        for v in values:
            c.set_setting(key, v)
            assert c.get_setting(key) == v
    for key, value, text in (("display_tonemap", "reinhard", 'display_tonemap must be "aces" or "none"'),
                             ("display_tonemap", "", 'display_tonemap must be "aces" or "none"'),
                             ("display_fxaa", "2", 'display_fxaa must be "0" or "1"'),
                             ("display_fxaa", "on", 'display_fxaa must be "0" or "1"'),
                             ("display_srgb", "yes", 'display_srgb must be "0" or "1"')):
        with pytest.raises(RuntimeError) as e:
            c.set_setting(key, value)
        assert text in str(e.value)
        assert c.get_setting(key) in ("aces", "0", "1")  # unchanged by the refused value
    keys = c.get_settings()
    assert len(keys) == 31 and not any(k.startswith("display") for k in keys)


def _render(pkg, c, scene, w, h, spp=4, **settings):
    c.init(w, h)
    scene.upload(c)
    c.set_setting("integrator", "pt")
    c.set_setting("spp", spp)
    for k, v in settings.items():
        c.set_setting(k, v)
    c.render_frame(scene.camera, pkg.RESET)
    return c


def test_rendered_frame(pkg, make_emu):
    scene = pkg.scenes.cornell(96, 64)
    scene.camera.brightness, scene.camera.contrast = 0.1, 0.9
    c = _render(pkg, make_emu(), scene, 96, 64)

    def check(label):
        fb = c.framebuffer()
        m = dm.display(fb, 0.1, 0.9)
        dm.judge(c.display("rgba32f"), m, label=label + " rgba32f")
        assert np.array_equal(c.framebuffer().view(np.uint32), fb.view(np.uint32))
        dm.judge(c.display("rgba8"), m, label=label + " rgba8")
        assert np.array_equal(c.framebuffer().view(np.uint32), fb.view(np.uint32))
        return fb
    raw = check("raw")
    assert raw[..., :3].max() > 1.0  # an HDR image: the tone map has work to do
    c.set_setting("denoise", 1)
    den = check("denoised")
    assert not np.array_equal(den, raw)
    assert np.array_equal(c.display(), c.display())


def test_before_the_first_render_the_defaults_apply_to_the_empty_image(make_emu):
    c = make_emu()
    c.init(21, 9)
    empty = np.zeros((9, 21, 4), np.float32)
    assert np.array_equal(c.framebuffer(), empty)
    dm.judge(c.display("rgba32f"), dm.display(empty, 0.05, 1.0), label="empty")
    assert c.display("rgba8")[..., :3].max() > 0  # (brightness 0.05 lifts black)


@pytest.mark.parametrize("fxaa", [1, 0])
def test_constant_image_is_the_tone_map_of_the_constant(make_emu, fxaa):
    c = make_emu()
    c.init(37, 23)
    _set(c, fxaa=fxaa)
    img = np.empty((23, 37, 4), np.float32)
    img[...] = (0.8, 0.35, 2.5, 0.6)
    t, a = dm.tone(img[:1, :1], 0.05, 1.0)
    out = c.display_image(img, 0.05, 1.0, "rgba32f")
    assert np.abs(out[..., :3] - t[0, 0]).max() <= dm.TOL and np.abs(out[..., 3] - a[0, 0]).max() <= 1e-7
    b = c.display_image(img, 0.05, 1.0, "rgba8")
    assert (b == b[0, 0]).all()


@pytest.mark.parametrize("n", [2, 3])
def test_group_equals_the_single_context(pkg, make_emu, emu_lib, n):
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)  # (the scene of test_group.py's equality test, 70 x 51: ragged strips)
    settings = {"max_depth": 2}
    frames = 3
    one = make_emu()
    want8, want32 = [], []
    for k in range(frames):
        if k == 0:
            _render(pkg, one, scene, 70, 51, spp=4, **settings)
        else:
            one.render_frame(scene.camera, pkg.CONVERGE)
        want8.append(one.display("rgba8")), want32.append(one.display("rgba32f"))
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0] * n, "peer")
    g.init(70, 51)
    scene.upload(g)
    for k, v in dict(settings, integrator="pt", spp=4).items():
        g.set_setting(k, v)
    g.render_frame(scene.camera, pkg.RESET)
    assert np.array_equal(g.display("rgba8"), want8[0])
    assert np.array_equal(g.display("rgba32f"), want32[0])
    # frames in flight through the display slots: frame k into slot k % 2, the frame before it handed out meanwhile
    g.present_display_async(0, "rgba8")
    for k in range(1, frames):
        g.render_async(scene.camera, pkg.CONVERGE)
        g.present_display_async(k % 2, "rgba8" if k % 2 == 0 else "rgba32f")
        shown = g.present_display_wait((k - 1) % 2)
        assert np.array_equal(shown, (want8 if (k - 1) % 2 == 0 else want32)[k - 1]), k
    last = g.present_display_wait((frames - 1) % 2)
    assert last.dtype == np.uint8 and np.array_equal(last, want8[frames - 1])
    # a slot remembers what was presented into it
    with pytest.raises(RuntimeError) as e:
        g.present_wait(0)
    assert "holds a display image" in str(e.value)
    g.present_async(1)
    with pytest.raises(RuntimeError) as e:
        g.present_display_wait(1)
    assert "holds a float image" in str(e.value)
    assert np.array_equal(g.present_wait(1), one.framebuffer())
    with pytest.raises(RuntimeError):
        g.present_display_wait(2)  # nothing presented
    with pytest.raises(RuntimeError):
        g.present_display_async(0, 7)
    with pytest.raises(RuntimeError):
        g.present_display_async(4, "rgba8")
    with pytest.raises(RuntimeError):
        g.display(2)
    g.destroy()


def test_errors(make_emu, emu_lib):
    c = make_emu()
    img = np.zeros((4, 4, 4), np.float32)
    lib = emu_lib
    lib.rfwhip_last_error.restype = ctypes.c_char_p
    fn = lib.rfwhip_display_image
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    out = np.zeros((4, 4, 4), np.float32)
    # no render target
    assert fn(c._ctx, img.ctypes.data, 0.05, 1.0, 0, out.ctypes.data) != 0 and b"no render target" in lib.rfwhip_last_error()
    with pytest.raises(RuntimeError, match="no render target"):
        c.display()
    c.init(4, 4)
    assert fn(c._ctx, img.ctypes.data, 0.05, 1.0, 0, out.ctypes.data) == 0
    # null pointers, an unknown format
    assert fn(c._ctx, None, 0.05, 1.0, 0, out.ctypes.data) != 0
    assert fn(c._ctx, img.ctypes.data, 0.05, 1.0, 0, None) != 0
    assert fn(None, img.ctypes.data, 0.05, 1.0, 0, out.ctypes.data) != 0
    for call in (lambda: c.display_image(img, format=2), lambda: c.display(2), lambda: c.display(-1),
                 lambda: c.read_display_device(out.ctypes.data, 5), lambda: c.display_stream(img.ctypes.data, out.ctypes.data, 3)):
        with pytest.raises(RuntimeError, match="unknown display format"):
            call()
    with pytest.raises(RuntimeError, match="null"):
        c.read_display_device(0)
    with pytest.raises(RuntimeError, match="null"):
        c.display_stream(0, out.ctypes.data)
    with pytest.raises(RuntimeError, match="null"):
        c.display_stream(img.ctypes.data, 0)
    with pytest.raises(RuntimeError, match="in place"):
        c.display_stream(out.ctypes.data, out.ctypes.data, "rgba32f")
    # the stream-ordered form is the same stage (emulation: host memory stands in for the device's)
    src = dm.image("noise", 4, 4)
    c.display_stream(src.ctypes.data, out.ctypes.data, "rgba32f")
    c.wait()
    assert np.array_equal(out, c.display_image(src, 0.05, 1.0, "rgba32f"))
    # a rank of a larger world owns strips: no display of its own
    r = make_emu(1, 2)
    r.init(8, 8)
    with pytest.raises(RuntimeError, match="owns 1/2"):
        r.display()


def test_camera_defaults_are_the_references(pkg):
    cam = pkg.Camera()
    assert (cam.brightness, cam.contrast) == (0.05, 1.0)
    pod = cam.pod()
    assert abs(pod.brightness - 0.05) < 1e-8 and pod.contrast == 1.0
