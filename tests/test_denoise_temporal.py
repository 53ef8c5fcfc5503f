"""The denoiser's temporal stage (setting "denoise_temporal", include/rfwhip.h; csrc/denoise.h dn_temporal_item), CPU tier: the
host-emulation build runs the same work items as the HIP kernels.  Held to the numpy model of tests/denoise_temporal_model.py frame
by frame, to the spatial filter bit for bit where the header promises it, to one context for groups, and to a converged render for
quality."""

import numpy as np
import pytest

import denoise_temporal_model as M

W, H = 96, 64


def _ctx(pkg, make_emu, scene, w=W, h=H, spp=1, **settings):
    c = make_emu()
    c.init(w, h)
    scene.upload(c)
    c.set_setting("integrator", "pt")
    c.set_setting("spp", spp)
    for k, v in settings.items():
        c.set_setting(k, v)
    return c


def _scene(pkg, name, w=W, h=H):
    return pkg.scenes.cornell(w, h, geometric_emitter=True) if name == "cornell" else pkg.scenes.cards(w, h)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cut(scene, up=True):
    """A camera above (or below) the scene looking at it: every surface it sees faces away from the earlier views (a cut)."""
    c = M.panned(scene.camera, 0.0)
    y = float(scene.camera.position[1])
    c.look_at((0.1, 3.5 * y if up else -2.0 * y, 0.3), (0.0, y, 0.0))
    return c


def _close(a, b, rtol=1e-4, atol=1e-6):
    return np.isclose(a, b, rtol=rtol, atol=atol)


def check_frame(native_out, hist, out, st):
    """One presented frame against the model (st / out: model_frame's state and output, fed the native history of P)."""
    v = st["valid"]
    # the blend adds a few roundings to the passes'; a pixel whose tap sits on a consistency bound (depth, normal, the weight sum)
    # may round the other way and move its a-trous neighbourhood: at most 1 in 1000 pixels
    close = _close(native_out, out, 5e-4, 1e-6).all(-1)
    assert close.mean() > 0.999, close.mean()
    assert _close(hist["pre"], st["pre"], 1e-3, 1e-5).all(-1).mean() > 0.999
    # the moments, the variance taken from them, n and the colour history carry the rounding of the reprojection's weights times the
    # history's magnitude; a pixel whose tap sits on a consistency bound may also round the other way, and var = mu2 - mu1^2 cancels
    # (at most 1 in 200 pixels)
    ms = st["mscale"]
    ok = _close(hist["length"], st["length"], 1e-4, 1e-3)
    ok &= (np.abs(hist["moments"] - st["moments"]) <= 1e-3 * ms + 1e-6).all(-1)
    from_moments = v & (st["length"] >= M.VAR_N) & (hist["length"] >= M.VAR_N)
    tol = np.where(from_moments, 2e-3 * (ms[..., 1] + ms[..., 0] ** 2) + 1e-6, 1e-4 * np.abs(st["var"]) + 1e-6)
    ok &= np.abs(hist["var"] - st["var"]) <= tol
    ok &= _close(hist["history"], st["history"], 1e-3, 1e-5).all(-1)
    assert ok.mean() > 0.995, ok.mean()
    assert (hist["length"][~v] == 0).all()


def _seq_cameras(scene, n=6, step=0.03):
    return [M.panned(scene.camera, step * k) for k in range(n)] + [_cut(scene)]


@pytest.mark.parametrize("name", ["cornell", "cards"])
def test_moving_sequence_matches_the_model(pkg, make_emu, name):
    scene = _scene(pkg, name)
    den = _ctx(pkg, make_emu, scene, denoise=1, denoise_temporal=1)
    raw_ctx = _ctx(pkg, make_emu, scene, denoise_temporal=1)  # (the same samples: the origin does not depend on "denoise")
    changed = np.zeros(len(scene.instances), bool)
    prev = None
    cams = _seq_cameras(scene)
    for f, cam in enumerate(cams):
        den.render_frame(cam, pkg.RESET)
        raw_ctx.render_frame(cam, pkg.RESET)
        raw = raw_ctx.framebuffer()
        out = den.framebuffer()
        assert np.array_equal(_bits(den.framebuffer()), _bits(out)), f  # a further read of the same frame: the same bits
        hist = den.read_denoise_history()
        want, st = M.model_frame(den, cam, raw, prev, changed)
        check_frame(out, hist, want, st)
        v = st["valid"]
        assert v.mean() > (0.1 if f == len(cams) - 1 else 0.3), f
        if f == 0 or f == len(cams) - 1:
            # the first frame and the cut: fresh everywhere, the spatial filter's output bit for bit
            assert (hist["length"][v] == 1).all(), f
            assert np.array_equal(_bits(out), _bits(den.denoise_image(raw))), f
        else:
            assert hist["length"][v].mean() > f + 0.5, f  # the history grows along the pan
            assert not np.array_equal(out, den.denoise_image(raw))
        prev = dict(st, history=hist["history"], moments=hist["moments"], length=hist["length"])
    # reads do not advance the history: the last frame's stage once more gives the same values
    again = den.read_denoise_history()
    for k in hist:
        assert np.array_equal(_bits(again[k]), _bits(hist[k])), k


def test_converge_frames_are_the_spatial_filter(pkg, make_emu):
    scene = _scene(pkg, "cornell")
    c = _ctx(pkg, make_emu, scene, denoise=1, denoise_temporal=1)
    r = _ctx(pkg, make_emu, scene, denoise_temporal=1)
    for f, st in enumerate([pkg.RESET, pkg.RESET, pkg.CONVERGE, pkg.CONVERGE, pkg.RESET]):
        c.render_frame(scene.camera, st)
        r.render_frame(scene.camera, st)
        out, raw = c.framebuffer(), r.framebuffer()
        n = c.read_denoise_history()["length"]
        spatial = np.array_equal(_bits(out), _bits(c.denoise_image(raw)))
        if f in (0, 2, 3):  # the first frame, CONVERGE frames (the accumulator already holds P's samples)
            assert spatial and (n[n > 0] == 1).all(), f
        else:  # a RESET after a presented frame: the history is used
            assert not spatial and n.max() == 2, f


def test_reset_frames_are_decorrelated(pkg, make_emu):
    scene = _scene(pkg, "cornell")
    for temporal in (0, 1):
        c = _ctx(pkg, make_emu, scene, denoise_temporal=temporal)
        c.render_frame(scene.camera, pkg.RESET)
        a = c.framebuffer()
        c.render_frame(scene.camera, pkg.RESET)
        b = c.framebuffer()
        assert np.array_equal(_bits(a), _bits(b)) == (temporal == 0), temporal
        if temporal:
            # a re-init restarts the origin: the first frame again
            c.init(W, H)
            c.render_frame(scene.camera, pkg.RESET)
            assert np.array_equal(_bits(c.framebuffer()), _bits(a))


def test_a_moving_instance_restarts_its_history(pkg, make_emu):
    scene = _scene(pkg, "cornell")
    mover = 2  # the second box (an instance of the box mesh; instance 1 stays)
    c = _ctx(pkg, make_emu, scene, denoise=1, denoise_temporal=1)
    t0 = np.array(scene.instances[mover]["transform"], np.float64)
    prev = None
    for f in range(4):
        t = t0.copy()
        t[0, 3] += 0.05 * f
        if f:
            c.set_instance(mover, scene.instances[mover]["mesh"], t)
            c.update()
        c.render_frame(scene.camera, pkg.RESET)
        c.framebuffer()
        h = c.read_denoise_history()
        g = c.read_denoise_guides()
        ids = M.centre_ids(c, scene.camera, g["valid"])
        moving, still = ids == mover, ids == 1
        assert moving.sum() > 50 and still.sum() > 50
        if f:
            assert (h["length"][moving] == 1).all(), f
            assert (h["length"][still] == f + 1).mean() > 0.95, f
            # ... exactly what the model says with that instance marked as changed
            changed = np.zeros(len(scene.instances), bool)
            changed[mover] = True
            _, st = M.temporal(c.framebuffer(), g, ids, M.camera_of(c, scene.camera), prev, changed)
            np.testing.assert_allclose(h["length"], st["length"], rtol=1e-4, atol=1e-3)
        prev = dict(M.temporal(np.zeros((H, W, 4), np.float32), g, ids, M.camera_of(c, scene.camera))[1],
                    history=h["history"], moments=h["moments"], length=h["length"])


@pytest.mark.parametrize("order", ["scene_setting_init", "setting_scene_init", "init_scene_setting"])
def test_any_call_order_gives_the_stage_its_instance_table(pkg, make_emu, order):
    """The per-instance table of the instance test exists on the device whatever the order of the scene's rfwhip_update, the
    setting and rfwhip_init (the table does not depend on the size): the same frames as the usual order."""
    scene = _scene(pkg, "cornell")

    def build(steps):
        c = make_emu()
        for step in steps:
            if step == "scene":
                scene.upload(c)
            elif step == "setting":
                for k, v in (("integrator", "pt"), ("spp", 1), ("denoise", 1), ("denoise_temporal", 1)):
                    c.set_setting(k, v)
            else:
                c.init(W, H)
        return c
    ref = build(["init", "scene", "setting"])
    c = build(order.split("_"))
    for f in range(3):
        cam = M.panned(scene.camera, 0.03 * f)
        ref.render_frame(cam, pkg.RESET)
        c.render_frame(cam, pkg.RESET)
        out = c.framebuffer()
        assert np.array_equal(_bits(out), _bits(ref.framebuffer())), f
    n = c.read_denoise_history()["length"]
    assert n.max() > 2.5  # (the history was used: three frames)


@pytest.mark.parametrize("n", [2, 3])
def test_groups_equal_one_context_over_a_moving_sequence(pkg, make_emu, emu_lib, n):
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    settings = {"integrator": "pt", "spp": 1, "max_depth": 2, "denoise": 1, "denoise_temporal": 1}
    ref = make_emu()
    ref.init(70, 51)
    scene.upload(ref)
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0] * n, "peer")
    g.init(70, 51)
    scene.upload(g)
    for k, v in settings.items():
        ref.set_setting(k, v), g.set_setting(k, v)
    for f in range(5):
        cam = M.panned(scene.camera, 0.4 * f)
        ref.render_frame(cam, pkg.RESET)
        g.render_frame(cam, pkg.RESET)
        want = ref.framebuffer()
        assert np.array_equal(_bits(g.framebuffer()), _bits(want)), f
    assert ref.read_denoise_history()["length"].max() >= 4
    g.destroy()


def test_settings_keys_and_clearing(pkg, make_emu, emu_lib):
    c = make_emu()
    c.init(16, 16)
    keys = list(c.get_settings())
    assert "denoise_temporal" in keys and "denoise_alpha" in keys
    assert c.get_setting("denoise_temporal") == "0" and float(c.get_setting("denoise_alpha")) == pytest.approx(0.2)
    for k, v in [("denoise_temporal", "2"), ("denoise_temporal", ""), ("denoise_alpha", "0"), ("denoise_alpha", "1.5"),
                 ("denoise_alpha", "-0.1"), ("denoise_alpha", "x"), ("denoise_alpha", "nan")]:
        with pytest.raises(RuntimeError):
            c.set_setting(k, v)
    c.set_setting("denoise_alpha", "1")
    assert float(c.get_setting("denoise_alpha")) == 1.0
    # the history is cleared by a re-init and by turning denoise or denoise_temporal on
    scene = _scene(pkg, "cornell")
    c = _ctx(pkg, make_emu, scene, denoise=1, denoise_temporal=1)
    r = _ctx(pkg, make_emu, scene, denoise_temporal=1)

    def frame():
        c.render_frame(scene.camera, pkg.RESET)
        r.render_frame(scene.camera, pkg.RESET)
        out = c.framebuffer()
        return out, np.array_equal(_bits(out), _bits(c.denoise_image(r.framebuffer())))
    assert frame()[1] and not frame()[1]
    for clear in (lambda: (c.set_setting("denoise_temporal", 0), c.set_setting("denoise_temporal", 1)),
                  lambda: (c.set_setting("denoise", 0), c.set_setting("denoise", 1)),
                  lambda: (c.init(W, H), r.init(W, H))):
        clear()
        assert frame()[1]  # fresh
        assert not frame()[1]
    with pytest.raises(RuntimeError):
        c.set_setting("denoise_temporal", 0)
        c.read_denoise_history()


def _mse(a, b):
    return float(((a[..., :3].astype(np.float64) - b[..., :3]) ** 2).mean())


# MSE against a converged render after 8 RESET frames, spatial-only / temporal.  Measured on the emulation: 1.75 (static camera),
# 1.81 (pan) — DESIGN.md §10; the thresholds keep about half of the gain over 1
QUALITY = {"static": 1.4, "pan": 1.4}


@pytest.mark.parametrize("motion", ["static", "pan"])
def test_quality_against_a_converged_render(pkg, make_emu, motion):
    scene = pkg.scenes.cornell(64, 64, geometric_emitter=True)
    cams = [M.panned(scene.camera, (0.02 * k) if motion == "pan" else 0.0) for k in range(8)]
    ref = _ctx(pkg, make_emu, scene, 64, 64, spp=1024)
    ref.render_frame(cams[-1], pkg.RESET)
    ref = ref.framebuffer()
    t = _ctx(pkg, make_emu, scene, 64, 64, denoise=1, denoise_temporal=1)
    s = _ctx(pkg, make_emu, scene, 64, 64, denoise=1, denoise_temporal=1)
    for cam in cams:
        t.render_frame(cam, pkg.RESET)
        s.render_frame(cam, pkg.RESET)
        temporal = t.framebuffer()  # (every frame presented: the history follows)
    spatial = s.denoise_image(_raw(pkg, make_emu, scene, cams))
    gain = _mse(spatial, ref) / _mse(temporal, ref)
    print("temporal quality %s: MSE spatial %.5g temporal %.5g gain %.2f" % (motion, _mse(spatial, ref), _mse(temporal, ref), gain))
    assert gain >= QUALITY[motion]


def _raw(pkg, make_emu, scene, cams):
    r = _ctx(pkg, make_emu, scene, 64, 64, denoise_temporal=1)
    for cam in cams:
        r.render_frame(cam, pkg.RESET)
    return r.framebuffer()
