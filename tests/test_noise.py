"""The noise estimate (include/rfwhip.h, rfwhip_get_noise; csrc/noise.h), CPU tier: the host-emulation build runs the work items
of k_resolve_noise, k_noise_merge, k_noise_tiles and k_noise_final in plain loops.  Held to the float64 model of
tests/noise_model.py within the bounds counted there — not to the HIP build — and to the unchanged framebuffer."""
import ctypes

import numpy as np
import pytest

import noise_model as nm

SPPS = (1, 3, 8, 64)


def setup(pkg, c, spp, noise, w=96, h=64, **settings):
    scene = pkg.scenes.cornell(w, h)
    c.init(w, h)
    scene.upload(c)
    for k, v in dict(settings, integrator="pt", spp=spp, noise_estimate=noise).items():
        c.set_setting(k, v)
    return scene


def frames(pkg, c, scene, calls):
    """RESET then calls - 1 CONVERGE calls; the framebuffer after every call."""
    out = []
    for k in range(calls):
        c.render_frame(scene.camera, pkg.CONVERGE if k else pkg.RESET)
        out.append(c.framebuffer())
    return out


def check_images_untouched(pkg, make, spp):
    """RESET + three CONVERGE calls: the framebuffer is bit-equal with noise_estimate 0 and 1, sumY / n is the framebuffer's
    luminance within rounding, and toggling the setting between RESETs leaves no stale moments."""
    off, on = make(), make()
    s_off, s_on = setup(pkg, off, spp, 0), setup(pkg, on, spp, 1)
    f_off, f_on = frames(pkg, off, s_off, 4), frames(pkg, on, s_on, 4)
    for a, b in zip(f_off, f_on):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    n = 4 * spp
    sumY, m2 = on.read_noise_moments()
    want = nm.luma(f_on[-1][..., :3])
    # two float32 sums of the same n samples: per channel (2 n additions: radiance and connection records) and scaled by 1 / n
    # (2 roundings), against luminance first (3 roundings) and then n additions
    tol = (nm.gamma(2 * n) + nm.gamma(n + 3) + 2 * nm.U) * nm.SLACK * want + 1e-30
    err = np.abs(sumY / np.float64(n) - want)
    print("spp %d: max |sumY / n - luma(F)| / tol = %.3g" % (spp, float((err / tol).max())))
    assert (err <= tol).all() and (m2 >= 0).all() and on.get_noise()["samples"] == n
    # off: the moments are gone, and a query says so; on again without a RESET: still refused; RESET: the moments of that call alone
    first = None
    for round_ in range(2):
        on.set_setting("noise_estimate", 0)
        on.render_frame(s_on.camera, pkg.CONVERGE)
        with pytest.raises(RuntimeError, match="noise_estimate is off"):
            on.get_noise()
        on.set_setting("noise_estimate", 1)
        on.render_frame(s_on.camera, pkg.CONVERGE)
        with pytest.raises(RuntimeError, match="RESET first"):
            on.read_noise_moments()
        on.render_frame(s_on.camera, pkg.RESET)
        again = on.read_noise_moments()
        assert np.array_equal(on.framebuffer().view(np.uint32), f_off[0].view(np.uint32))
        if first is None:
            first = again
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    if spp == 1:
        assert (first[1] == 0).all()  # one sample: no spread


def check_end_to_end(pkg, make):
    """spp 1, RESET + 6 CONVERGE calls: the samples are k F_k - (k - 1) F_(k-1) of the successive framebuffers, in float64."""
    c = make()
    scene = setup(pkg, c, 1, 1)
    F = [f[..., :3].astype(np.float64).reshape(-1, 3) for f in frames(pkg, c, scene, 7)]
    steps, y_err = [], []
    for k in range(1, len(F) + 1):
        cur, prev = k * F[k - 1], (k - 1) * F[k - 2] if k > 1 else 0.0 * F[0]
        steps.append(nm.luma(cur - prev)[:, None])
        # what the difference carries: acc_k = fl(fl(acc_(k-1) + rad) + rad_nee) (2 u acc_k), the sample's own fl(rad + rad_nee)
        # (u), and F = fl(acc fl(1 / k)) on both framebuffers (2 u each): at most 8 u acc_k per channel
        y_err.append(nm.luma(8 * nm.U * np.maximum(cur, prev))[:, None])
    ws, wm, es, em = nm.moment_bounds(steps, y_err)
    sumY, m2 = (a.astype(np.float64).ravel() for a in c.read_noise_moments())
    print("end to end: sumY err / bound %.3g, M2 err / bound %.3g, median M2 bound / M2 %.3g" %
          (float((np.abs(sumY - ws) / es).max()), float((np.abs(m2 - wm) / em).max()), float(np.median(em[wm > 0] / wm[wm > 0]))))
    assert (np.abs(sumY - ws) <= es).all() and (np.abs(m2 - wm) <= em).all()
    assert np.median(em[wm > 0] / wm[wm > 0]) < 1e-3  # (the bound says something)
    # the metric on the rendered moments: the map and the stats are the model's on the device's own moments
    n = len(F)
    st, e = c.get_noise(), c.read_noise_map()
    s32, m32 = c.read_noise_moments()
    want = nm.error(s32, m32, n, float(c.get_setting("noise_floor")))
    assert (np.abs(e - want) <= nm.E_REL * want).all()
    t = c.read_noise_tiles()
    assert t.shape == (8, 3) and int(t["pixels"].sum()) == 96 * 64 == st["pixels"] and st["samples"] == n
    assert st["converged"] == int(t["converged"].sum()) == int((e <= np.float32(st["threshold"])).sum())
    assert st["max_error"] == e.max() and abs(st["mean_error"] - e.astype(np.float64).mean()) <= nm.gamma(256) * st["mean_error"]
    assert c.get_noise() == st and c.read_noise_map().tobytes() == e.tobytes()


def check_state_errors(pkg, make, lib):
    c = make()
    scene = setup(pkg, c, 1, 0)
    c.render_frame(scene.camera, pkg.RESET)
    c.render_frame(scene.camera, pkg.CONVERGE)
    for call in (c.get_noise, c.read_noise_map, c.read_noise_tiles, c.read_noise_moments):
        with pytest.raises(RuntimeError, match="noise_estimate is off"):
            call()
    c.set_setting("noise_estimate", 1)
    c.render_frame(scene.camera, pkg.RESET)
    with pytest.raises(RuntimeError, match="1 samples per pixel, the estimate needs 2"):
        c.get_noise()
    c.render_frame(scene.camera, pkg.CONVERGE)
    assert c.get_noise()["samples"] == 2
    # null pointers and a capacity too small, through the C ABI
    vp = ctypes.c_void_p
    INVALID = 1
    buf, u = (ctypes.c_float * (96 * 64 * 4))(), ctypes.c_uint32()
    st = pkg.abi.NoiseStats()
    for name, args in (("get_noise", [None]), ("read_noise_map", [vp(None)]),
                       ("read_noise_tiles", [vp(None), ctypes.c_size_t(24), ctypes.byref(u), ctypes.byref(u)]),
                       ("read_noise_tiles", [buf, ctypes.c_size_t(24), None, ctypes.byref(u)]),
                       ("read_noise_tiles", [buf, ctypes.c_size_t(23), ctypes.byref(u), ctypes.byref(u)]),
                       ("read_noise_moments", [buf, vp(None)]),
                       ("noise_merge", [ctypes.c_size_t(1), 0, buf, buf, 1, vp(None), buf, buf]),
                       ("noise_merge", [ctypes.c_size_t(0), 0, buf, buf, 1, buf, buf, buf]),
                       ("noise_image", [4, 4, 2, buf, vp(None), ctypes.byref(st), buf, vp(None)]),
                       ("noise_image", [4, 4, 2, buf, buf, None, buf, vp(None)]),
                       ("noise_image", [0, 4, 2, buf, buf, ctypes.byref(st), buf, vp(None)])):
        assert c._fn(name)(c._ctx, *args) == INVALID, (name, args)
    assert c._fn("noise_image")(c._ctx, 4, 4, 1, buf, buf, ctypes.byref(st), buf, vp(None)) not in (0, INVALID)  # n < 2: a state error
    assert "needs 2" in c._fn("last_error")().decode()
    assert c._fn("read_noise_tiles")(c._ctx, buf, ctypes.c_size_t(24), ctypes.byref(u), ctypes.byref(u)) == 0
    for key in ("noise_floor", "noise_threshold"):
        for bad in ("0", "-1", "nan", "inf", "", "x"):
            with pytest.raises(RuntimeError, match="finite number > 0"):
                c.set_setting(key, bad)
    with pytest.raises(RuntimeError, match='"0" or "1"'):
        c.set_setting("noise_estimate", "2")
    assert (c.get_setting("noise_estimate"), c.get_setting("noise_floor"), c.get_setting("noise_threshold")) == ("1", "0.01", "0.05")
    assert len(c.get_settings()) == 31 and not any(k.startswith("noise") for k in c.get_settings())


def check_render_until(pkg, make):
    c = make()
    scene = setup(pkg, c, 2, 0)
    st = c.render_until(scene.camera, threshold=1e-6, max_samples=8)  # unreachable: the cap
    assert st["samples"] == 8 and st["converged"] < st["pixels"] and c.get_setting("noise_estimate") == "1"
    st = c.render_until(scene.camera, threshold=1e3, max_samples=64)  # generous: the first look
    assert st["samples"] == 2 and st["converged"] == st["pixels"]
    st = c.render_until(scene.camera, threshold=1e3, max_samples=64, check_every=3)  # ... which comes after three calls
    assert st["samples"] == 6
    # the 1 / sqrt(n) law: four times the samples, half the error (the band is wide: the estimate itself is noisy at 96 x 64)
    c.set_setting("spp", 8)
    e1 = c.render_until(scene.camera, threshold=1e-6, max_samples=16)
    e4 = c.render_until(scene.camera, threshold=1e-6, max_samples=64)
    assert (e1["samples"], e4["samples"]) == (16, 64)
    print("mean error at 16 / 64 samples: %.4g / %.4g, ratio %.3f" % (e1["mean_error"], e4["mean_error"], e4["mean_error"] / e1["mean_error"]))
    assert 0.35 <= e4["mean_error"] / e1["mean_error"] <= 0.7


@pytest.mark.parametrize("spp", SPPS)
def test_images_untouched(pkg, make_emu, spp):
    check_images_untouched(pkg, make_emu, spp)


def test_step_update_on_given_samples(make_emu):
    nm.merge_cases(make_emu())


def test_end_to_end(pkg, make_emu):
    check_end_to_end(pkg, make_emu)


@pytest.mark.parametrize("size", nm.SIZES, ids=lambda s: "%dx%d" % s)
def test_metric_on_given_moments(make_emu, size):
    c = make_emu()
    for kind in nm.KINDS:
        nm.check_metric(c, kind, *size)
    nm.check_metric(c, "straddle", *size, floor=0.1, threshold=0.2)


@pytest.mark.parametrize("n", [2, 3])
def test_group_equals_the_single_context(pkg, make_emu, emu_lib, n):
    one = make_emu()
    scene = setup(pkg, one, 3, 1, 70, 51)
    frames(pkg, one, scene, 2)
    want = one.get_noise()
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0] * n, "peer")
    g.init(70, 51)
    scene.upload(g)
    for k, v in dict(integrator="pt", spp=3, noise_estimate=1).items():
        g.set_setting(k, v)
    g.render_frame(scene.camera, pkg.RESET)
    g.render_frame(scene.camera, pkg.CONVERGE)
    got = g.get_noise()
    assert np.array_equal(g.framebuffer(), one.framebuffer())
    g.destroy()
    for k in ("samples", "pixels", "converged", "max_error", "threshold"):
        assert got[k] == want[k], k
    assert abs(got["mean_error"] - want["mean_error"]) <= nm.gamma(256) * want["mean_error"]


def test_state_errors(pkg, make_emu, emu_lib):
    check_state_errors(pkg, make_emu, emu_lib)


def test_render_until(pkg, make_emu):
    check_render_until(pkg, make_emu)
