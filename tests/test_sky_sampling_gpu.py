"""Sky sampling on the MI355X (k_shade_pt_sky, the sky cases of k_kat): the device against the host emulation of the same sources
(bit for bit under the strict build), scheduling independence, and the estimator on the 1080p bench terrain."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from test_sky_sampling import _kat_sample, _random_sky

pytestmark = pytest.mark.gpu

STRICT_FLAGS = ("-DRT_STRICT_MATH", "-ffp-contract=off")


@pytest.fixture(scope="module")
def emu_strict_lib():
    import build_emu
    return ctypes.CDLL(build_emu.build(defines=STRICT_FLAGS, tag="_strict"))


def _strict_hip():
    so = os.path.join(ROOT, "tests", "_strict", "librfwhip_strict.so")
    assert os.path.exists(so), "build it with __graft_entry__.build() (build.py: build_strict)"
    return ctypes.CDLL(so)


def _upload(pkg, c, scene, w, h, settings):
    c.init(w, h)
    scene.upload(c)
    for k, v in settings.items():
        c.set_setting(k, v)
    return c


def _render(pkg, c, scene, frames=1):
    for f in range(frames):
        c.render_frame(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
    st = c.get_stats()
    return c.framebuffer(), (st.primaryCount, st.secondaryCount, st.deepCount, st.shadowCount)


def _kat_scene(pkg, sky):
    s = pkg.scenes.cornell(64, 48, geometric_emitter=True)
    s.sky = sky
    return s


@pytest.mark.parametrize("strict", [False, True])
def test_device_kat_equals_the_emulation(pkg, make_hip, make_emu, emu_strict_lib, strict):
    """RFWHIP_KAT_SKY_SAMPLE / _PDF on the device: bit-equal to the emulation under the strict build; within the KAT tolerances
    (directions 2e-6, densities 1e-5 relative, the texel the same but where rounding moves a direction across an edge) otherwise."""
    sky = _random_sky(3)
    scene = _kat_scene(pkg, sky)
    settings = {"integrator": "pt", "sky_sampling": 1}
    if strict:
        dev = _upload(pkg, pkg._binding.CoreBinding(_strict_hip(), "rfwhip_", 0, 0, 1), scene, 64, 48, settings)
        emu = _upload(pkg, pkg._binding.CoreBinding(emu_strict_lib, "rfwhip_", 0, 0, 1), scene, 64, 48, settings)
    else:
        dev = _upload(pkg, make_hip(), scene, 64, 48, settings)
        emu = _upload(pkg, make_emu(), scene, 64, 48, settings)
    rec, a, ta = _kat_sample(dev, 200_000, seed=17)
    _, b, tb = _kat_sample(emu, 200_000, seed=17)
    rq = np.zeros_like(rec)
    rq[:, :3] = b[:, :3]
    pa, pb = dev.kat("sky_pdf", rq), emu.kat("sky_pdf", rq)
    if strict:
        assert np.array_equal(a, b) and np.array_equal(pa, pb)
        return
    assert np.array_equal(ta, tb)  # (the table and the alias decision are integer / exact float work)
    np.testing.assert_allclose(a[:, :3], b[:, :3], atol=2e-6)
    np.testing.assert_allclose(a[:, 3:7], b[:, 3:7], rtol=1e-5)
    same = pa[:, 7].view(np.int32) == pb[:, 7].view(np.int32)
    assert (~same).mean() <= 1e-4
    np.testing.assert_allclose(pa[same, 3:7], pb[same, 3:7], rtol=1e-5)


@pytest.mark.parametrize("scene_name", ["cornell", "cards", "bench_terrain"])
def test_strict_hip_equals_strict_emulation_bit_for_bit(pkg, emu_strict_lib, scene_name):
    w, h = 480, 270
    if scene_name == "bench_terrain":
        scene = pkg.scenes.terrain(n=708, width=w, height_px=h)
    elif scene_name == "cornell":
        scene = pkg.scenes.cornell(w, h, geometric_emitter=True)
        scene.set_test_sky(256, 128)
    else:
        scene = pkg.scenes.cards(w, h)
        scene.set_test_sky(256, 128)
    settings = {"integrator": "pt", "spp": 8, "max_depth": 2, "sky_sampling": 1}
    hip = _upload(pkg, pkg._binding.CoreBinding(_strict_hip(), "rfwhip_", 0, 0, 1), scene, w, h, settings)
    emu = _upload(pkg, pkg._binding.CoreBinding(emu_strict_lib, "rfwhip_", 0, 0, 1), scene, w, h, settings)
    a, b = _render(pkg, hip, scene), _render(pkg, emu, scene)
    differing = int((np.abs(a[0] - b[0]).max(-1) > 0).sum())
    print("%s: strict HIP vs strict emulation with sky_sampling=1: %d of %d pixels differ; counts %s / %s" % (scene_name, differing, w * h, a[1], b[1]))
    assert a[1] == b[1] and differing == 0


def test_scheduling_does_not_change_the_image(pkg, make_hip):
    """spp 16 on the 480 x 270 bench terrain (the packet form of the depth-0 connection wave is active): fuse, shadow_packets,
    shadow_side, ring (pipelined calls) and streams give the same image and ray counts with sky_sampling=1."""
    w, h = 480, 270
    scene = pkg.scenes.terrain(n=708, width=w, height_px=h)
    base = {"integrator": "pt", "spp": 16, "max_depth": 2, "sky_sampling": 1}
    ref = None
    variants = [{}, {"fuse": 0}, {"fuse": 1}, {"shadow_packets": 0}, {"shadow_packets": 1}, {"shadow_side": 0},
                {"shadow_side": 1}, {"streams": 1}, {"streams": 4}]
    c = _upload(pkg, make_hip(), scene, w, h, base)
    assert c.get_setting("sky") == "1"
    for v in variants:
        for k, x in base.items():
            c.set_setting(k, x)
        for k, x in v.items():
            c.set_setting(k, x)
        img = _render(pkg, c, scene)
        if ref is None:
            ref = img
        assert img[1] == ref[1] and np.array_equal(img[0], ref[0]), v
    for ring in (1, 2, 4):  # pipelined: frames in flight on the ring of buffer sets
        c.set_setting("ring", ring)
        for f in range(3):
            c.render_async(scene.camera, pkg.RESET)
        c.wait()
        st = c.get_stats()
        assert np.array_equal(c.framebuffer(), ref[0]), ring
        assert (st.primaryCount, st.secondaryCount, st.deepCount, st.shadowCount) == ref[1], ring
    # and the default kernels give another image
    c.set_setting("sky_sampling", 0)
    assert not np.array_equal(_render(pkg, c, scene)[0], ref[0])


def test_bench_terrain_unbiased_and_less_noisy(pkg, make_hip):
    """The 1080p bench terrain without its lights (the sky's estimator alone; with lights the reference's light term moves with
    p): tile means (40 x 40 pixels) of 16 frames of 16 spp show no systematic difference (mean z, share of |z| > 4, image mean), and
    the per-pixel variance drops."""
    w, h = 1920, 1080
    scene = pkg.scenes.terrain(n=708, width=w, height_px=h, lights=False)
    scene.camera.clampValue = 1e9
    t, n = 40, 16
    tiles, var = [], []
    for ss in (0, 1):
        c = _upload(pkg, make_hip(), scene, w, h, {"integrator": "pt", "spp": 16, "max_depth": 2, "sky_sampling": ss})
        tl, s1, s2, prev = [], 0.0, 0.0, None
        for k in range(1, n + 1):
            c.render_frame(scene.camera, pkg.RESET if k == 1 else pkg.CONVERGE)
            m = c.framebuffer()[..., :3].astype(np.float64)
            f = m if prev is None else k * m - (k - 1) * prev  # (this frame's own samples)
            prev = m
            tl.append(f.reshape(h // t, t, w // t, t, 3).mean((1, 3)))
            s1, s2 = s1 + f, s2 + f * f
        tiles.append(np.stack(tl))
        var.append(float(((s2 - s1 * s1 / n) / (n - 1)).mean()))
    ta, tb = tiles
    z = (ta.mean(0) - tb.mean(0)) / np.sqrt(ta.var(0, ddof=1) / n + tb.var(0, ddof=1) / n + 1e-30)
    ratio = var[0] / var[1]
    rel = abs(tb.mean() / ta.mean() - 1.0)
    tail = float((np.abs(z) > 4.0).mean())
    print("1080p terrain, sky only: z over %d tile channels: mean %.3f, max |z| %.2f, share beyond 4: %.4f; image means %.5f / %.5f "
          "(%.2e relative); per-pixel variance ratio %.2f" % (z.size, z.mean(), np.abs(z).max(), tail, ta.mean(), tb.mean(), rel, ratio))
    # (the default estimator is heavy-tailed here — the sun, radiance 20, found by a few bounce rays — and 16 frames estimate its
    # variance poorly: the test is for a SYSTEMATIC difference, the mean z over all tiles and the image mean)
    assert abs(z.mean()) <= 0.15 and tail <= 5e-3 and rel <= 5e-3 and ratio >= 2.0
