"""Sky sampling (settings sky_sampling / sky_pick, include/rfwhip.h; csrc/sky_sampling.h, rt_core.h sky_sample / sky_eval and
pt_shade<TEX, true>), CPU tier: the host-emulation build runs the same shade work items as k_shade_pt_sky.  The distribution is
held to the numpy model of tests/sky_sampling_model.py through the known-answer hooks; the estimator to the default one (same
expectation, less noise); the switch to the default kernels bit for bit wherever p is 0."""

import numpy as np
import pytest

import sky_sampling_model as model

W, H = 64, 48


# ---------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------
def _open_scene(pkg, lights=False, w=W, h=H):
    """A diffuse ground with two boxes under the sky (opaque, non-transmissive materials: the BSDF samples what bsdf_pdf
    describes); lights=True adds an emissive quad (an area light) and a point light."""
    sc = pkg.scenes
    s = sc.Scene()
    ground = s.add_material(color=(0.6, 0.55, 0.5), roughness=1.0)
    boxm = s.add_material(color=(0.7, 0.7, 0.75), roughness=0.6)
    corners = np.array([[-4, 0, -4], [4, 0, -4], [-4, 0, 4], [4, 0, 4]], np.float32)
    s.add_instance(s.add_mesh(corners, np.array([[0, 2, 1], [1, 2, 3]], np.uint32), material=ground))
    for lo, hi in (((-1.5, 0.0, -0.5), (-0.5, 1.2, 0.5)), ((0.4, 0.0, 0.2), (1.4, 0.7, 1.2))):
        v, i = sc._box(lo, hi)
        s.add_instance(s.add_mesh(v, i, material=boxm))
    if lights:
        em = s.add_material(color=(6.0, 5.0, 4.0), roughness=1.0)
        s.add_instance(s.add_mesh(sc.quad((0.0, -1.0, 0.0), (0.3, 2.5, -0.6), 0.8, 0.8), None, material=em))
        s.update_area_lights()
        s.add_point_light((-1.0, 2.0, -1.5), (4.0, 4.0, 3.5))
    s.set_test_sky(64, 32)
    cam = sc.Camera(aperture=0.0, FOV=50.0, focalDistance=5.0)
    cam.look_at((0.0, 2.2, -4.0), (0.0, 0.3, 0.0))
    cam.resize(w, h)
    cam.clampValue = 1e9  # (clamping is not linear: the statistical tests keep every contribution)
    s.camera = cam
    s.wh = (w, h)
    return s


def _random_sky(seed, w=24, h=12):
    rng = np.random.default_rng(seed)
    px = (rng.random((h, w, 3)) ** 4 * 5).astype(np.float32)
    px[:, : w // 3] *= 0.05  # asymmetric
    px[2, 3] = (20, 30, 10)  # a bright texel
    px[5, 7] = (-1, -1, -1)  # weighs 0
    px[6, 9] = (np.nan, 1, 1)  # weighs 0
    px[h - 1] = 0  # a black row
    return px.reshape(-1, 3), w, h


def _ctx(pkg, make_emu, scene, spp=1, upload_sky=True, **settings):
    c = make_emu()
    c.init(*scene.wh)
    if upload_sky:
        scene.upload(c)
    else:  # Scene.upload without set_sky: a context that never had a sky
        c.set_textures(scene.textures)
        mats, ids = pkg.scenes.pack_materials(scene.host_materials, scene.textures)
        c.set_materials(mats, ids)
        for i, m in enumerate(scene.meshes):
            c.set_mesh(i, m["vertices"], m["triangles"], m["indices"])
        for i, inst in enumerate(scene.instances):
            c.set_instance(i, inst["mesh"], inst["transform"])
        c.set_lights(*scene.light_arrays())
        c.update()
    c.set_setting("integrator", "pt")
    c.set_setting("spp", spp)
    for k, v in settings.items():
        c.set_setting(k, v)
    return c


def _render(pkg, c, scene, frames=1):
    for f in range(frames):
        c.render_frame(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
    return c.framebuffer()


def _frames(pkg, c, scene, frames):
    """Per-frame images from the running means of CONVERGE frames: f_k = k M_k - (k - 1) M_{k-1}."""
    out, prev = [], None
    for k in range(1, frames + 1):
        c.render_frame(scene.camera, pkg.RESET if k == 1 else pkg.CONVERGE)
        m = c.framebuffer()[..., :3].astype(np.float64)
        out.append(m if prev is None else k * m - (k - 1) * prev)
        prev = m
    return np.stack(out)


def _tile_z(fa, fb, t=8):
    """z-scores of the differences of 8 x 8 tile means of two stacks of independent frames (variance from the frames)."""
    def tiles(f):
        k, h, w, c = f.shape
        return f[:, : h // t * t, : w // t * t].reshape(k, h // t, t, w // t, t, c).mean((2, 4))
    ta, tb = tiles(fa), tiles(fb)
    va, vb = ta.var(0, ddof=1) / len(ta), tb.var(0, ddof=1) / len(tb)
    d = ta.mean(0) - tb.mean(0)
    return d / np.sqrt(va + vb + 1e-30), ta.mean(0), tb.mean(0)


# ---------------------------------------------------------------------------------------------------------------------------
# settings
# ---------------------------------------------------------------------------------------------------------------------------
def test_settings_defaults_validation_and_keys(pkg, make_emu):
    c = make_emu()
    assert c.get_setting("sky_sampling") == "0"
    assert c.get_setting("sky_pick") == "-1"
    assert c.get_setting("sky") == "0"
    keys = list(c.get_settings())
    assert "sky_sampling" in keys and "sky_pick" in keys
    for bad in ("2", "-1", "yes", ""):
        with pytest.raises(Exception):
            c.set_setting("sky_sampling", bad)
    for bad in ("1.5", "-0.5", "-2", "x", "", "nan"):
        with pytest.raises(Exception):
            c.set_setting("sky_pick", bad)
    c.set_setting("sky_pick", "0.25")
    assert c.get_setting("sky_pick") == "0.25"
    c.set_setting("sky_pick", "-1")
    assert c.get_setting("sky_pick") == "-1"
    c.set_setting("sky_sampling", "1")
    assert c.get_setting("sky_sampling") == "1"
    assert c.get_setting("sky") == "0"  # (no sky yet)


def test_plugin_lists_the_key():
    import os
    src = open(os.path.join(os.path.dirname(__file__), "..", "rendering-fw_amd", "csrc", "plugin", "HipRT.cpp")).read()
    line = next(l for l in src.splitlines() if "s.settingKeys" in l)
    assert '"sky_sampling"' in line


def test_sky_key_follows_the_scene(pkg, make_emu):
    scene = _open_scene(pkg)
    c = _ctx(pkg, make_emu, scene, sky_sampling=1)
    assert c.get_setting("sky") == "1"
    c.set_setting("sky_pick", 0)
    assert c.get_setting("sky") == "0"
    c.set_setting("sky_pick", -1)
    assert c.get_setting("sky") == "1"
    c.set_setting("sky_sampling", 0)
    assert c.get_setting("sky") == "0"


# ---------------------------------------------------------------------------------------------------------------------------
# p = 0: the default kernels, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["black_sky", "no_sky", "pick0"])
def test_p_zero_is_bit_identical_to_the_default(pkg, make_emu, case):
    scene = _open_scene(pkg, lights=True)
    if case == "black_sky":
        scene.sky = (np.zeros((16 * 8, 3), np.float32), 16, 8)
    extra = {"sky_pick": 0} if case == "pick0" else {}
    up = case != "no_sky"
    ref = _render(pkg, _ctx(pkg, make_emu, scene, spp=2, upload_sky=up, max_depth=3), scene, frames=2)
    c = _ctx(pkg, make_emu, scene, spp=2, upload_sky=up, max_depth=3, sky_sampling=1, **extra)
    assert c.get_setting("sky") == "0"
    assert np.array_equal(_render(pkg, c, scene, frames=2), ref)


def test_sky_variant_changes_the_image(pkg, make_emu):
    scene = _open_scene(pkg, lights=True)
    a = _render(pkg, _ctx(pkg, make_emu, scene, spp=2), scene)
    b = _render(pkg, _ctx(pkg, make_emu, scene, spp=2, sky_sampling=1), scene)
    assert np.isfinite(b).all() and not np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# the distribution, through the known-answer hooks
# ---------------------------------------------------------------------------------------------------------------------------
def _kat_ctx(pkg, make_emu, sky):
    scene = _open_scene(pkg)
    scene.sky = sky
    return _ctx(pkg, make_emu, scene, sky_sampling=1)


def _kat_sample(c, n, seed):
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 24), np.float32)
    rec[:, :5] = rng.random((n, 5), np.float32)
    out = c.kat("sky_sample", rec)
    return rec, out, out[:, 7].view(np.uint32).astype(np.int64)


SKIES = {"test_sky": lambda pkg: _open_scene(pkg).sky, "random": lambda pkg: _random_sky(3)}


@pytest.mark.parametrize("sky", sorted(SKIES))
def test_pdf_integrates_to_one_and_matches_the_model(pkg, make_emu, sky):
    px, w, h = SKIES[sky](pkg)
    c = _kat_ctx(pkg, make_emu, (px, w, h))
    D = model.texel_centre_directions(w, h)
    rec = np.zeros((len(D), 24), np.float32)
    rec[:, :3] = D
    out = c.kat("sky_pdf", rec)
    texel = out[:, 7].view(np.int32)
    assert np.array_equal(texel, np.arange(w * h))
    omega = np.broadcast_to(model.solid_angles(w, h), (h, w)).reshape(-1)
    assert abs((out[:, 3].astype(np.float64) * omega).sum() - 1.0) < 1e-5
    np.testing.assert_allclose(out[:, 3], model.pdf(D, px, w, h), rtol=1e-5, atol=0)
    np.testing.assert_array_equal(out[:, 4:7], np.asarray(px, np.float32))  # pt_sky's radiance, bit for bit


@pytest.mark.parametrize("sky", sorted(SKIES))
def test_histogram_matches_the_texel_probabilities(pkg, make_emu, sky):
    px, w, h = SKIES[sky](pkg)
    c = _kat_ctx(pkg, make_emu, (px, w, h))
    n = 1_000_000
    rec, out, texel = _kat_sample(c, n, seed=11)
    P, lum, S = model.distribution(px, w, h)
    P = P.reshape(-1)
    counts = np.bincount(texel, minlength=w * h)
    assert counts[P == 0].sum() == 0, "a texel of weight 0 was drawn"
    e = n * P
    big = e >= 5
    chi2 = (((counts[big] - e[big]) ** 2) / e[big]).sum()
    rest_o, rest_e = counts[~big].sum(), e[~big].sum()
    dof = int(big.sum()) - 1
    if rest_e >= 5:
        chi2 += (rest_o - rest_e) ** 2 / rest_e
        dof += 1
    assert chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)
    # the sample's pdf and radiance are the drawn texel's
    np.testing.assert_allclose(out[:, 3], (lum.reshape(-1) / S)[texel], rtol=1e-5)
    np.testing.assert_array_equal(out[:, 4:7], np.asarray(px, np.float32)[texel])


@pytest.mark.parametrize("sky", sorted(SKIES))
def test_sampled_directions_are_uniform_inside_their_texel(pkg, make_emu, sky):
    px, w, h = SKIES[sky](pkg)
    c = _kat_ctx(pkg, make_emu, (px, w, h))
    rec, out, texel = _kat_sample(c, 200_000, seed=5)
    D = out[:, :3].astype(np.float64)
    assert np.abs(np.linalg.norm(D, axis=1) - 1) .max() < 1e-5
    # the sampled pdf is SKY_PDF of the direction, except for directions that rounding puts across a texel edge
    rq = np.zeros((len(D), 24), np.float32)
    rq[:, :3] = out[:, :3]
    back = c.kat("sky_pdf", rq)
    same = back[:, 7].view(np.int32) == texel
    assert (~same).mean() <= 1e-4
    assert np.array_equal(back[same, 3], out[same, 3])
    # (a, b) recovered from the direction are the numbers that placed it: uniform in (phi, cos theta) inside the texel
    a, b = model.local_coordinates(D, texel, w, h)
    assert np.quantile(np.abs(a - rec[:, 3]), 0.999) < 2e-3
    assert np.quantile(np.abs(b - rec[:, 4]), 0.999) < 2e-3


def test_kat_needs_a_table(pkg, make_emu):
    scene = _open_scene(pkg)
    c = _ctx(pkg, make_emu, scene)
    with pytest.raises(Exception):
        c.kat("sky_pdf", np.zeros((1, 24), np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# the estimator
# ---------------------------------------------------------------------------------------------------------------------------
def _terrain(pkg, lights, sky="gradient", w=48, h=32):
    """The bench scene, small: displaced ground (opaque, non-transmissive materials: the BSDF samples what bsdf_pdf describes)."""
    s = pkg.scenes.terrain(n=24, width=w, height_px=h, lights=lights)
    if sky == "test":
        s.set_test_sky(64, 32)
    else:
        s.set_gradient_sky(256, 128)
    s.camera.clampValue = 1e9  # (clamping is not linear: the statistical tests keep every contribution)
    s.wh = (w, h)
    return s


@pytest.mark.parametrize("max_depth", [1, 2])
def test_unbiased_against_the_default(pkg, make_emu, max_depth):
    """Tile means of sky_sampling=1 agree with the default's within z <= 4 on a sky-only scene; max_depth=2 checks the 1 / s
    factor of the sky's term (s < 1 at the second vertex)."""
    scene = _terrain(pkg, lights=False)
    frames = 24
    fa = _frames(pkg, _ctx(pkg, make_emu, scene, spp=8, max_depth=max_depth), scene, frames)
    fb = _frames(pkg, _ctx(pkg, make_emu, scene, spp=8, max_depth=max_depth, sky_sampling=1), scene, frames)
    z, ma, mb = _tile_z(fa, fb)
    assert np.abs(z).max() <= 4.0, np.abs(z).max()
    assert ma.mean() > 0.1


def test_with_lights_only_the_lights_estimator_moves(pkg, make_emu):
    """Lights and sky at max_depth=1.  The lights' next-event term is the reference's (Kernels.cu:702-755): it divides by
    bsdfPdf + lightPdf pickProb with a light pdf that is not the density the light is sampled with (area lights: divided by
    |radiance|; point lights: a delta light with a BSDF pdf beside it), so its expectation depends on the pick probability and
    with it on p — not a bias of the sky's estimator, and not fixed here.  What holds: the sky's share
    is unbiased (the same scene with the lights' radiance scaled to 0 is test_unbiased_against_the_default's), and the image
    with lights stays within a few per cent of the default's (measured on this scene: -4.1 % of the mean)."""
    scene = _terrain(pkg, lights=True)
    frames = 16
    fa = _frames(pkg, _ctx(pkg, make_emu, scene, spp=8, max_depth=1), scene, frames)
    fb = _frames(pkg, _ctx(pkg, make_emu, scene, spp=8, max_depth=1, sky_sampling=1), scene, frames)
    _, ma, mb = _tile_z(fa, fb)
    assert abs(mb.mean() / ma.mean() - 1.0) < 0.08, (ma.mean(), mb.mean())


def test_noise_drops(pkg, make_emu):
    """Sky-only scene under the test sky (three small 10x patches): MSE against a converged image at equal spp drops by >= 3x.
    Measured on the emulation build: ratio 4.33 (default 4 spp and sky_sampling 4 spp against 512 spp of sky_sampling)."""
    scene = _terrain(pkg, lights=False, sky="test")
    ref = _render(pkg, _ctx(pkg, make_emu, scene, spp=64, max_depth=2, sky_sampling=1), scene, frames=8)[..., :3]
    a = _render(pkg, _ctx(pkg, make_emu, scene, spp=4, max_depth=2), scene)[..., :3]
    b = _render(pkg, _ctx(pkg, make_emu, scene, spp=4, max_depth=2, sky_sampling=1), scene)[..., :3]
    mse_a, mse_b = ((a - ref) ** 2).mean(), ((b - ref) ** 2).mean()
    assert mse_a >= 3.0 * mse_b, (mse_a, mse_b, mse_a / mse_b)


def test_closed_room_under_a_distant_lid_stays_black(pkg, make_emu):
    """The sky's shadow rays reach to t = 1e34: a room whose lid is a million units up gets no sky light."""
    sc = pkg.scenes
    s = sc.Scene()
    m = s.add_material(color=(0.8, 0.8, 0.8), roughness=1.0)
    v, i = sc._box((-1.0, 0.0, -1.0), (1.0, 1.0e6, 1.0), skip_bottom=False)
    s.add_instance(s.add_mesh(v, i, material=m))
    s.set_test_sky(64, 32, base=1.0)
    cam = sc.Camera(aperture=0.0, FOV=60.0, focalDistance=1.0)
    cam.look_at((0.0, 0.5, -0.9), (0.0, 0.2, 0.5))
    cam.resize(32, 24)
    s.camera = cam
    c = make_emu()
    c.init(32, 24)
    s.upload(c)
    for k, v_ in {"integrator": "pt", "spp": 16, "max_depth": 3, "sky_sampling": 1}.items():
        c.set_setting(k, v_)
    assert c.get_setting("sky") == "1"
    img = _render(pkg, c, s)
    assert np.array_equal(img[..., :3], np.zeros_like(img[..., :3]))


@pytest.mark.parametrize("n", [2, 3])
def test_group_of_emulated_contexts_equals_the_single_context(pkg, make_emu, emu_lib, n):
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    settings = {"integrator": "pt", "spp": 4, "max_depth": 2, "sky_sampling": 1}

    def run(target):
        target.init(70, 51)
        scene.upload(target)
        for k, v in settings.items():
            target.set_setting(k, v)
        for f in range(2):
            target.render_async(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
        target.wait()
        return target.framebuffer()

    ref = run(make_emu())
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0] * n, "peer")
    img = run(g)
    g.destroy()
    assert np.array_equal(img, ref)
    # ... and the sky variant did run: the image is not the default's
    settings["sky_sampling"] = 0
    assert not np.array_equal(run(make_emu()), ref)
