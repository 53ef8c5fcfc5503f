"""The denoiser of the presented image (setting "denoise", include/rfwhip.h; csrc/denoise.h), CPU tier: the host-emulation build
runs the same guide and filter work items as the HIP kernels.  Held to the numpy model of tests/denoise_model.py, to the
invariants the header promises, to rfwhip_trace_rays for the guides, and to the single context for groups."""
import ctypes

import numpy as np
import pytest

import denoise_model

W, H = 96, 64


def _ctx(pkg, make_emu, scene, w=W, h=H, spp=1, frames=1, **settings):
    c = make_emu()
    c.init(w, h)
    scene.upload(c)
    c.set_setting("integrator", "pt")
    c.set_setting("spp", spp)
    for k, v in settings.items():
        c.set_setting(k, v)
    for f in range(frames):
        c.render_frame(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
    return c


def _model(img, g, **kw):
    return denoise_model.denoise(img, g["albedo"], g["valid"], g["normal"], g["z"], **kw)


def _scene(pkg, name, w=W, h=H):
    return pkg.scenes.cornell(w, h, geometric_emitter=True) if name == "cornell" else pkg.scenes.cards(w, h)


@pytest.mark.parametrize("name", ["cornell", "cards"])
def test_filter_matches_the_numpy_model(pkg, make_emu, name):
    scene = _scene(pkg, name)
    c = _ctx(pkg, make_emu, scene)
    raw = c.framebuffer()
    g = c.read_denoise_guides()
    assert g["valid"].mean() > 0.5
    out = c.denoise_image(raw)
    np.testing.assert_allclose(out, _model(raw, g), rtol=1e-4, atol=1e-6)
    # other knobs go through too
    c.set_setting("denoise_iterations", 2)
    c.set_setting("denoise_sigma_luminance", 2.5)
    np.testing.assert_allclose(c.denoise_image(raw), _model(raw, g, iterations=2, sigma_l=2.5), rtol=1e-4, atol=1e-6)
    # the presented image with denoise=1 is the filter applied to the raw one
    c.set_setting("denoise_iterations", 5)
    c.set_setting("denoise_sigma_luminance", 4)
    c.set_setting("denoise", 1)
    assert np.array_equal(c.framebuffer(), out)
    assert not np.array_equal(out, raw)


def test_invariants(pkg, make_emu):
    scene = _scene(pkg, "cards")
    c = _ctx(pkg, make_emu, scene)
    raw = c.framebuffer()
    g = c.read_denoise_guides()
    v = g["valid"]
    # k * albedo (the demodulation's albedo, max(albedo, 1e-3)) on valid pixels comes back unchanged
    img = raw.copy()
    img[..., :3] = np.where(v[..., None], 0.37 * np.maximum(g["albedo"], 1e-3), raw[..., :3])
    out = c.denoise_image(img)
    np.testing.assert_allclose(out[v], img[v], rtol=1e-5)
    # invalid pixels: bit for bit, and the w channel is the input's
    assert (~v).any()
    out = c.denoise_image(raw)
    assert np.array_equal(out[~v].view(np.uint32), raw[~v].view(np.uint32))
    assert np.array_equal(out[..., 3], raw[..., 3])


def test_sky_only_scene_is_returned_unchanged(pkg, make_emu):
    s = pkg.scenes.Scene()
    s.add_material(color=(0.5, 0.5, 0.5))
    s.add_mesh(np.array([[0, -100, 0], [1, -100, 0], [0, -100, 1]], np.float32), np.array([[0, 1, 2]], np.uint32))
    s.add_instance(0)
    s.set_test_sky(64, 32)
    s.camera = pkg.Camera(aperture=0.0, FOV=40.0, focalDistance=5.0)
    s.camera.look_at((0, 0, 0), (0, 1, 1))
    s.camera.resize(48, 32)
    c = _ctx(pkg, make_emu, s, 48, 32, denoise=1)
    g = c.read_denoise_guides()
    assert not g["valid"].any()
    c.set_setting("denoise", 0)
    raw = c.framebuffer()
    c.set_setting("denoise", 1)
    assert np.array_equal(c.framebuffer().view(np.uint32), raw.view(np.uint32))


def test_denoise_off_is_the_raw_image_also_after_a_toggle(pkg, make_emu):
    scene = _scene(pkg, "cornell")
    a = _ctx(pkg, make_emu, scene)
    b = _ctx(pkg, make_emu, scene)
    for f in range(1, 5):
        if f == 2:
            b.set_setting("denoise", 1)
            den = b.framebuffer()
            assert not np.array_equal(den, a.framebuffer())
            b.set_setting("denoise", 0)
        a.render_frame(scene.camera, pkg.CONVERGE)
        b.render_frame(scene.camera, pkg.CONVERGE)
        assert np.array_equal(a.framebuffer().view(np.uint32), b.framebuffer().view(np.uint32)), f


def _centre_rays(c, cam, w, h):
    v = c.camera_view(cam)
    p1, p2, p3, pos = (np.array(getattr(v, k)[:3], np.float32) for k in ("p1", "p2", "p3", "pos"))
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    u = ((xs + np.float32(0.5)) * np.float32(1.0 / w)).astype(np.float32)
    vv = ((ys + np.float32(0.5)) * np.float32(1.0 / h)).astype(np.float32)
    d = p1 + (p2 - p1) * u[..., None] + (p3 - p1) * vv[..., None] - pos
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.broadcast_to(pos, d.shape).reshape(-1, 3), d.reshape(-1, 3).astype(np.float32)


@pytest.mark.parametrize("name", ["cornell", "cards"])
def test_guides_agree_with_trace_rays_and_the_material_table(pkg, make_emu, name):
    scene = _scene(pkg, name)
    c = _ctx(pkg, make_emu, scene)
    g = c.read_denoise_guides()
    o, d = _centre_rays(c, scene.camera, W, H)
    hit = c.trace_rays(o, d)
    z, valid = g["z"].reshape(-1), g["valid"].reshape(-1)
    alb, nrm = g["albedo"].reshape(-1, 3), g["normal"].reshape(-1, 3)
    packed, _ = pkg.scenes.pack_materials(scene.host_materials, scene.textures)
    checked = alpha = 0
    for i in range(0, W * H, 7):
        if hit["prim"][i] < 0:
            assert not valid[i]
            continue
        inst = scene.instances[hit["inst"][i]]
        mesh = scene.meshes[inst["mesh"]]
        tri = mesh["triangles"][hit["prim"][i]]
        mat = packed[tri["material"]]
        colour = np.asarray(mat["diffuse"], np.float32)
        textured = mat["flags"] & (1 << 2)
        if (colour > 1).any():
            assert not valid[i]
            continue
        if textured and z[i] != pytest.approx(hit["t"][i], rel=1e-5):
            alpha += 1  # an alpha hole: the guide ray went on behind the card
            assert z[i] > hit["t"][i]
            continue
        assert valid[i] and z[i] == pytest.approx(hit["t"][i], rel=1e-5, abs=1e-5), i
        assert abs(np.linalg.norm(nrm[i]) - 1) < 1e-4
        if not textured:
            np.testing.assert_allclose(alb[i], colour, rtol=1e-6)
            # flat geometry: the shading normal is the face normal, turned towards the camera
            idx = mesh["indices"][hit["prim"][i]] if mesh["indices"] is not None else np.arange(3) + 3 * hit["prim"][i]
            vt = (inst["transform"] @ np.c_[mesh["vertices"][idx][:, :3], np.ones(3)].T).T[:, :3]
            fn = np.cross(vt[1] - vt[0], vt[2] - vt[0])
            fn /= np.linalg.norm(fn)
            fn = fn if fn @ d[i] < 0 else -fn
            assert fn @ nrm[i] > 0.999, (i, fn, nrm[i])
        checked += 1
    assert checked > 300
    if name == "cards":
        assert alpha > 0


@pytest.mark.parametrize("n", [2, 3, 5])
def test_groups_equal_the_single_denoised_context(pkg, make_emu, emu_lib, n):
    # (the terrain: its group image is the single context's raw image bit for bit — test_group.py says which scenes are)
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    settings = {"integrator": "pt", "spp": 4, "max_depth": 2, "denoise": 1}
    ref = make_emu()
    ref.init(70, 51)
    scene.upload(ref)
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0] * n, "peer")
    g.init(70, 51)
    scene.upload(g)
    for k, v in settings.items():
        ref.set_setting(k, v), g.set_setting(k, v)
    for f in range(2):
        st = pkg.RESET if f == 0 else pkg.CONVERGE
        ref.render_frame(scene.camera, st)
        g.render_frame(scene.camera, st)
        want = ref.framebuffer()
        assert np.array_equal(g.framebuffer(), want), f
    # strip-local reads are never denoised (denoise=1 on every rank): each rank's strips are the raw image's rows, and so is the
    # root's de-interleave of them (the emulation's device memory is host memory: numpy buffers stand in for device buffers)
    ref.set_setting("denoise", 0)
    raw = ref.framebuffer()
    assert not np.array_equal(raw, want)
    lr = g.contexts[0].local_rows()
    gathered = np.zeros((n, lr, 70, 4), np.float32)
    for r, ctx in enumerate(g.contexts):
        ctx.read_local_framebuffer_device(gathered[r].ctypes.data)
        for yl in range(lr):
            k = yl // 8
            y = (k * n + ((n - 1 - r) if k & 1 else r)) * 8 + yl % 8  # rfwhip_row_owner's serpentine rule
            if y < 51:
                assert np.array_equal(gathered[r, yl], raw[y]), (r, yl)
    full = np.zeros((51, 70, 4), np.float32)
    g.contexts[0].deinterleave_device(gathered.ctypes.data, full.ctypes.data)
    assert np.array_equal(full, raw)
    g.destroy()


def _mse(a, b):
    return float(((a[..., :3].astype(np.float64) - b[..., :3]) ** 2).mean())


# measured on the emulation (Cornell, 64 x 64, max_depth 2, against 1024 spp): 1 spp 15.3x, 4 spp 9.3x — committed with margin
QUALITY = {1: 6.0, 4: 3.0}


@pytest.mark.parametrize("spp", [1, 4])
def test_quality_against_a_converged_render(pkg, make_emu, spp):
    scene = pkg.scenes.cornell(64, 64, geometric_emitter=True)
    ref = _ctx(pkg, make_emu, scene, 64, 64, spp=1024).framebuffer()
    c = _ctx(pkg, make_emu, scene, 64, 64, spp=spp)
    raw = c.framebuffer()
    c.set_setting("denoise", 1)
    den = c.framebuffer()
    gain = _mse(raw, ref) / _mse(den, ref)
    print("quality spp=%d: MSE raw %.5g denoised %.5g gain %.2f" % (spp, _mse(raw, ref), _mse(den, ref), gain))
    assert gain >= QUALITY[spp]


def _family6(emu_lib, c):
    ms, n = ctypes.c_float(), ctypes.c_uint32()
    f = emu_lib.rfwhip_get_kernel_time
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]
    assert f(c._ctx, 6, ctypes.byref(ms), ctypes.byref(n), 0) == 0
    return n.value


def test_guides_are_cached(pkg, make_emu, emu_lib):
    scene = _scene(pkg, "cornell")
    c = _ctx(pkg, make_emu, scene, stage_timing=1, denoise=1, denoise_iterations=3)
    filt = 1 + 3
    for f in range(4):
        c.render_frame(scene.camera, pkg.CONVERGE)
        c.framebuffer()
    assert _family6(emu_lib, c) == 2 + 4 * filt  # one guide pass (2 launches) for four presents
    cam = scene.camera
    cam.look_at((0.5, 5.3, -17.0), (0.0, 5.0, 0.0))
    c.render_frame(cam, pkg.RESET)
    c.framebuffer()
    c.render_frame(cam, pkg.CONVERGE)
    c.framebuffer()
    assert _family6(emu_lib, c) == 2 * 2 + 6 * filt  # the camera moved: one more
    c.update()
    c.render_frame(cam, pkg.CONVERGE)
    c.framebuffer()
    assert _family6(emu_lib, c) == 3 * 2 + 7 * filt  # rfwhip_update: one more


def test_settings_are_checked(pkg, make_emu):
    c = make_emu()
    c.init(16, 16)
    for k, v in [("denoise", "2"), ("denoise_iterations", "0"), ("denoise_iterations", "9"), ("denoise_sigma_normal", "x")]:
        with pytest.raises(RuntimeError):
            c.set_setting(k, v)
    with pytest.raises(RuntimeError, match="no frame"):
        c.read_denoise_guides()


def _uniform_texture(pkg, rgba):
    return pkg.scenes.make_texture_rgba8(np.broadcast_to(np.asarray(rgba, np.uint8), (16, 16, 4)).copy())


def _tangent_space(n):  # rt_core.h create_tangent_space (tools.h:204-211)
    s = 1.0 if n[2] >= 0 else -1.0
    a = -1.0 / (s + n[2])
    b = n[0] * n[1] * a
    return np.array([1 + s * n[0] * n[0] * a, s * b, -s * n[0]]), np.array([b, s + n[1] * n[1] * a, -n[1]])


def test_guides_after_texture_layers_normal_maps_and_alpha_cards(pkg, make_emu):
    """Textured guides against an independent numpy restatement, on cards whose textures are uniform (every mip level the same
    texel, so the level of detail cannot matter): albedo = (colour * t0 + t1) * t0 (getShadingData.h:150-166, 206: the base layer
    multiplies twice, the second layer adds), the normal = the tangent-space normal map applied to the card's shading normal, and an
    alpha card whose texels all have alpha 0 is passed through: its pixels show what lies behind, at the distance of both segments."""
    scene = pkg.scenes.cornell(W, H, geometric_emitter=True)
    t0, t1 = (200, 100, 50, 255), (20, 30, 40, 255)
    sn = np.array([0.3, -0.2, 0.93])
    sn /= np.linalg.norm(sn)
    nm = tuple(int(v) for v in np.clip(np.rint((sn * 0.5 + 0.5) * 255), 0, 255)) + (255,)
    colour = (0.8, 0.6, 0.9)
    m_tex = scene.add_material(color=colour, roughness=0.8, texture=scene.add_texture(_uniform_texture(pkg, t0)),
                               texture1=scene.add_texture(_uniform_texture(pkg, t1)),
                               normalmap=scene.add_texture(_uniform_texture(pkg, nm)))
    m_hole = scene.add_material(color=(1, 1, 1), texture=scene.add_texture(_uniform_texture(pkg, (0, 255, 0, 0))), alpha=True)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    quad_idx = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)

    def card(p0, ex, ey, mat):  # ex x ey = -z: facing the camera
        p0, ex, ey = (np.asarray(a, np.float32) for a in (p0, ex, ey))
        v = np.array([p0, p0 + ex, p0 + ex + ey, p0 + ey], np.float32)
        return scene.add_instance(scene.add_mesh(v, quad_idx, uvs=uv, material=mat))
    i_tex = card((1.0, 1.5, -3.0), (-3.0, 0, 0), (0, 3.0, 0), m_tex)
    i_hole = card((4.0, 1.0, -2.0), (-1.5, 0, 0), (0, 2.0, 0), m_hole)
    c = _ctx(pkg, make_emu, scene)
    g = c.read_denoise_guides()
    o, d = _centre_rays(c, scene.camera, W, H)
    hit = c.trace_rays(o, d)
    z, valid = g["z"].reshape(-1), g["valid"].reshape(-1)
    alb, nrm = g["albedo"].reshape(-1, 3), g["normal"].reshape(-1, 3)
    tex0, tex1 = np.array(t0[:3]) / 256.0, np.array(t1[:3]) / 256.0  # decode_rgba8: byte / 256
    want_alb = (np.float16(colour).astype(np.float64) * tex0 + tex1) * tex0
    n_card = np.array([0.0, 0.0, -1.0])
    T, B = _tangent_space(n_card)
    s = (np.array(nm[:3]) / 256.0 - 0.5) * 2.0
    s /= np.linalg.norm(s)
    want_n = T * s[0] + B * s[1] + n_card * s[2]
    want_n /= np.linalg.norm(want_n)
    on_tex = np.flatnonzero(hit["inst"] == i_tex)
    on_hole = np.flatnonzero(hit["inst"] == i_hole)
    assert len(on_tex) > 100 and len(on_hole) > 20
    assert valid[on_tex].all()
    np.testing.assert_allclose(z[on_tex], hit["t"][on_tex], rtol=1e-5)
    np.testing.assert_allclose(alb[on_tex], np.broadcast_to(want_alb, (len(on_tex), 3)), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(nrm[on_tex], np.broadcast_to(want_n, (len(on_tex), 3)), atol=2e-4)  # (octahedral snorm16)
    # the alpha card: on from I + 1e-5 D; the guide is the surface behind it, its z the sum of the two segments
    i1 = o[on_hole] + d[on_hole] * hit["t"][on_hole, None]
    behind = c.trace_rays(i1 + d[on_hole] * np.float32(1e-5), d[on_hole])
    assert (behind["prim"] >= 0).all()
    np.testing.assert_allclose(z[on_hole], hit["t"][on_hole] + 1e-5 + behind["t"], rtol=1e-5)
    packed, _ = pkg.scenes.pack_materials(scene.host_materials, scene.textures)
    for k, i in enumerate(on_hole):
        inst = scene.instances[behind["inst"][k]]
        mat = packed[scene.meshes[inst["mesh"]]["triangles"][behind["prim"][k]]["material"]]
        assert valid[i]
        np.testing.assert_allclose(alb[i], np.asarray(mat["diffuse"], np.float32), rtol=1e-6)


def test_reads_before_a_render_and_with_pending_scene_changes(pkg, make_emu):
    scene = _scene(pkg, "cornell")
    c = make_emu()
    c.init(W, H)
    scene.upload(c)
    c.set_setting("integrator", "pt")
    c.set_setting("denoise", 1)
    assert not c.framebuffer().any()  # nothing rendered: the empty image, unfiltered
    c.render_frame(scene.camera, pkg.RESET)
    den = c.framebuffer()
    c.set_sky(*scene.sky)  # a pending scene change: the current guides still belong to the rendered image
    assert np.array_equal(c.framebuffer(), den)
    cam = scene.camera
    cam.look_at((0.5, 5.3, -17.0), (0.0, 5.0, 0.0))
    with pytest.raises(RuntimeError, match="scene changed"):
        c.render_frame(cam, pkg.RESET)
    c.update()
    c.render_frame(cam, pkg.RESET)
    assert not np.array_equal(c.framebuffer(), den)
