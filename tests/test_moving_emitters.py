"""Moving emitters (setting lights_follow_geometry; include/rfwhip.h; csrc/light_follow.h), CPU tier: the
host-emulation build runs the work items of k_light_refresh / k_lt_refit_level / k_lt_refit_top.  The refreshed lights are held to
the float64 model of tests/moving_emitters_model.py within bounds counted from the roundings, everything the refresh must not
touch byte for byte; the refitted tree to the model's exact boxes, to containment of every light's normal, and to the pairwise
float64 union within four times the largest excess measured on this build."""
import ctypes
import math

import numpy as np
import pytest

import light_tree_model as lt_model
import moving_emitters_model as model
from test_light_tree import _all_pick_probs, _points, _with_light
from test_sky_sampling import _frames, _tile_z

SIZES = [1, 2, 3, 5, 64, 65, 1000]
GEOMETRY = ("position", "normal", "area", "vertex0", "vertex1", "vertex2")
KEPT = ("energy", "radiance", "dummy0", "triIdx", "instIdx", "dummy1")

# Tightness of the refitted cones (test_refit_known_answer, d): acos(cos_o) of a refitted inner node less the half angle of the
# model's pairwise float64 union.  Largest excess over every n of SIZES on the emulation build: 5.87e-5 rad (n = 1000; 3.5e-5 at
# 64 and 65, 1.4e-5 at 2) — the 2^-22 the kernel steps below the float cosine (light_follow.h: LF_COS_STEP) is 2^-22 / sin(theta)
# in angle, which is what shows at the narrow cones of neighbouring triangles; the angle margin itself is 7.6e-6.  Allowed: four
# times the measurement, the habit of test_light_tree.py for this tree.  The GPU tier reuses this allowance.
EXCESS_MEASURED = 5.87e-5
EXCESS_ALLOWED = 4.0 * EXCESS_MEASURED
# (c): a . n >= cos_o - 2^-22, four float32 ulps at 1 for the two rounded inputs
CONTAIN_SLACK = 2.0 ** -22


# ---------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------
def lamp_scene(pkg, n, w=48, h=32):
    """lamp_scene: a lamp of n emissive triangles (the last instance), two point lights, a spot, a directional light — plus two
    free-standing (-1, -1) area lights behind the lamp's in the list."""
    s = pkg.scenes.lamp_scene(n, w, h, extras=True)
    s.add_area_light_quad((0.0, -1.0, 0.0), (-3.0, 6.5, 2.0), 1.0, 0.8, (9.0, 8.0, 7.0))
    s.camera.clampValue = 1e9
    s.wh = (w, h)
    s.lamp_inst = len(s.instances) - 1
    s.n_lamp = n
    return s


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K


def trs(axis, deg, scale, t):
    M = np.eye(4)
    M[:3, :3] = rot(axis, deg) @ np.diag(scale)
    M[:3, 3] = t
    return M


MOVE = trs((1.0, 2.0, 0.5), 37.0, (1.3, 0.7, 1.9), (0.8, -1.1, 2.4))  # a rotation, a non-uniform scale, a translation


def model_instances(scene, verts=None):
    """what the model needs of every instance of the scene; verts: {mesh: float64 object-space vertices} where they are not the
    scene's own (a posed or morphed mesh: then the model computes the face normals itself)"""
    out = []
    for inst in scene.instances:
        mesh = scene.meshes[inst["mesh"]]
        t = np.asarray(inst["transform"], np.float64)
        tris = mesh["triangles"]
        idx = mesh["indices"] if mesh["indices"] is not None else np.arange(3 * len(tris)).reshape(-1, 3)
        d = dict(M=t.astype(np.float32), Nm=np.linalg.inv(t[:3, :3]).T.astype(np.float32), tris=np.asarray(idx, np.int64),
                 light_tri=tris["lightTriIdx"] >= 0)
        if verts is not None and inst["mesh"] in verts:
            v = np.asarray(verts[inst["mesh"]], np.float64)
            cr = np.cross(v[d["tris"][:, 1]] - v[d["tris"][:, 0]], v[d["tris"][:, 2]] - v[d["tris"][:, 0]])
            d["verts"], d["N"] = v, cr / np.linalg.norm(cr, axis=1, keepdims=True)
        else:
            d["verts"] = mesh["vertices"][:, :3].astype(np.float64)
            d["N"] = np.stack([tris["Nx"], tris["Ny"], tris["Nz"]], 1)
        out.append(d)
    return out


def zeroed(lights):
    """the lights with their geometry fields zeroed: only triIdx / instIdx say where they belong"""
    z = lights.copy()
    for f in GEOMETRY:
        z[f] = 0
    return z


def check_refreshed(got, given, scene, n_bound, verts=None, vertex_err=0.0, normal_err=0.0):
    """`got` (read_area_lights) against the model on `given` (what set_lights was handed); returns the bound mask"""
    mask, exp, err = model.derive(given, model_instances(scene, verts), vertex_err, normal_err)
    assert mask.sum() == n_bound
    # unbound lights: the host's bytes; bound ones: every field the refresh does not derive
    assert got[~mask].tobytes() == given[~mask].tobytes()
    for f in KEPT:
        assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(given[f]).tobytes(), f
    worst = {}
    for f in GEOMETRY:
        d = np.abs(got[f][mask].astype(np.float64) - exp[f][mask])
        assert np.all(d <= err[f][mask]), (f, float((d - err[f][mask]).max()))
        worst[f] = float((d / np.maximum(err[f][mask], 1e-300)).max()) if mask.any() else 0.0
    return mask, worst


def ctx_on(make, scene, lights=None, **settings):
    c = make() if callable(make) else make
    c.init(*scene.wh)
    scene.upload(c)
    c.set_setting("integrator", "pt")
    c.set_setting("lights_follow_geometry", 1)
    for k, v in settings.items():
        c.set_setting(k, v)
    if lights is not None:
        a, p, s, d = scene.light_arrays()
        c.set_lights(lights, p, s, d)
    c.update()  # (the setting came on, or the lights were set: this update refreshes)
    return c


def move_lamp(c, scene, M):
    scene.instances[scene.lamp_inst]["transform"] = np.asarray(M, np.float64)
    c.set_instance(scene.lamp_inst, scene.instances[scene.lamp_inst]["mesh"], M)
    c.update()


# ---------------------------------------------------------------------------------------------------------------------------
# setting
# ---------------------------------------------------------------------------------------------------------------------------
def test_setting_defaults_values_and_unlisted_keys(pkg, make_emu):
    c = make_emu()
    assert c.get_setting("lights_follow_geometry") == "0"
    assert c.get_setting("lights_bound") == "0" and c.get_setting("light_tree_refits") == "0"
    for v in ("1", "0", "1"):
        c.set_setting("lights_follow_geometry", v)
        assert c.get_setting("lights_follow_geometry") == v
    for bad in ("", "2", "-1", "on", "1 "):
        with pytest.raises(Exception, match="must be"):
            c.set_setting("lights_follow_geometry", bad)
    for key in ("lights_bound", "light_tree_refits"):
        with pytest.raises(Exception):
            c.set_setting(key, "1")  # read-only
    keys = list(c.get_settings())
    assert len(keys) == 31 and not {"lights_follow_geometry", "lights_bound", "light_tree_refits"} & set(keys)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. refresh, known answer
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_refresh_known_answer(pkg, make_emu, n):
    """The lamp under a rotation, a non-uniform scale and a translation; the lights handed over with zeroed geometry.  The bounds
    are counted in moving_emitters_model.derive: 4 roundings per vertex coordinate, 4 more for the centroid, 3 per normal
    coordinate, and for the area 4 per component of the cross product, 3 for its squared length and 1 for the root."""
    scene = lamp_scene(pkg, n)
    scene.instances[scene.lamp_inst]["transform"] = MOVE
    given = zeroed(scene.area_lights)
    c = ctx_on(make_emu, scene, lights=given)
    got = c.read_area_lights()
    mask, worst = check_refreshed(got, given, scene, n)
    print("n = %d: largest |error| / bound per field: %s" % (n, {k: round(v, 3) for k, v in worst.items()}))
    assert c.get_setting("lights_bound") == "%d" % n
    assert not mask[n:].any() and np.all(got["area"][:n] > 0)


def test_binding_rules(pkg, make_emu):
    """Unbound: (-1, -1), an instance index out of range or not in use, a triangle index out of range, a triangle that is not a light
    triangle — each keeps the host's bytes; the rest follow."""
    scene = lamp_scene(pkg, 5)
    given = zeroed(scene.area_lights)
    extra = given[:5].copy()
    extra["position"] = 7.0
    extra["instIdx"] = [99, scene.lamp_inst, 0, -5, scene.lamp_inst]
    extra["triIdx"] = [0, 1000000, 3, 2, -1]  # (instance 0 is the ground: triangle 3 exists and does not emit)
    given = np.concatenate([given, extra])
    c = ctx_on(make_emu, scene, lights=given)
    check_refreshed(c.read_area_lights(), given, scene, 5)
    assert c.get_setting("lights_bound") == "5"
    # nothing happened since: the next update does not refresh (the lights keep the bytes they have, the count stays)
    c.update()
    check_refreshed(c.read_area_lights(), given, scene, 5)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. lights follow device animation
# ---------------------------------------------------------------------------------------------------------------------------
def strip_scene(pkg, w=48, h=32):
    """The lamp scene with a lamp of two triangles (bumpy ground, two boxes, two point lights, a spot, a directional light) and, above
    the ground, an emissive strip of 8 indexed triangles (10 vertices) facing down, with its area lights derived as
    Scene.update_area_lights derives them; two free-standing lights last."""
    sc = pkg.scenes
    s = sc.lamp_scene(2, w, h, extras=True)
    em = s.add_material(color=(9.0, 8.0, 6.0), roughness=1.0)
    x = np.linspace(-2.0, 2.0, 5)
    verts = np.array([[xi, 3.0 + 0.1 * k, z] for k, xi in enumerate(x) for z in (-0.5, 0.6)], np.float32)
    idx = np.array([t for k in range(4) for t in ([2 * k, 2 * k + 2, 2 * k + 1], [2 * k + 1, 2 * k + 2, 2 * k + 3])], np.uint32)
    s.strip_mesh = s.add_mesh(verts, idx, material=em)
    M = trs((0, 1, 0), 20.0, (1.0, 1.0, 1.0), (0.5, 0.0, 1.0))
    s.lamp_inst = s.add_instance(s.strip_mesh, M)
    tris = s.meshes[s.strip_mesh]["triangles"]
    base = len(s.area_lights)
    lights = np.zeros(8, dtype=pkg.abi.AREA_LIGHT_DTYPE)
    Nm = np.linalg.inv(M[:3, :3]).T
    for k, f in enumerate(("vertex0", "vertex1", "vertex2")):
        lights[f] = (tris[f][:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    lights["position"] = (lights["vertex0"] + lights["vertex1"] + lights["vertex2"]) * np.float32(1.0 / 3.0)
    lights["normal"] = (np.stack([tris["Nx"], tris["Ny"], tris["Nz"]], 1).astype(np.float64) @ Nm.T).astype(np.float32)
    lights["radiance"] = (9.0, 8.0, 6.0)
    lights["energy"] = np.float32(np.linalg.norm(np.array((9.0, 8.0, 6.0), np.float32)))
    lights["area"] = tris["area"]
    lights["triIdx"], lights["instIdx"] = np.arange(8), s.lamp_inst
    tris["lightTriIdx"] = base + np.arange(8)
    s.area_lights = np.concatenate([s.area_lights, lights])
    s.add_area_light_quad((0.0, -1.0, 0.0), (-3.0, 6.5, 2.0), 1.0, 0.8, (9.0, 8.0, 7.0))
    s.wh, s.n_lamp, s.strip_first = (w, h), 8, base
    return s


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def test_lights_follow_pose_morph_and_instance(pkg, make_emu):
    """After rfwhip_pose_mesh, rfwhip_morph_mesh and rfwhip_set_instance, each followed by an update.  The model deforms in
    float64; the bound widens by the deformation's own roundings: skinning = 4 products and sums per matrix element, then 4 products
    and 3 sums per coordinate (gamma(12) of the magnitudes), morphing = one product and one sum per target (gamma(2 T))."""
    scene = strip_scene(pkg)
    mesh = scene.meshes[scene.strip_mesh]
    base = _f32(mesh["vertices"][:, :3])
    nv = len(base)
    given = zeroed(scene.area_lights)
    # -- pose: two joints, the weights run along the strip
    c = ctx_on(make_emu, scene, lights=given)
    wgt = np.zeros((nv, 4), np.float32)
    wgt[:, 0] = np.linspace(1.0, 0.0, nv)
    wgt[:, 1] = np.float32(1.0) - wgt[:, 0]
    joints = np.zeros((nv, 4), np.uint32)
    joints[:, 1] = 1
    c.set_mesh_skin(scene.strip_mesh, joints, wgt, np.tile(np.array([0.0, 1.0, 0.0], np.float32), (nv, 1)))
    J = np.stack([trs((0, 0, 1), 15.0, (1, 1, 1), (0.0, 0.2, 0.0)), trs((1, 0, 0), -25.0, (1.1, 0.9, 1.0), (0.3, 0.5, -0.2))]).astype(np.float32)
    c.pose_mesh(scene.strip_mesh, J)
    c.update()
    Jd, wd = J.astype(np.float64), wgt.astype(np.float64)
    blend = wd[:, 0, None, None] * Jd[0] + wd[:, 1, None, None] * Jd[1]
    posed = np.einsum("vij,vj->vi", blend[:, :3, :3], base) + blend[:, :3, 3]
    mag = np.einsum("vij,vj->vi", wd[:, 0, None, None] * np.abs(Jd[0])[:3, :3] + wd[:, 1, None, None] * np.abs(Jd[1])[:3, :3], np.abs(base)) + np.abs(blend[:, :3, 3])
    verr = model.gamma(12) * float(mag.max())
    nerr = _normal_err(posed, mesh["indices"], verr)
    check_refreshed(c.read_area_lights(), given, scene, 10, verts={scene.strip_mesh: posed}, vertex_err=verr, normal_err=nerr)
    assert c.get_setting("lights_bound") == "10"
    # ... and the instance moves under the posed mesh
    move_lamp(c, scene, MOVE)
    check_refreshed(c.read_area_lights(), given, scene, 10, verts={scene.strip_mesh: posed}, vertex_err=verr, normal_err=nerr)
    # -- morph: two targets on a fresh context
    scene = strip_scene(pkg)
    c = ctx_on(make_emu, scene, lights=given)
    rng = np.random.default_rng(5)
    tp = rng.normal(size=(2, nv, 3)).astype(np.float32) * 0.3
    c.set_mesh_morph(scene.strip_mesh, np.tile(np.array([0.0, 1.0, 0.0], np.float32), (nv, 1)), tp, np.zeros_like(tp))
    wm = np.array([0.75, -0.4], np.float32)
    c.morph_mesh(scene.strip_mesh, wm)
    c.update()
    morphed = base + (wm.astype(np.float64)[:, None, None] * tp.astype(np.float64)).sum(0)
    verr = model.gamma(4) * float((np.abs(base) + (np.abs(wm.astype(np.float64))[:, None, None] * np.abs(tp.astype(np.float64))).sum(0)).max())
    nerr = _normal_err(morphed, mesh["indices"], verr)
    check_refreshed(c.read_area_lights(), given, scene, 10, verts={scene.strip_mesh: morphed}, vertex_err=verr, normal_err=nerr)
    move_lamp(c, scene, MOVE)
    check_refreshed(c.read_area_lights(), given, scene, 10, verts={scene.strip_mesh: morphed}, vertex_err=verr, normal_err=nerr)


def _normal_err(v, idx, verr):
    """Bound of |device N - model N| per coordinate for N = normalize(cross(v1 - v0, v2 - v0)) in float32 on vertices off by verr:
    the cross product's error (two roundings of the edges, two per component, the vertices' own error) over its length — the
    part of it across N turns N by that much, to first order; doubled for the second order — and 6 roundings of the normalisation."""
    idx = np.asarray(idx, np.int64)
    worst = 0.0
    for t in idx:
        e1, e2 = v[t[1]] - v[t[0]], v[t[2]] - v[t[0]]
        d = model.U * (np.abs(v[t]).max() * 2) + 2 * verr
        a1, a2 = np.abs(e1) + d, np.abs(e2) + d
        dcr = np.array([model.gamma(2) * (a1[(a + 1) % 3] * a2[(a + 2) % 3] + a2[(a + 1) % 3] * a1[(a + 2) % 3])
                        + d * (a1[(a + 1) % 3] + a2[(a + 2) % 3] + a2[(a + 1) % 3] + a1[(a + 2) % 3]) for a in range(3)])
        worst = max(worst, 2.0 * float(np.linalg.norm(dcr)) / float(np.linalg.norm(np.cross(e1, e2))) + model.gamma(6))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# 3. off means off, 4. same bytes, same image
# ---------------------------------------------------------------------------------------------------------------------------
def _render(pkg, c, scene, status=None):
    c.render_frame(scene.camera, pkg.RESET if status is None else status)
    return c.framebuffer(), c.get_stats()


def _rays(st):
    return (st.primaryCount, st.secondaryCount, st.deepCount, st.shadowCount)


def test_off_means_off(pkg, make_emu):
    scene = lamp_scene(pkg, 65)
    imgs = []
    for explicit in (False, True):
        c = make_emu()
        c.init(*scene.wh)
        scene.instances[scene.lamp_inst]["transform"] = np.eye(4)
        scene.upload(c)
        c.set_setting("integrator", "pt")
        c.set_setting("spp", 4)
        c.set_setting("light_sampling", "tree")
        if explicit:
            c.set_setting("lights_follow_geometry", 0)
        move_lamp(c, scene, MOVE)
        assert c.read_area_lights().tobytes() == scene.area_lights.tobytes()
        assert c.get_setting("lights_bound") == "0" and c.get_setting("light_tree_refits") == "0"
        imgs.append(_render(pkg, c, scene)[0])
    assert np.array_equal(imgs[0], imgs[1])


@pytest.mark.parametrize("mode", ["reference", "linear"])
def test_same_bytes_same_image(pkg, make_emu, mode):
    """A derives its lights on the device; B, setting off, is handed A's lights (and, as a host that derives them itself would
    write, each light triangle's area = its light's area).  Same bytes, same image: 0 pixels differ, the ray counts are equal —
    which also says that the area A's emitter hits read from the shading record is the float its lights carry."""
    w, h = 96, 64
    scene = lamp_scene(pkg, 65, w, h)
    a = ctx_on(make_emu, scene, spp=8, max_depth=2, light_sampling=mode)
    move_lamp(a, scene, MOVE)
    la = a.read_area_lights()
    img_a, st_a = _render(pkg, a, scene)
    # B reaches the same scene the same way — uploaded at rest, then moved — so that both walk the same trees
    sb = lamp_scene(pkg, 65, w, h)
    lamp_mesh = sb.meshes[sb.instances[sb.lamp_inst]["mesh"]]
    lamp_mesh["triangles"]["area"][la["triIdx"][:65]] = la["area"][:65]
    b = make_emu()
    b.init(w, h)
    sb.upload(b)
    for k, v in dict(integrator="pt", spp=8, max_depth=2, light_sampling=mode).items():
        b.set_setting(k, v)
    b.update()
    move_lamp(b, sb, MOVE)
    b.set_lights(la, *sb.light_arrays()[1:])
    b.update()
    img_b, st_b = _render(pkg, b, sb)
    assert b.read_area_lights().tobytes() == la.tobytes() and b.get_setting("lights_bound") == "0"
    assert img_a[..., :3].mean() > 1e-3
    assert int((img_a != img_b).any(-1).sum()) == 0 and _rays(st_a) == _rays(st_b)


def _deform(c, scene, kind):
    """the strip posed (two joints) or morphed (two targets) on the device, then an update"""
    nv = len(scene.meshes[scene.strip_mesh]["vertices"])
    up = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (nv, 1))
    if kind == "pose":
        wgt = np.zeros((nv, 4), np.float32)
        wgt[:, 0] = np.linspace(1.0, 0.0, nv)
        wgt[:, 1] = np.float32(1.0) - wgt[:, 0]
        joints = np.zeros((nv, 4), np.uint32)
        joints[:, 1] = 1
        c.set_mesh_skin(scene.strip_mesh, joints, wgt, up)
        c.pose_mesh(scene.strip_mesh, np.stack([trs((0, 0, 1), 15.0, (1.6, 1.0, 1.5), (0.0, 0.2, 0.0)),
                                                trs((1, 0, 0), -25.0, (1.7, 0.9, 1.8), (0.3, 0.5, -0.2))]).astype(np.float32))
    else:
        tp = np.random.default_rng(5).normal(size=(2, nv, 3)).astype(np.float32) * 0.5
        c.set_mesh_morph(scene.strip_mesh, up, tp, np.zeros_like(tp))
        c.morph_mesh(scene.strip_mesh, np.array([0.75, -0.4], np.float32))
    c.update()


@pytest.mark.parametrize("mode", ["reference", "linear"])
@pytest.mark.parametrize("kind", ["pose", "morph"])
def test_light_area_is_the_shading_record_area_after_a_deformation(pkg, make_emu, kind, mode):
    """After rfwhip_pose_mesh / rfwhip_morph_mesh the light's `area` (next-event estimation) and the triangle's shading-record
    area (the density of an emitter found by a BSDF ray) are the same float.  A: the setting on.  B: the setting off, the same
    deformation on the device, A's lights through rfwhip_set_lights, and the shading-record area a host writes: its triangles'
    `area` = A's lights' (the deformation kernels carry ex.x through: the host's value stays).  B's two areas are A's light area by
    construction, so bit-equal images and ray counts say A's shading record holds it too.  C is B with the bind pose's areas in
    the strip's triangles — the state the records were left in before: its image differs, which is what makes the comparison a test."""
    w, h = 96, 64
    settings = dict(integrator="pt", spp=8, max_depth=2, light_sampling=mode)

    def other(areas):
        s = strip_scene(pkg, w, h)
        for k in np.nonzero(la["instIdx"] >= 0)[0]:  # (every bound light's triangle: the static lamp's two as well)
            if areas is not None or not first <= k < first + 8:
                s.meshes[s.instances[la["instIdx"][k]]["mesh"]]["triangles"]["area"][la["triIdx"][k]] = la["area"][k]
        c = make_emu()
        c.init(w, h)
        s.upload(c)
        for k, v in settings.items():
            c.set_setting(k, v)
        c.update()
        _deform(c, s, kind)
        c.set_lights(la, *s.light_arrays()[1:])
        c.update()
        assert c.get_setting("lights_bound") == "0" and c.read_area_lights().tobytes() == la.tobytes()
        img, st = _render(pkg, c, s)
        return img, _rays(st)

    sa = strip_scene(pkg, w, h)
    a = ctx_on(make_emu, sa, lights=zeroed(sa.area_lights), **{k: v for k, v in settings.items() if k != "integrator"})
    _deform(a, sa, kind)
    assert a.get_setting("lights_bound") == "10"
    la = a.read_area_lights()
    first = sa.strip_first
    bind = sa.area_lights["area"][first:first + 8]
    change = np.abs(la["area"][first:first + 8] / bind - 1.0)
    assert np.all(change > 1e-3) and (change > 0.05).sum() >= 6  # (the deformation changes every area by far more than rounding)
    img_a, st_a = _render(pkg, a, sa)
    img_b, rays_b = other(True)
    assert img_a[..., :3].mean() > 1e-3 and rays_b[1] > 0 and rays_b[3] > 0
    assert int((img_a != img_b).any(-1).sum()) == 0 and _rays(st_a) == rays_b
    if mode == "linear":  # (`reference` weights an emitter hit without the area)
        img_c, _ = other(None)
        assert int((img_a != img_c).any(-1).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 5. refit, known answer
# ---------------------------------------------------------------------------------------------------------------------------
def moved_lights(lights, n, seed):
    """the first n lights after a random rigid move plus per-vertex noise (normals, centroids and areas follow in float32)"""
    rng = np.random.default_rng(seed)
    R = rot(rng.normal(size=3), float(rng.uniform(20, 160)))
    t = rng.uniform(-3, 3, 3)
    out = lights.copy()
    v = [(lights[f][:n].astype(np.float64) @ R.T + t + rng.normal(size=(n, 3)) * 0.02).astype(np.float32) for f in ("vertex0", "vertex1", "vertex2")]
    out["vertex0"][:n], out["vertex1"][:n], out["vertex2"][:n] = v
    out["position"][:n] = (v[0] + v[1] + v[2]) * np.float32(1.0 / 3.0)
    out["normal"][:n] = np.cross(v[1] - v[0], v[2] - v[0])  # (not normalised: the leaf normalises)
    return out


def refit_case(pkg, c_tree, scene, n, seed=None):
    """(nodes before, nodes after the hook, moved lights, bound) for the lamp scene's tree"""
    nodes, _ = c_tree.get_light_tree()
    area = moved_lights(scene.area_lights, n, 100 + n if seed is None else seed)
    bound = np.zeros(len(area), np.uint8)
    bound[:n] = 1
    if n >= 5:
        area["normal"][3] = 0.0  # (e) a degenerate normal
        bound[1] = 0             # an area light of the lamp that is not bound: it stays where the host put it, its leaf keeps its bytes
        area[1] = scene.area_lights[1]
    return nodes, area, bound


def check_refit(nodes, after, area, bound, n, allowed):
    touched, lo, hi, axis, theta = model.refit(nodes, area, bound)
    n_area = len(area)
    # (a) topology, energy, and every node without a bound leaf below: bit for bit
    for f in ("child", "light", "count", "energy", "pad"):
        assert after[f].tobytes() == nodes[f].tobytes(), f
    assert after[~touched].tobytes() == nodes[~touched].tobytes()
    leaves = nodes["child"] == 0
    other = leaves & ((nodes["light"] >= n_area) | ~bound.astype(bool)[np.minimum(nodes["light"], n_area - 1)])
    if len(nodes) > 1:
        other[1] = True
    assert not touched[other].any() and other.sum() >= (len(nodes) // 2 - int(bound.sum())) 
    # (b) the boxes are the exact bottom-up bounds
    assert after["lo"][touched].tobytes() == lo[touched].tobytes() and after["hi"][touched].tobytes() == hi[touched].tobytes()
    # (c) every light's normal in every cone above it
    gap = model.containment_gaps(after, area)
    assert gap >= -CONTAIN_SLACK, gap
    # (d) tightness against the pairwise float64 union
    excess = 0.0
    for i in np.nonzero(touched & ~leaves)[0]:
        co = float(after["cos_o"][i])
        got = math.acos(min(1.0, co)) if co > -1.0 else math.pi
        assert got >= theta[i] - 1e-6, (i, got, theta[i])  # (never tighter than the union of what it unites)
        excess = max(excess, got - theta[i])
    assert excess <= allowed, excess
    # (e) a degenerate normal: the leaf opens up
    if n >= 5:
        leaf = np.nonzero(leaves & (nodes["light"] == 3))[0][0]
        assert float(after["cos_o"][leaf]) == -1.0 and touched[leaf]
    for i in np.nonzero(touched & leaves)[0]:
        k = int(nodes["light"][i])
        if not (n >= 5 and k == 3):
            assert float(after["cos_o"][i]) == 1.0
    return excess


@pytest.mark.parametrize("n", SIZES)
def test_refit_known_answer(pkg, make_emu, n):
    scene = lamp_scene(pkg, n)
    c = ctx_on(make_emu, scene, light_sampling="tree")
    nodes, area, bound = refit_case(pkg, c, scene, n)
    after = c.light_tree_refit(nodes, area, bound)
    excess = check_refit(nodes, after, area, bound, n, EXCESS_ALLOWED)
    print("n = %d: %d nodes, largest excess of a refitted cone over the float64 pairwise union: %.3e rad (allowed %.3e)" % (n, len(nodes), excess, EXCESS_ALLOWED))
    # the same lights give the same bytes
    assert c.light_tree_refit(nodes, area, bound).tobytes() == after.tobytes()
    # the context's own tree was not touched by the hook
    assert c.get_light_tree()[0].tobytes() == nodes.tobytes() and c.get_setting("light_tree_refits") == "0"


def test_topology_is_built_from_the_refreshed_lights(pkg, make_emu):
    """rfwhip_set_lights under the setting does not make a topology of geometry fields that are about to be overwritten (here:
    zeros, which would split the lights by index): the update builds the tree from the lights its refresh derives — the topology of
    a context that was handed the true lights — also when the tree was asked for in between.  A later move refits it."""
    scene = lamp_scene(pkg, 65)
    ref = ctx_on(make_emu, scene, light_sampling="tree")
    want = ref.get_light_tree()[0]
    for ask_first in (False, True):
        c = make_emu()
        c.init(*scene.wh)
        scene.upload(c)
        for k, v in dict(integrator="pt", lights_follow_geometry=1, light_sampling="tree").items():
            c.set_setting(k, v)
        given = scene.area_lights.copy()
        given[:65] = zeroed(given[:65])  # (the free-standing lights keep their bytes, so they keep their geometry)
        c.set_lights(given, *scene.light_arrays()[1:])
        if ask_first:
            assert len(c.get_light_tree()[0]) == len(want)  # (built of zeros, for whoever asks now)
        c.update()
        got = c.get_light_tree()[0]
        assert c.get_setting("light_tree_refits") == "0" and c.get_setting("lights_bound") == "65"
        for f in ("child", "light", "count", "lo", "hi"):
            assert got[f].tobytes() == want[f].tobytes(), (ask_first, f)
    move_lamp(c, scene, MOVE)
    assert c.get_setting("light_tree_refits") == "1"
    scene.instances[scene.lamp_inst]["transform"] = np.eye(4)


def test_refit_hook_refuses_what_is_not_a_tree(pkg, make_emu):
    scene = lamp_scene(pkg, 5)
    c = ctx_on(make_emu, scene, light_sampling="tree")
    nodes, area, bound = refit_case(pkg, c, scene, 5)
    bad = nodes.copy()
    bad["child"][0] = 2 * len(nodes)
    with pytest.raises(Exception, match="not a tree"):
        c.light_tree_refit(bad, area, bound)
    bad = nodes.copy()
    bad["light"][bad["child"] == 0] = 1000
    with pytest.raises(Exception, match="not a tree"):
        c.light_tree_refit(bad, area, bound)
    with pytest.raises(Exception):
        c.light_tree_refit(nodes[:-1], area, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. picking stays consistent on a refit tree
# ---------------------------------------------------------------------------------------------------------------------------
def moved_tree_ctx(pkg, make, n, **settings):
    scene = lamp_scene(pkg, n)
    c = ctx_on(make, scene, light_sampling="tree", **settings)
    move_lamp(c, scene, trs((0.3, 1.0, 0.2), 140.0, (1.0, 1.0, 1.0), (-2.5, 0.5, 1.5)))
    assert c.get_setting("light_tree_refits") == "1" and c.get_setting("lights_bound") == "%d" % n
    return scene, c


def check_picking(pkg, scene, c, n):
    area = c.read_area_lights()
    _, point, spot, dirs = scene.light_arrays()
    total = len(area) + len(point) + len(spot) + len(dirs)
    nodes, paths = c.get_light_tree(total)
    rec = _points(600, seed=31, lo=(-8, 0, -8), hi=(8, 8, 8))
    rec[:200, 0:3] = np.random.default_rng(32).uniform((-4.5, 2.0, 0.0), (-0.5, 8.0, 4.0), (200, 3))  # around the moved lamp
    probs = _all_pick_probs(c, rec, total)
    # the sampler's q is LT_PICK_PROB of the light it drew, bit for bit
    out = c.kat("lt_sample", rec)
    light = out[:, 5].view(np.int32)
    found = light >= 0
    assert found.sum() > 200
    q = probs[np.nonzero(found)[0], light[found]]
    assert np.array_equal(q.view(np.uint32), out[found, 3].view(np.uint32)) and np.all(q > 0)
    # the probabilities and what ends nowhere sum to 1
    I, N = rec[:, 0:3].astype(np.float64), rec[:, 3:6].astype(np.float64)
    p_model, lost = lt_model.light_probabilities(nodes, total - len(dirs), dirs, I, N)
    nothing = p_model.sum(1) + lost == 0
    assert np.abs(probs.astype(np.float64).sum(1) + lost - 1.0)[~nothing].max() <= 1e-5
    # conservative: wherever the reference's potential of a light is positive, every node on its path has an importance
    checked = 0
    for where in ("position", "vertex0", "vertex1", "vertex2"):
        for k in range(min(n, 65)):
            r = _with_light(rec, k)
            r[:, 9:12] = rec[:, 0:3]
            r[:, 0:3] = area[where][k]
            pos = c.kat("light_pick_prob", r)[:, 0] > 0
            checked += int(pos.sum())
            assert np.all(probs[pos, k] > 0), (where, k)
    return checked


@pytest.mark.parametrize("n", [5, 65])
def test_picking_is_consistent_on_a_refit_tree(pkg, make_emu, n):
    scene, c = moved_tree_ctx(pkg, make_emu, n)
    assert check_picking(pkg, scene, c, n) > 1000


# ---------------------------------------------------------------------------------------------------------------------------
# 7. no bias after a move
# ---------------------------------------------------------------------------------------------------------------------------
def test_tree_after_refit_and_linear_have_the_same_expectation(pkg, make_emu):
    """The thresholds of test_light_tree.py: |z| <= 4 per 8 x 8 tile over 24 frames of 8 spp at 48 x 32, for `tree` on the refit
    tree against `linear` on the same refreshed lights, and for `linear` against `linear` from another sample origin."""
    frames = 24
    sl, cl = _moved(pkg, make_emu, 300, "linear")
    st, ct = _moved(pkg, make_emu, 300, "tree")
    assert ct.get_setting("light_tree_refits") == "1" and cl.read_area_lights().tobytes() == ct.read_area_lights().tobytes()
    fl = _frames(pkg, cl, sl, 2 * frames)
    ft = _frames(pkg, ct, st, frames)
    z0, _, _ = _tile_z(fl[:frames], fl[frames:])
    z, ma, mb = _tile_z(fl[:frames], ft)
    print("max |z| linear / linear %.2f, linear / refit tree %.2f; means %.4f / %.4f" % (np.abs(z0).max(), np.abs(z).max(), ma.mean(), mb.mean()))
    assert np.abs(z0).max() <= 4.0, np.abs(z0).max()
    assert np.abs(z).max() <= 4.0, np.abs(z).max()
    assert ma.mean() > 0.05 and mb.mean() > 0.05


def _moved(pkg, make, n, mode, **settings):
    scene = lamp_scene(pkg, n)
    c = ctx_on(make, scene, spp=8, max_depth=2, light_sampling=mode, **settings)
    move_lamp(c, scene, trs((0.3, 1.0, 0.2), 140.0, (1.0, 1.0, 1.0), (-2.5, 0.5, 1.5)))
    return scene, c


# ---------------------------------------------------------------------------------------------------------------------------
# 8. scheduling, 10. groups
# ---------------------------------------------------------------------------------------------------------------------------
def sequence(pkg, target, scene, settings, wait_between):
    """render, move, update, render — pipelined: the first call is still in flight when the move arrives unless wait_between"""
    target.init(*scene.wh)
    scene.instances[scene.lamp_inst]["transform"] = np.eye(4)
    scene.upload(target)
    for k, v in settings.items():
        target.set_setting(k, v)
    target.update()
    target.render_async(scene.camera, pkg.RESET)
    target.render_async(scene.camera, pkg.CONVERGE)
    if wait_between:
        target.wait()
    M = trs((0.3, 1.0, 0.2), 140.0, (1.0, 1.0, 1.0), (-2.5, 0.5, 1.5))
    scene.instances[scene.lamp_inst]["transform"] = M
    target.set_instance(scene.lamp_inst, scene.instances[scene.lamp_inst]["mesh"], M)
    target.update()
    target.render_async(scene.camera, pkg.RESET)
    target.render_async(scene.camera, pkg.CONVERGE)
    target.wait()
    st = target.get_stats()  # (a group: one record per rank)
    return target.framebuffer(), [_rays(x) for x in (st if isinstance(st, list) else [st])]


SEQ_BASE = {"integrator": "pt", "spp": 4, "max_depth": 2, "light_sampling": "tree", "lights_follow_geometry": 1}
SEQ_MATRIX = ({"ring": 1, "streams": 1}, {"ring": 2}, {"ring": 4}, {"streams": 4, "sub_batch_paths": 1}, {"fuse": 0}, {"fuse": 0, "ring": 4},
              {"shadow_packets": 1, "spp": 16}, {"shadow_packets": 0, "spp": 16}, {"shadow_side": 0, "overlap": 1})


@pytest.fixture(scope="module")
def streams_lib():
    import build_emu
    lib = ctypes.CDLL(build_emu.build(defines=("-DRFWHIP_EMU_STREAMS=1",), tag="_streams"))
    lib.rfwhip_emu_set_schedule.restype, lib.rfwhip_emu_set_schedule.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_uint]
    yield lib
    lib.rfwhip_emu_set_schedule(0, 0)


@pytest.mark.parametrize("policy", [(1, 0), (2, 7), (2, 1234), (3, 0)], ids=["late", "random-7", "random-1234", "eager"])
def test_scheduling_changes_no_bit(pkg, streams_lib, policy):
    """test_schedule.py's mechanism: the deferred-stream emulation runs what each sync point needs in an adversarial order."""
    scene = lamp_scene(pkg, 65)
    make = lambda: pkg._binding.CoreBinding(streams_lib, "rfwhip_", 0, 0, 1)
    refs = {}
    for extra in SEQ_MATRIX:
        settings = dict(SEQ_BASE, **extra)
        spp = settings["spp"]
        if spp not in refs:
            assert streams_lib.rfwhip_emu_set_schedule(0, 0) == 0
            refs[spp] = sequence(pkg, make(), scene, dict(SEQ_BASE, spp=spp, ring=1, streams=1), True)
        assert streams_lib.rfwhip_emu_set_schedule(*policy) == 0
        img, rays = sequence(pkg, make(), scene, settings, False)
        assert np.array_equal(img, refs[spp][0]) and rays == refs[spp][1], extra
    assert refs[4][0][..., :3].mean() > 1e-3 and refs[4][1][0][0] > 0


@pytest.mark.parametrize("world", [2, 3])
def test_group_of_emulated_contexts(pkg, make_emu, emu_lib, world):
    scene = lamp_scene(pkg, 65, 70, 51)
    ref, _ = sequence(pkg, make_emu(), scene, SEQ_BASE, False)
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0] * world, "peer")
    img, _ = sequence(pkg, g, scene, SEQ_BASE, False)
    lights = [c.read_area_lights().tobytes() for c in g.contexts]
    assert all(l == lights[0] for l in lights) and lights[0] != scene.area_lights.tobytes()
    assert [c.get_setting("lights_bound") for c in g.contexts] == ["65"] * world
    assert [c.get_setting("light_tree_refits") for c in g.contexts] == ["1"] * world
    g.destroy()
    assert np.array_equal(img, ref)
