"""The light tree (setting light_sampling = reference | linear | tree; include/rfwhip.h; csrc/light_tree.h,
rt_core.h lt_importance / lt_sample / lt_pick_prob and pt_shade<TEX, SKY, true>), CPU tier: the host-emulation build runs the
same shade work items as k_shade_pt_lt.  The tree the host builds is downloaded and held to its invariants; the probabilities
of the known-answer hooks to the float64 model of tests/light_tree_model.py; the estimator of `tree` to that of `linear` (the
same weights, another picking rule: the same expectation); `reference` to the default kernels bit for bit."""
import math

import numpy as np
import pytest

import light_tree_model as model
from test_sky_sampling import _frames, _tile_z

# Largest |p_kat - p_model| over every light and every point of test_probabilities_match_the_float64_model, measured on the
# emulation build: 1.71e-6 (float32 sines and cosines against float64 angles; the probabilities are at most 1).  Allowed: four times it.
MODEL_ABS_MEASURED = 1.71e-6
MODEL_ABS_TOL = 4.0 * MODEL_ABS_MEASURED


# ---------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------
def _random_area_lights(pkg, n, seed, coincident=False):
    """n light triangles in a 12 x 6 x 12 box (no geometry of their own: the tree reads the light list)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform((-6, 1, -6), (6, 7, 6), (n, 3))
    if coincident:
        c[:] = c[0]
    e = rng.normal(size=(n, 2, 3)) * 0.3
    if coincident:
        e[:] = e[0]
    v0, v1, v2 = c, c + e[:, 0], c + e[:, 1]
    lights = np.zeros(n, dtype=pkg.abi.AREA_LIGHT_DTYPE)
    lights["vertex0"], lights["vertex1"], lights["vertex2"] = v0, v1, v2
    lights["position"] = (v0 + v1 + v2) / 3.0
    nrm = np.cross(e[:, 0], e[:, 1])
    lights["normal"] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    rad = rng.uniform(2.0, 20.0, (n, 3))
    lights["radiance"] = rad
    lights["energy"] = np.linalg.norm(rad.astype(np.float32), axis=1)
    lights["area"] = pkg.scenes.triangle_area(lights["vertex0"], lights["vertex1"], lights["vertex2"])
    lights["triIdx"], lights["instIdx"] = -1, -1
    return lights


def _light_scene(pkg, case):
    sc = pkg.scenes
    s = sc.Scene()
    m = s.add_material(color=(0.6, 0.6, 0.6), roughness=1.0)
    corners = np.array([[-8, 0, -8], [8, 0, -8], [-8, 0, 8], [8, 0, 8]], np.float32)
    s.add_instance(s.add_mesh(corners, np.array([[0, 2, 1], [1, 2, 3]], np.uint32), material=m))
    if isinstance(case, int):
        s.area_lights = _random_area_lights(pkg, case, seed=case)
    elif case == "coincident":
        s.area_lights = _random_area_lights(pkg, 9, seed=5, coincident=True)
    elif case == "zero_energy":
        s.area_lights = _random_area_lights(pkg, 12, seed=6)
        s.area_lights["energy"][[1, 4, 5]] = 0.0
        s.area_lights["energy"][7] = -3.0
        s.area_lights["energy"][9] = np.nan
    elif case in ("mixed", "directional_only"):
        if case == "mixed":
            s.area_lights = _random_area_lights(pkg, 20, seed=7)
            for k in range(5):
                s.add_point_light((-5.0 + 2.5 * k, 3.0 + 0.5 * k, 4.0 - k), (5.0 + k, 6.0, 7.0 - k))
            for k in range(4):
                s.add_spot_light((4.0 - 2.0 * k, 6.0, -3.0 + k), 15.0, (20.0, 18.0 + k, 15.0), 30.0, (0.1 * k, -1.0, 0.2))
        for d in ((0.3, -1.0, 0.2), (-0.5, -0.7, 0.1), (0.0, -1.0, -0.6)):
            s.add_directional_light(d, (0.9, 0.8, 0.7))
    cam = sc.Camera(aperture=0.0, FOV=50.0, focalDistance=5.0)
    cam.look_at((0.0, 3.0, -9.0), (0.0, 0.5, 0.0))
    cam.resize(32, 24)
    s.camera = cam
    s.wh = (32, 24)
    return s


def _lamp(pkg, n, w=48, h=32, extras=True):
    s = pkg.scenes.lamp_scene(n, w, h, extras=extras)
    s.camera.clampValue = 1e9  # (clamping is not linear: the statistical tests keep every contribution)
    s.wh = (w, h)
    return s


def _ctx(make_emu, scene, **settings):
    c = make_emu() if callable(make_emu) else make_emu
    c.init(*scene.wh)
    scene.upload(c)
    c.set_setting("integrator", "pt")
    for k, v in settings.items():
        c.set_setting(k, v)
    return c


def _n_lights(scene):
    return sum(len(a) for a in scene.light_arrays())


def _points(n, seed, lo=(-8, 0, -8), hi=(8, 7, 8)):
    """n records [I, N, r0, r1] with I in a box around the lights (and so inside many node boxes)."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 24), np.float32)
    rec[:, 0:3] = rng.uniform(lo, hi, (n, 3))
    nn = rng.normal(size=(n, 3))
    rec[:, 3:6] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
    rec[:, 6:8] = rng.random((n, 2))
    return rec


def _with_light(rec, light):
    r = rec.copy()
    r[:, 8] = np.broadcast_to(np.asarray(light, np.uint32), (len(rec),)).view(np.float32)
    return r


def _all_pick_probs(c, rec, n_lights):
    return np.stack([c.kat("lt_pick_prob", _with_light(rec, k))[:, 0] for k in range(n_lights)], 1)


# ---------------------------------------------------------------------------------------------------------------------------
# settings
# ---------------------------------------------------------------------------------------------------------------------------
def test_settings_defaults_values_and_unlisted_keys(pkg, make_emu):
    c = make_emu()
    assert c.get_setting("light_sampling") == "reference"
    assert c.get_setting("light_tree") == "0"
    for v in ("linear", "tree", "reference"):
        c.set_setting("light_sampling", v)
        assert c.get_setting("light_sampling") == v
    for bad in ("", "0", "1", "Tree", "bvh", "tree "):
        with pytest.raises(Exception, match="must be"):
            c.set_setting("light_sampling", bad)
    with pytest.raises(Exception):
        c.set_setting("light_tree", "5")  # read-only
    keys = list(c.get_settings())
    assert "light_sampling" not in keys and "light_tree" not in keys


def test_record_sizes(pkg):
    assert pkg.abi.LIGHT_TREE_NODE_DTYPE.itemsize == 64 and pkg.abi.LIGHT_TREE_PATH_DTYPE.itemsize == 8
    import os
    import re
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "rfwhip_abi.h")).read()
    assert re.search(r"sizeof\(rfwhip_light_tree_node\) == 64", text) and re.search(r"sizeof\(rfwhip_light_tree_path\) == 8", text)


def test_light_tree_key_follows_mode_and_lights(pkg, make_emu):
    scene = _light_scene(pkg, 17)
    c = _ctx(make_emu, scene)
    assert c.get_setting("light_tree") == "0"
    c.set_setting("light_sampling", "tree")
    assert c.get_setting("light_tree") == "34"
    c.set_setting("light_sampling", "linear")
    assert c.get_setting("light_tree") == "0" and len(c.get_light_tree(17)[0]) == 0
    c.set_setting("light_sampling", "tree")
    two = _light_scene(pkg, 2)
    c.set_lights(*two.light_arrays())  # (rfwhip_set_lights rebuilds the tree)
    assert c.get_setting("light_tree") == "4"
    for fn in ("lt_sample", "lt_pick_prob"):  # scene changed since the last update
        with pytest.raises(Exception):
            c.kat(fn, np.zeros((1, 24), np.float32))


def test_kat_needs_tree_mode(pkg, make_emu):
    scene = _light_scene(pkg, 3)
    c = _ctx(make_emu, scene)
    for mode in ("reference", "linear"):
        c.set_setting("light_sampling", mode)
        for fn in ("lt_sample", "lt_pick_prob"):
            with pytest.raises(Exception, match="light_sampling=tree"):
                c.kat(fn, np.zeros((1, 24), np.float32))
    c.set_setting("light_sampling", "tree")
    with pytest.raises(Exception, match="names light"):
        c.kat("lt_pick_prob", _with_light(_points(1, 0), 3))
    assert c.kat("lt_pick_prob", _with_light(_points(1, 0), 2)).shape == (1, 8)


def test_reference_after_tree_is_the_default_bit_for_bit(pkg, make_emu):
    scene = pkg.scenes.cornell(96, 64, geometric_emitter=True)
    scene.wh = (96, 64)

    def render(c):
        c.render_frame(scene.camera, pkg.RESET)
        return c.framebuffer()

    ref = render(_ctx(make_emu, scene, spp=2, max_depth=2))
    c = _ctx(make_emu, scene, spp=2, max_depth=2, light_sampling="tree")
    tree = render(c)
    assert not np.array_equal(tree, ref)
    c.set_setting("light_sampling", "reference")
    assert np.array_equal(render(c), ref)
    assert c.get_setting("light_tree") == "0"


# ---------------------------------------------------------------------------------------------------------------------------
# the tree
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [1, 2, 3, 17, 65, 1000, "coincident", "zero_energy", "mixed", "directional_only"])
def test_tree_invariants(pkg, make_emu, case):
    scene = _light_scene(pkg, case)
    c = _ctx(make_emu, scene, light_sampling="tree")
    area, point, spot, dirs = scene.light_arrays()
    nodes, paths = c.get_light_tree()
    assert int(c.get_setting("light_tree")) == len(nodes) and len(paths) == _n_lights(scene)
    model.check_tree(nodes, paths, area, point, spot, len(dirs))
    if case == "directional_only":
        assert len(nodes) == 0
    if case == 1:
        assert len(nodes) == 1 and nodes[0]["child"] == 0
    if case == "zero_energy":
        assert abs(float(nodes[0]["energy"]) - float(area["energy"][[0, 2, 3, 6, 8, 10, 11]].sum())) < 1e-3
    if case == "mixed":
        assert float(nodes[0]["cos_o"]) == -1.0


# ---------------------------------------------------------------------------------------------------------------------------
# probabilities
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(pkg, emu_lib):
    """The 1000-light scene of the probability tests: a lamp of 1000 triangles, two point lights, a spot and a directional
    light; 2000 points around and inside it; every light's probability at every point, once."""
    scene = _lamp(pkg, 1000)
    c = _ctx(pkg._binding.CoreBinding(emu_lib, "rfwhip_", 0, 0, 1), scene, light_sampling="tree")
    n = _n_lights(scene)
    rec = _points(2000, seed=11, lo=(-8, 0, -8), hi=(8, 8, 8))
    rec[:400, 0:3] = np.random.default_rng(12).uniform((-1.5, 3.0, -1.5), (2.5, 7.0, 2.5), (400, 3))  # around and inside the lamp
    nodes, paths = c.get_light_tree(n)
    return dict(scene=scene, c=c, n=n, rec=rec, nodes=nodes, paths=paths, probs=_all_pick_probs(c, rec, n))


def test_probabilities_sum_to_one_less_what_ends_nowhere(pkg, big):
    """The sum over all lights of LT_PICK_PROB is 1 within 1e-5 — less the share of the descent that ends at a node whose
    children both have no importance ("no light", as sum <= 0 gives today: every light below has no potential either, so
    nothing is lost but the sample).  That share comes from the float64 model; where it is 0 the sum is 1, where nothing has
    an importance the sum is 0."""
    area, point, spot, dirs = big["scene"].light_arrays()
    I, N = big["rec"][:, 0:3].astype(np.float64), big["rec"][:, 3:6].astype(np.float64)
    p_model, lost = model.light_probabilities(big["nodes"], big["n"] - len(dirs), dirs, I, N)
    total = big["probs"].astype(np.float64).sum(1)
    nothing = p_model.sum(1) + lost == 0
    assert nothing.sum() == 0 or np.all(total[nothing] == 0)
    whole = lost == 0
    assert whole.sum() > 100 and (~whole).sum() > 100  # (both kinds of point are there)
    assert np.abs(total[whole & ~nothing] - 1.0).max() <= 1e-5
    assert np.abs(total + lost - 1.0)[~nothing].max() <= 1e-5
    # How much may end nowhere: the lamp is a closed convex surface, so from any point outside it half of its energy or less
    # faces the point, and bounds that are worth having lose no more than what faces away — on average over the points that
    # see some light at most half.  (Measured on this scene: 0.25.)  A change that loosens the bounds shows up here.
    lit = p_model.sum(1) > 0
    print("share of the descent that ends nowhere, mean over %d lit points: %.3f" % (lit.sum(), lost[lit].mean()))
    assert lost[lit].mean() <= 0.5


def test_probabilities_match_the_float64_model(pkg, big):
    area, point, spot, dirs = big["scene"].light_arrays()
    I, N = big["rec"][:, 0:3].astype(np.float64), big["rec"][:, 3:6].astype(np.float64)
    p_model, _ = model.light_probabilities(big["nodes"], big["n"] - len(dirs), dirs, I, N)
    err = np.abs(big["probs"].astype(np.float64) - p_model).max()
    print("largest |p_kat - p_model| over %d x %d probabilities: %.3e (allowed %.3e)" % (p_model.shape + (err, MODEL_ABS_TOL)))
    assert err <= MODEL_ABS_TOL


def test_sample_probability_is_pick_prob_bit_for_bit(pkg, big):
    c, rec = big["c"], big["rec"]
    out = c.kat("lt_sample", rec)
    light = out[:, 5].view(np.int32)
    found = light >= 0
    assert found.sum() > 1000
    assert np.all(out[~found, 3] == 0) and np.all(out[~found, 4] == 0)
    q = big["probs"][np.nonzero(found)[0], light[found]]
    assert np.array_equal(q.view(np.uint32), out[found, 3].view(np.uint32))
    assert np.all(q > 0)
    # the point lies on the drawn light: an area light's inside its triangle's box
    area = big["scene"].light_arrays()[0]
    la = found & (light < len(area))
    v = np.stack([area[k][light[la]] for k in ("vertex0", "vertex1", "vertex2")])
    assert np.all(out[la, 0:3] >= v.min(0) - 1e-5) and np.all(out[la, 0:3] <= v.max(0) + 1e-5)


def test_conservative_wherever_a_potential_is_positive(pkg, make_emu, big):
    """Every area light whose RFWHIP_KAT_LIGHT_PICK_PROB is positive has LT_PICK_PROB > 0 — no exception.  On a 65-triangle lamp
    through the hook (it runs over all lights per record), with the emitter point at each corner and the centroid of the
    light; and on the 1000-light scene against the float64 potentials of the model at the same points."""
    scene = _lamp(pkg, 65)
    c = _ctx(make_emu, scene, light_sampling="tree")
    area = scene.light_arrays()[0]
    n = _n_lights(scene)
    rec = _points(2000, seed=21, lo=(-6, 0, -6), hi=(6, 8, 6))
    rec[:500, 0:3] = np.random.default_rng(22).uniform((-1.5, 3.0, -1.5), (2.5, 7.0, 2.5), (500, 3))
    lt = _all_pick_probs(c, rec, n)
    checked = 0
    for where in ("position", "vertex0", "vertex1", "vertex2"):
        for k in range(len(area)):
            r = _with_light(rec, k)
            r[:, 9:12] = rec[:, 0:3]   # O: the shading point
            r[:, 0:3] = area[where][k]  # I: the point on the emitter
            ref = c.kat("light_pick_prob", r)[:, 0]
            pos = ref > 0
            checked += int(pos.sum())
            assert np.all(lt[pos, k] > 0), (where, k)
    assert checked > 20000
    area = big["scene"].light_arrays()[0]
    I, N = big["rec"][:, 0:3].astype(np.float64), big["rec"][:, 3:6].astype(np.float64)
    for where in ("position", "vertex0", "vertex1", "vertex2"):
        pot = model.pot_area(area, I, N, area[where].astype(np.float64))
        assert np.all(big["probs"][:, : len(area)][pot > 0] > 0), where


def test_leaf_rank_is_monotone_in_r1_and_shares_match(pkg, big):
    """Along an increasing grid of 2^16 values of r1 the leaf rank never decreases, and the share of the grid that reaches a
    light equals its probability to within the grid spacing times the depth (one cell may straddle each interval's edge per
    level, and the rescaling rounds: depth + 2 cells are allowed)."""
    c = big["c"]
    g = 1 << 16
    depth_max = int(big["paths"]["depth"].max())
    for k in (3, 450, 1207):
        rec = np.repeat(big["rec"][k : k + 1], g, 0)
        rec[:, 7] = (np.arange(g, dtype=np.float64) + 0.5) / g
        out = c.kat("lt_sample", rec)
        light, rank = out[:, 5].view(np.int32), out[:, 6].view(np.int32)
        found = light >= 0
        if not found.any():
            continue
        assert np.all(np.diff(rank[found]) >= 0)
        share = np.bincount(light[found], minlength=big["n"]) / g
        assert np.abs(share - big["probs"][k]).max() <= (depth_max + 2) / g
    assert depth_max <= math.ceil(math.log2(big["n"]))


def test_directional_lights_only(pkg, make_emu):
    scene = _light_scene(pkg, "directional_only")
    c = _ctx(make_emu, scene, light_sampling="tree")
    rec = _points(500, seed=3)
    p = _all_pick_probs(c, rec, 3).astype(np.float64)
    dirs = scene.light_arrays()[3]
    pd = model.pot_dir(dirs, rec[:, 3:6].astype(np.float64))
    lit = pd.sum(1) > 0
    assert np.abs(p[lit] - pd[lit] / pd[lit].sum(1, keepdims=True)).max() <= 1e-6 and np.all(p[~lit] == 0)
    out = c.kat("lt_sample", rec)
    light = out[:, 5].view(np.int32)
    assert np.array_equal(light >= 0, lit)
    assert np.array_equal(out[lit, 3].view(np.uint32), p[lit][np.arange(lit.sum()), light[lit]].astype(np.float32).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# the estimator
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [1, 2])
def test_tree_and_linear_have_the_same_expectation(pkg, make_emu, max_depth):
    """Tile means of `tree` against `linear` within |z| <= 4 (test_sky_sampling._tile_z) on the lamp scene — 300 light
    triangles, two point lights, a spot, a directional light — at 48 x 32, spp 8, 24 frames.  The same bound holds for `linear`
    against `linear` from another sample origin (the second run's frames are the 25th to 48th of the sequence): what the
    bound lets through is the noise of the method, not the difference of the rules."""
    scene = _lamp(pkg, 300)
    frames = 24
    fl = _frames(pkg, _ctx(make_emu, scene, spp=8, max_depth=max_depth, light_sampling="linear"), scene, 2 * frames)
    ft = _frames(pkg, _ctx(make_emu, scene, spp=8, max_depth=max_depth, light_sampling="tree"), scene, frames)
    z0, _, _ = _tile_z(fl[:frames], fl[frames:])
    z, ma, mb = _tile_z(fl[:frames], ft)
    print("max_depth %d: max |z| linear / linear %.2f, linear / tree %.2f; means %.4f / %.4f" % (max_depth, np.abs(z0).max(), np.abs(z).max(), ma.mean(), mb.mean()))
    assert np.abs(z0).max() <= 4.0, np.abs(z0).max()
    assert np.abs(z).max() <= 4.0, np.abs(z).max()
    assert ma.mean() > 0.05 and mb.mean() > 0.05


def test_both_modes_meet_a_ground_truth_built_light_by_light(pkg, make_emu):
    """Point lights and a directional light at max_depth 1: the image is the sum of the images with each light alone (one light:
    nothing is picked, q = 1) less twice the image without lights (the lamp's geometry found by BSDF rays, part of every one of
    them).  `linear` and `tree` both agree with that sum within |z| <= 4 per tile over 32 frames.  This is the experiment behind
    the new kernels' own random-number stream: on the reference's depth-0 stream, where the light
    selection number is the pixel jitter, `tree` missed this sum by |z| = 11.5 and up to 29 % of a tile at this resolution."""
    frames = 32

    def base():
        s = _lamp(pkg, 300)
        s.area_lights = s.area_lights[:0]
        s.spot_lights = []
        return s

    def run(scene, mode):
        return _frames(pkg, _ctx(make_emu, scene, spp=8, max_depth=1, light_sampling=mode), scene, frames)

    parts = []
    for k in range(3):
        s = base()
        if k < 2:
            s.point_lights, s.directional_lights = [s.point_lights[k]], []
        else:
            s.point_lights = []
        parts.append(run(s, "linear"))
    s = base()
    s.point_lights, s.directional_lights = [], []
    truth = parts[0] + parts[1] + parts[2] - 2.0 * run(s, "linear")
    for mode in ("linear", "tree"):
        z, ma, mb = _tile_z(run(base(), mode), truth)
        print("%s against the light-by-light sum: max |z| %.2f, means %.4f / %.4f" % (mode, np.abs(z).max(), ma.mean(), mb.mean()))
        assert np.abs(z).max() <= 4.0, (mode, np.abs(z).max())
        assert ma.mean() > 0.05


@pytest.mark.parametrize("kind", ["point", "triangle"])
def test_one_light_tree_equals_linear_bit_for_bit(pkg, make_emu, kind):
    sc = pkg.scenes
    scene = sc.cornell(48, 32, geometric_emitter=False, point_light=(kind == "point"))
    scene.area_lights = scene.area_lights[:0]
    if kind == "triangle":  # one emissive triangle as geometry (BSDF rays find it) and as the one light
        em = scene.add_material(color=(20.0, 20.0, 20.0), roughness=1.0)
        q = sc.quad((0.0, -1.0, 0.0), (0.0, 9.99, 0.0), 3.0, 3.0)[:3]
        scene.add_instance(scene.add_mesh(q, None, material=em))
        scene.update_area_lights()
    assert _n_lights(scene) == 1
    scene.wh = (48, 32)
    imgs = []
    for mode in ("linear", "tree"):
        c = _ctx(make_emu, scene, spp=4, max_depth=2, light_sampling=mode)
        c.render_frame(scene.camera, pkg.RESET)
        imgs.append(c.framebuffer())
    assert imgs[0][..., :3].mean() > 1e-3
    assert np.array_equal(imgs[0], imgs[1])


@pytest.mark.parametrize("n", [2, 3])
def test_group_of_emulated_contexts_equals_the_single_context(pkg, make_emu, emu_lib, n):
    scene = _lamp(pkg, 65, 70, 51)
    settings = {"integrator": "pt", "spp": 4, "max_depth": 2, "light_sampling": "tree"}

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
    assert [c.get_setting("light_tree") for c in g.contexts] == ["%d" % (2 * 68)] * n  # (65 + 2 + 1 lights with a position)
    g.destroy()
    assert np.array_equal(img, ref)
    settings["light_sampling"] = "linear"
    assert not np.array_equal(run(make_emu()), ref)
