"""Animations on the device, CPU tier (include/rfwhip.h, rfwhip_set_rig / rfwhip_bind_rig / rfwhip_animate / rfwhip_read_rig;
csrc/animation.h): the host emulation of the work items is held to the float64 model of tests/animation_model.py — every value
within a bound counted from the roundings of the header's shapes, no measured tolerance — the model itself to gltf.py's recorded
float64 values, and the validator and the work items to the host sanitizers in a stand-alone program.  The HIP kernel runs the same
checks in test_animation_gpu.py."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import animation_model as am
from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")
f32, f64 = np.float32, np.float64


@pytest.fixture
def emu(make_emu):
    c = make_emu()
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def rigs(pkg):
    return am.all_rigs(pkg)


RIG_NAMES = ["sampling 1 keys", "sampling 2 keys", "sampling 4 keys", "duration 0", "65 channels", "zero quaternions"] + \
    ["hierarchy %s" % k for k in ("one", "roots", "reversed", "chain", 65, 300, am.LDS_NODES, am.LDS_NODES + 1)] + \
    ["skin %s" % k for k in (1, 65, "two", "animated", "singular")]


# ---- 1. the model ----------------------------------------------------------------------------------------------------------------
def test_the_rig_list_is_the_parameter_list(rigs):
    assert sorted(rigs) == sorted(RIG_NAMES)


def test_bounds_are_not_vacuous(rigs):
    """From the model alone: on every test rig and time, every bound stays below 2^-12 of the largest entry of its matrix, and
    every mesh node's |det| lies within [1/8, 8] (the singular one's is exactly 0)."""
    worst = 0.0
    for name, (rig, times) in rigs.items():
        for t in times:
            ev = am.evaluate(rig, 0, t)
            worst = max(worst, am.largest_relative_bound(ev))
            for det in ev["det"]:
                assert det.v == 0.0 if (name == "skin singular" and det is ev["det"][1]) else 0.125 <= abs(det.v) <= 8.0, (name, t, det.v)
    assert 0.0 < worst < am.CAP, worst


def test_the_model_samples_known_values(pkg):
    """Hand-computed values: LINEAR halfway, STEP, the inner key reached as f == 1 of the segment before, the wrap, a CUBICSPLINE
    with zero tangents at f = 1/2 (the Hermite form gives the mean), and the interleaved layout of a weights key."""
    t = [0.0, 1.0, 3.0]
    rig = am.pack(pkg, [am.node(weights=[0.0, 0.0]), am.node(parent=0), am.node(parent=0)], [],
                  [[am.channel(0, am.TRANSLATION, am.LINEAR, t, [0, 0, 0, 2, 4, 6, 4, 4, 4]),
                    am.channel(1, am.SCALE, am.STEP, t, [1, 1, 1, 2, 2, 2, 3, 3, 3]),
                    am.channel(2, am.TRANSLATION, am.CUBICSPLINE, t, [9, 9, 9, 1, 2, 3, 0, 0, 0, 0, 0, 0, 3, 4, 5, 9, 9, 9, 0, 0, 0, 7, 7, 7, 0, 0, 0]),
                    am.channel(0, am.WEIGHTS, am.CUBICSPLINE, t, [9, 0.25, 0, 9, 0.5, 0, 0, 0.75, 0, 0, 1.0, 0, 0, 0, 9, 0, 0, 9])]])
    at = lambda time: am.evaluate(rig, 0, time)  # noqa: E731
    assert np.array_equal(at(0.5)["trs"].v[0, :3], [1, 2, 3]) and np.array_equal(at(0.5)["trs"].v[1, 7:], [1, 1, 1])
    assert np.array_equal(at(1.0)["trs"].v[0, :3], [2, 4, 6]) and np.array_equal(at(1.0)["trs"].v[1, 7:], [1, 1, 1])  # (f == 1 of segment 0)
    assert np.array_equal(at(2.0)["trs"].v[1, 7:], [2, 2, 2]) and np.array_equal(at(3.0)["trs"].v[0, :3], [4, 4, 4])
    assert np.array_equal(at(3.5)["trs"].v[0, :3], [1, 2, 3]) and at(3.5)["status"]["time"] == 0.5  # (wraps to 0.5)
    assert np.array_equal(at(-1.0)["trs"].v[0, :3], [0, 0, 0]) and np.array_equal(at(-1.0)["trs"].v[2, :3], [1, 2, 3])
    assert np.allclose(at(0.5)["trs"].v[2, :3], [2, 3, 4], atol=1e-15)
    assert np.allclose(at(0.5)["weights"].v, [0.5, 0.75], atol=1e-15) and np.array_equal(at(0.0)["weights"].v, [0.25, 0.5])


def test_the_model_is_gltf_py_on_the_fixture(pkg):
    """On the fixture's rigs and times the model agrees with gltf.py's recorded float64 values to 1e-12 of the largest entry."""
    fx = np.load(os.path.join(GOLD, "asset_animation.npz"))
    names = sorted(set(k.split("/")[0] for k in fx.files))
    assert "cesiumman" in names
    for name in names:
        rig = _fixture_rig(pkg, fx, name)
        for k, t in enumerate(fx[name + "/times"]):
            ev = am.evaluate(rig, 0, t)

            def close(got, want):
                want = np.asarray(want, f64)
                scale = np.abs(want).max(axis=(-1, -2), keepdims=True) if want.ndim >= 2 else max(1.0, np.abs(want).max(initial=0.0))
                assert (np.abs(got - want) <= 1e-12 * scale).all(), (name, t, float(np.abs(got - want).max()))
            close(ev["trs"].v[:, None, :], fx[name + "/trs"][k][:, None, :])
            close(ev["world"].v, fx[name + "/world"][k])
            close(ev["weights"].v, fx[name + "/weights"][k])
            joints = fx[name + "/joints"][k]
            if len(joints):
                close(np.concatenate([j.v for j in ev["joints"]]), joints)


# ---- 2. sampling, hierarchy, skins: every read-back value within the model's bound ---------------------------------------------------
@pytest.mark.parametrize("name", RIG_NAMES)
def test_every_value_lies_within_the_bound(emu, rigs, name):
    rig, times = rigs[name]
    am.run_rig(emu, rig, times)


def test_fallbacks_are_counted(emu, rigs):
    got = am.run_rig(emu, rigs["zero quaternions"][0], [0.5])[0]
    assert got["status"]["rotation_fallbacks"] == 3 and got["status"]["inverse_fallbacks"] == 0
    assert np.array_equal(got["trs"][1:4, 3:7], np.tile(f32([0, 0, 0, 1]), (3, 1)))
    got = am.run_rig(emu, rigs["skin singular"][0], [0.9])[0]
    assert got["status"]["inverse_fallbacks"] == 1 and got["status"]["rotation_fallbacks"] == 0


def test_base_pose(emu, rigs):
    """animations[i] == RFWHIP_RIG_BASE_POSE, and a rig without animations whatever is asked: the base TRS and weights."""
    rig = rigs["sampling 4 keys"][0]
    emu.set_rig(0, rig)
    emu.animate(0, 0.7, None)
    got = am.read_all(emu, rig)
    am.check_against_model(got, rig, am.BASE_POSE, 0.7, serial=1)
    assert np.array_equal(got["trs"][:, :3], rig["nodes"]["translation"]) and got["status"]["animation"] == am.BASE_POSE
    bare = dict(rig, animations=rig["animations"][:0], channels=rig["channels"][:0], times=rig["times"][:0], values=rig["values"][:0])
    emu.set_rig(1, bare)
    emu.animate(1, 0.7, 5)
    assert np.array_equal(am.read_all(emu, bare, 1)["world"].view(np.uint32), got["world"].view(np.uint32))


# ---- 3. crowd ------------------------------------------------------------------------------------------------------------------------
def test_a_crowd_is_its_single_calls(make_emu, rigs):
    """Three rigs of different sizes in one call at different times: each rig's buffers equal those of its own call, bit for bit."""
    picks = [("skin 65", 0.9), ("hierarchy one", 0.7), ("hierarchy %d" % (am.LDS_NODES + 1), 1.1)]
    crowd, single = make_emu(), make_emu()
    for i, (name, _) in enumerate(picks):
        crowd.set_rig(i, rigs[name][0])
        single.set_rig(i, rigs[name][0])
    crowd.animate([2, 0, 1], [picks[2][1], picks[0][1], picks[1][1]], 0)
    for i, (name, t) in enumerate(picks):
        single.animate(i, t, 0)
        am.same_bits(am.read_all(crowd, rigs[name][0], i), am.read_all(single, rigs[name][0], i))
    with pytest.raises(RuntimeError, match="rig 1 is listed twice"):
        crowd.animate([0, 1, 1], [0.1, 0.2, 0.3], 0)
    with pytest.raises(RuntimeError, match="rig 7 has not been set"):
        crowd.animate([0, 7], 0.1, 0)
    with pytest.raises(RuntimeError, match="no animation 3"):
        crowd.animate(0, 0.1, 3)
    with pytest.raises(RuntimeError, match="not finite"):
        crowd.animate(0, np.inf, 0)
    crowd.destroy(), single.destroy()


# ---- 4. meshes that follow a rig ---------------------------------------------------------------------------------------------------
def test_animate_is_pose_mesh_with_the_read_back_matrices(pkg, make_emu):
    scene, a, b = am.animate_equals_pose(pkg, make_emu)
    # ... and a second frame, another time: still the same
    a.animate(0, 0.45)
    a.update()
    b.pose_mesh(0, a.read_rig(0, "joints", 0))
    b.update()
    am.same_scene_bits(pkg, scene, a, b)
    assert a.read_rig(0, "status")["serial"] == 2


def test_animate_is_morph_mesh_with_the_read_back_weights_and_lights_follow(pkg, make_emu):
    """The morph rig drives the emissive strip of test_moving_emitters.py under lights_follow_geometry=1: the area lights after
    animate + update equal those after morph_mesh with the read-back weights + update, byte for byte, and so does the image."""
    import test_moving_emitters as me
    scene = me.strip_scene(pkg)
    nv = len(scene.meshes[scene.strip_mesh]["vertices"])
    tp = (np.random.default_rng(5).normal(size=(2, nv, 3)) * 0.3).astype(f32)
    up = np.tile(f32([0.0, 1.0, 0.0]), (nv, 1))
    rig = am.strip_rig(pkg)
    ctxs = []
    for _ in range(2):
        c = me.ctx_on(make_emu, scene, lights=me.zeroed(scene.area_lights))
        c.set_setting("spp", 2)
        c.set_mesh_morph(scene.strip_mesh, up, tp, np.zeros_like(tp))
        ctxs.append(c)
    a, b = ctxs
    a.set_rig(0, rig)
    a.bind_rig(0, scene.strip_mesh, node=0)
    before = a.read_area_lights().tobytes()
    a.animate(0, 0.6)
    a.update()
    w = a.read_rig(0, "weights", 0)
    am.within(w, am.evaluate(rig, 0, 0.6)["weights"])
    assert np.abs(w).min() > 0.01
    b.morph_mesh(scene.strip_mesh, w)
    b.update()
    la, lb = a.read_area_lights(), b.read_area_lights()
    assert la.tobytes() == lb.tobytes() and la.tobytes() != before
    a.render_frame(scene.camera, pkg.RESET)
    b.render_frame(scene.camera, pkg.RESET)
    assert np.array_equal(a.framebuffer().view(np.uint32), b.framebuffer().view(np.uint32))


def test_binding_rules(pkg, make_emu, rigs):
    scene, (c,) = am.tube_contexts(pkg, make_emu, 1)
    with pytest.raises(RuntimeError, match="rig 0 has not been set"):
        c.bind_rig(0, 0)
    c.set_rig(0, am.tube_rig(pkg))
    c.set_rig(1, rigs["skin 1"][0])
    with pytest.raises(RuntimeError, match="refers to joint 1, skin 0 of rig 1 has 1 joints"):
        c.bind_rig(1, 0, skin=0)
    with pytest.raises(RuntimeError, match="no skin 4"):
        c.bind_rig(0, 0, skin=4)
    with pytest.raises(RuntimeError, match="neither a skin nor morph targets"):
        c.bind_rig(0, 1)
    c.bind_rig(0, 0, skin=0)
    c.set_rig(2, rigs["skin 65"][0])
    c.bind_rig(2, 0, skin=0)  # binding it again replaces the binding: rig 0 no longer moves the mesh
    org, d = am.tube_rays()
    before = c.trace_rays(org, d)
    c.animate(0, 1.4)
    c.update()
    assert np.array_equal(before["t"].view(np.uint32), c.trace_rays(org, d)["t"].view(np.uint32))
    c.bind_rig(0, 0, skin=0)
    c.animate(0, 1.4)
    c.update()
    assert not np.array_equal(before["t"].view(np.uint32), c.trace_rays(org, d)["t"].view(np.uint32))
    with pytest.raises(RuntimeError, match="has not been evaluated"):
        c.read_rig(1, "world")
    c.set_setting("stage_timing", 1)
    c.animate([0, 1], [0.2, 0.3])
    c.wait()
    assert c.get_kernel_time("rig")[1] == 1 and c.get_kernel_time(18)[0] >= 0.0
    c.destroy()


def test_a_loaded_scene_carries_its_rig(tmp_path, pkg, make_emu):
    """gltf.load_scene -> upload -> gltf.bind_scene -> animate(time): the joint matrices are gltf.py's at that time (the file of
    test_gltf.py: the mesh node translated, the joints beside it), within the model's bound, and the mesh moves."""
    from test_gltf import _write_tube_gltf
    path = tmp_path / "tube.gltf"
    _write_tube_gltf(path, pkg, 12, 10)
    scene, g, skins = pkg.gltf.load_scene(str(path), 48, 32)
    assert scene.rig is not None and scene.rig_bindings == {0: {"skin": 0}} and scene.rig["skin_of_node"] == {0: 0}
    scene.set_test_sky(16, 8)
    scene.camera = pkg.scenes.skinned_tube(0.0, rings=2, seg=3, width=48, height=32).camera
    c = make_emu()
    c.init(48, 32)
    scene.upload(c)
    assert pkg.gltf.bind_scene(c, scene)
    org, d = am.tube_rays()
    before = c.trace_rays(org, d)
    for t in (0.3, 1.7, 5.1):
        c.animate(0, t)
        c.update()
        got = c.read_rig(0, "joints", 0)
        am.within(got, am.evaluate(scene.rig, 0, t)["joints"][0])
        g.set_time(t)  # (from the file's doubles, at the double t, cast to float32: one u on the inputs, the time and the result)
        want = am.evaluate(scene.rig, 0, t, input_ulps=1, time_ulps=1)["joints"][0]
        want.e += am.U * np.abs(want.v)
        am.within(g.joint_matrices(0), want)
    assert not np.array_equal(before["t"], c.trace_rays(org, d)["t"])
    c.destroy()


# ---- 5. the fixtures ------------------------------------------------------------------------------------------------------------
def _fixture_rig(pkg, fx, name):
    dts = dict(pkg.abi.RIG_TABLES)
    return {k: (fx["%s/rig/%s" % (name, k)].view(dts[k]).reshape(-1) if dts[k] not in (np.float32, np.uint32) else fx["%s/rig/%s" % (name, k)])
            for k in dts}


def test_cesiumman_joint_matrices_of_the_asset_fixture(pkg, emu):
    """CesiumMan's rig at the three times of asset_cesiumman.npz gives that file's joint matrices within the model's bound.  That
    file holds float32 casts of values gltf.py computed from the file's own doubles, the rig holds their float32 roundings: one u
    of input error on the base values and on the time (the model's input_ulps, time_ulps) and one u for the recorded cast."""
    rig = _fixture_rig(pkg, np.load(os.path.join(GOLD, "asset_animation.npz")), "cesiumman")
    fx = np.load(os.path.join(GOLD, "asset_cesiumman.npz"))
    emu.set_rig(0, rig)
    for k, t in enumerate(fx["times"]):
        emu.animate(0, float(t))
        got = emu.read_rig(0, "joints", 0)
        am.within(got, am.evaluate(rig, 0, t)["joints"][0])
        want = am.evaluate(rig, 0, t, input_ulps=1, time_ulps=1)["joints"][0]
        want.e += am.U * np.abs(want.v)
        am.within(fx["joint_matrices"][k], want)
        assert np.abs(got - fx["joint_matrices"][k]).max() <= 2 * want.e.max()


def test_morph_cube_weights_of_the_asset_fixture(pkg, emu):
    """The weights channel of AnimatedMorphCube, with the rig built from the arrays of the animation fixture, gives the weights
    asset_morphcube.npz records at its four times (float32 casts of gltf.py's float64 values at times given as doubles, which the
    fixture holds as float32: one u on the time, one on the recorded value)."""
    rig = _fixture_rig(pkg, np.load(os.path.join(GOLD, "asset_animation.npz")), "morphcube")
    fm = np.load(os.path.join(GOLD, "asset_morphcube.npz"))
    node = int(np.nonzero(rig["nodes"]["weight_count"])[0][0])
    emu.set_rig(0, rig)
    for k, t in enumerate(fm["times"]):
        emu.animate(0, float(t))
        got = emu.read_rig(0, "weights", node)
        am.within(got, am.evaluate(rig, 0, t)["weights"])
        want = am.evaluate(rig, 0, t, time_ulps=1)["weights"]
        want.e += am.U * np.abs(want.v)
        am.within(fm["weights"][k], want)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def malformed(pkg):
    """(name, rig, words of the message): every refusal of rfwhip_set_rig."""
    good = am.sampling_rig(pkg, 4)

    def edit(table, index, field, value):
        r = {k: v.copy() for k, v in good.items()}
        if field is None:
            r[table][index] = value
        else:
            r[table][field][index] = value
        return r
    nan_time, flat_time = good["times"].copy(), good["times"].copy()
    nan_time[5], flat_time[6] = np.nan, flat_time[5]
    loop = {k: v.copy() for k, v in good.items()}
    loop["nodes"]["parent"][0], loop["nodes"]["parent"][3] = 3, 0
    no_weights = edit("nodes", 10, "weight_count", 0)
    twice = {k: v.copy() for k, v in good.items()}
    twice["channels"]["node"][1] = twice["channels"]["node"][0]
    return [("parent out of range", edit("nodes", 2, "parent", 99), ["node 2", "parent 99 out of range"]),
            ("parent below -1", edit("nodes", 2, "parent", -2), ["node 2", "parent -2"]),
            ("weights out of range", edit("nodes", 4, "weight_offset", 1000), ["node 4", "weights 1000 + 2 out of range"]),
            ("parent cycle", loop, ["parent cycle"]),
            ("self parent", edit("nodes", 5, "parent", 5), ["node 5", "parent cycle"]),
            ("mesh node out of range", edit("skins", 0, "mesh_node", 13), ["skin 0", "mesh node 13"]),
            ("skin without joints", edit("skins", 0, "joint_count", 0), ["skin 0 has no joints"]),
            ("joints out of range", edit("skins", 0, "joint_count", 13), ["skin 0", "joints 0 + 13 out of range"]),
            ("joint is no node", edit("joints", 3, None, 50), ["skin 0", "joint 3 is node 50"]),
            ("channel node out of range", edit("channels", 2, "node", 13), ["channel 2", "node 13 out of range"]),
            ("unknown path", edit("channels", 2, "path", 4), ["channel 2", "path 4"]),
            ("unknown method", edit("channels", 2, "method", 3), ["channel 2", "method 3"]),
            ("key_count 0", edit("channels", 7, "key_count", 0), ["channel 7", "key_count is 0"]),
            ("times out of range", edit("channels", 11, "time_offset", 46), ["channel 11", "key times 46 + 4 out of range"]),
            ("time not finite", dict(good, times=nan_time), ["channel 1", "key time 1 is not finite"]),
            ("time not increasing", dict(good, times=flat_time), ["channel 1", "key time 2 is not greater than its predecessor"]),
            ("value length", edit("channels", 2, "value_count", 35), ["channel 2", "35 values", "translation x CUBICSPLINE x 4 keys needs 36"]),
            ("values out of range", edit("channels", 11, "value_offset", 100000), ["channel 11", "values 100000 + 24 out of range"]),
            ("weights channel without weights", no_weights, ["channel 9", "weights channel on node 10, which has no weights"]),
            ("animation out of range", edit("animations", 0, "channel_count", 13), ["animation 0", "channels 0 + 13 out of range"]),
            ("two channels on one value", twice, ["channel 1", "another translation channel on node 1"])]


def test_malformed_rigs_are_refused_with_the_previous_rig_in_place(pkg, emu):
    good = am.sampling_rig(pkg, 4)
    emu.set_rig(0, good)
    emu.animate(0, 0.8)
    before = am.read_all(emu, good)
    cases = malformed(pkg)
    assert len(cases) >= 20
    for name, bad, words in cases:
        with pytest.raises(RuntimeError) as e:
            emu.set_rig(0, bad)
        assert "rfwhip_set_rig: rig 0:" in str(e.value) and all(w in str(e.value) for w in words), (name, str(e.value))
    emu.animate(0, 0.8)
    after = am.read_all(emu, good)
    assert after["status"].pop("serial") == 2 and before["status"].pop("serial") == 1
    am.same_bits(before, after)


# ---- 7. groups -------------------------------------------------------------------------------------------------------------------------
def test_group_of_emulated_contexts_equals_the_single_context(pkg, make_emu, emu_lib):
    scene, (single,) = am.tube_contexts(pkg, make_emu, 1)
    rig = am.tube_rig(pkg)
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0, 0], "peer")
    scene_g, (g,) = am.tube_contexts(pkg, lambda: g, 1)
    imgs = []
    for target in (single, g):
        target.set_rig(0, rig)
        target.bind_rig(0, 0, skin=0)
        target.animate(0, 1.4)
        target.update()
        target.render_frame(scene.camera, pkg.RESET)
        imgs.append(target.framebuffer())
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32))
    for c in g.contexts:
        assert c.read_rig(0, "status")["serial"] == 1
    with pytest.raises(RuntimeError, match="listed twice"):
        g.animate([0, 0], 0.1)
    # ... and the rig moved the mesh: the bind pose gives another image
    still = am.tube_contexts(pkg, make_emu, 1)[1][0]
    still.render_frame(scene.camera, pkg.RESET)
    assert not np.array_equal(still.framebuffer(), imgs[0])
    g.destroy()


# ---- 8. the sanitizers -----------------------------------------------------------------------------------------------------------------
def rig_file(pkg, rig, calls):
    """The stand-alone program's input: nine counts, the tables in abi.RIG_TABLES order, then (animation, time) pairs."""
    parts = [np.ascontiguousarray(rig[k], dtype=dt).reshape(-1) for k, dt in pkg.abi.RIG_TABLES]
    counts = [len(p) for p in parts]
    counts[4] = len(calls)  # (inverse_bind shares joints' count: its slot carries the number of calls)
    out = struct.pack("<9Q", *counts) + b"".join(p.tobytes() for p in parts)
    return out + b"".join(struct.pack("<If", a, t) for a, t in calls)


def test_sanitized_stand_alone_program(pkg, tmp_path, rigs):
    """The validator and the work items over exactly-sized heap arrays under AddressSanitizer and UBSan, in a child process."""
    gxx = shutil.which("g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if not gxx or subprocess.run([gxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ or its sanitizer runtime is not installed here")
    exe = tmp_path / "animation_san"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g"] + flags + ["-I" + os.path.join(ROOT, "rendering-fw_amd", "csrc"),
                        os.path.join(ROOT, "tests", "animation_san_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files, expect = [], []
    for k, (name, bad, _) in enumerate(malformed(pkg)):
        files.append(tmp_path / ("bad%02d.rig" % k))
        files[-1].write_bytes(rig_file(pkg, bad, [(0, 0.5)]))
        expect.append((name, 1))
    for k, name in enumerate(RIG_NAMES):
        rig, times = rigs[name]
        files.append(tmp_path / ("good%02d.rig" % k))
        files[-1].write_bytes(rig_file(pkg, rig, [(0, t) for t in times] + [(am.BASE_POSE, 0.0)]))
        expect.append((name, 0))
    r = subprocess.run([str(exe)] + [str(f) for f in files], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files) + 1 and lines[-1] == "done"
    for line, (name, code) in zip(lines, expect):
        assert int(line.split()[1]) == code, (name, line)
