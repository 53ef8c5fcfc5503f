"""Animations on the HIP kernel (csrc/animation.h, k_rig_evaluate, kernel family 18): the rigs and checks of tests/test_animation.py
through the shipped library — every value within the model's bound, and bit-equal to the host emulation, which the header's fixed
shapes promise for every value it writes — and through the validation build against the emulation built the same way."""
import ctypes
import os

import numpy as np
import pytest

import animation_model as am
from conftest import ROOT
from test_animation import RIG_NAMES, _fixture_rig

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
STRICT_FLAGS = ("-DRT_STRICT_MATH", "-ffp-contract=off")


@pytest.fixture(scope="module")
def rigs(pkg):
    return am.all_rigs(pkg)


@pytest.fixture(scope="module")
def emu_strict_lib():
    import build_emu
    return ctypes.CDLL(build_emu.build(defines=STRICT_FLAGS, tag="_strict"))


def _strict_hip(pkg):
    so = os.path.join(ROOT, "tests", "_strict", "librfwhip_strict.so")
    assert os.path.exists(so), "build it with __graft_entry__.build() (build.py: build_strict)"
    return pkg._binding.CoreBinding(ctypes.CDLL(so), "rfwhip_", 0, 0, 1)


GROUPS = {"sampling": RIG_NAMES[:6], "hierarchy": RIG_NAMES[6:14], "skins": RIG_NAMES[14:]}


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_value_lies_within_the_bound_and_equals_the_emulation(pkg, make_hip, make_emu, emu_strict_lib, rigs, group):
    hip, emu, strict = make_hip(), make_emu(), _strict_hip(pkg)
    strict_emu = pkg._binding.CoreBinding(emu_strict_lib, "rfwhip_", 0, 0, 1)
    for name in GROUPS[group]:
        rig, times = rigs[name]
        got = am.run_rig(hip, rig, times)  # (asserts the bound and the status record at every time)
        for a, b in zip(got, am.run_rig(emu, rig, times)):
            am.same_bits(a, b)
        for c in (strict, strict_emu):
            c.set_rig(0, rig)
        for t in times:
            strict.animate(0, t)
            strict_emu.animate(0, t)
            am.same_bits(am.read_all(strict, rig), am.read_all(strict_emu, rig))
    for c in (hip, emu, strict, strict_emu):
        c.destroy()


def test_a_crowd_is_its_single_calls(make_hip, rigs):
    picks = [("skin 65", 0.9), ("hierarchy one", 0.7), ("hierarchy %d" % (am.LDS_NODES + 1), 1.1)]
    crowd, single = make_hip(), make_hip()
    for i, (name, _) in enumerate(picks):
        crowd.set_rig(i, rigs[name][0])
        single.set_rig(i, rigs[name][0])
    crowd.animate([2, 0, 1], [picks[2][1], picks[0][1], picks[1][1]], 0)
    for i, (name, t) in enumerate(picks):
        single.animate(i, t, 0)
        am.same_bits(am.read_all(crowd, rigs[name][0], i), am.read_all(single, rigs[name][0], i))
    with pytest.raises(RuntimeError, match="rig 1 is listed twice"):
        crowd.animate([0, 1, 1], [0.1, 0.2, 0.3], 0)
    crowd.destroy(), single.destroy()


def test_sixty_four_rigs_in_one_call(make_hip, rigs):
    """64 copies of a rig at 64 times in one launch; rigs 0, 31 and 63 equal their single calls bit for bit."""
    rig = rigs["skin animated"][0]
    crowd, single = make_hip(), make_hip()
    times = np.linspace(0.05, 4.9, 64).astype(np.float32)
    for i in range(64):
        crowd.set_rig(i, rig)
    single.set_rig(0, rig)
    crowd.set_setting("stage_timing", 1)
    crowd.animate(np.arange(64), times, 0)
    crowd.wait()
    assert crowd.get_kernel_time("rig")[1] == 1
    for i in (0, 31, 63):
        single.animate(0, float(times[i]), 0)
        a, b = am.read_all(crowd, rig, i), am.read_all(single, rig, 0)
        b["status"]["serial"] = 1
        am.same_bits(a, b)
        am.check_against_model(a, rig, 0, float(times[i]), serial=1)
    crowd.destroy(), single.destroy()


def test_animate_is_pose_mesh_with_the_read_back_matrices(pkg, make_hip):
    am.animate_equals_pose(pkg, make_hip)


def test_cesiumman_animated_from_the_fixture(pkg, make_hip):
    """CesiumMan at the asset fixture's three times: the joint matrices within the model's bound, and the animated geometry is the
    geometry rfwhip_pose_mesh makes of the same matrices: the same hits on a fan of rays, bit for bit."""
    from test_assets import _rig_scene
    rig = _fixture_rig(pkg, np.load(os.path.join(GOLD, "asset_animation.npz")), "cesiumman")
    fx = np.load(os.path.join(GOLD, "asset_cesiumman.npz"))
    w, h = 96, 128
    scene = _rig_scene(pkg, fx["positions"], fx["normals"], fx["indices"], fx["node_transform"], w, h)
    ctxs = []
    for _ in range(2):
        c = make_hip()
        c.init(w, h)
        scene.upload(c)
        c.set_mesh_skin(0, fx["joints"], fx["weights"], fx["normals"])
        ctxs.append(c)
    a, b = ctxs
    a.set_rig(0, rig)
    a.bind_rig(0, 0, skin=0)
    t = np.asarray(fx["node_transform"], np.float64)
    world = (t[:3, :3] @ fx["positions"].T.astype(np.float64)).T + t[:3, 3]
    lo, hi = world.min(0), world.max(0)
    ys, xs = np.meshgrid(np.linspace(lo[1], hi[1], 32), np.linspace(lo[0], hi[0], 20), indexing="ij")
    target = np.stack([xs.reshape(-1), ys.reshape(-1), np.full(xs.size, 0.5 * (lo[2] + hi[2]))], 1)
    org = np.tile(np.array([0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), lo[2] - 3.0 * (hi[1] - lo[1])]), (len(target), 1))
    d = target - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for k, time in enumerate(fx["times"]):
        a.animate(0, float(time))
        a.update()
        mats = a.read_rig(0, "joints", 0)
        am.within(mats, am.evaluate(rig, 0, time)["joints"][0])
        want = am.evaluate(rig, 0, time, input_ulps=1, time_ulps=1)["joints"][0]
        want.e += am.U * np.abs(want.v)
        am.within(fx["joint_matrices"][k], want)
        b.pose_mesh(0, mats)
        b.update()
        ha, hb = a.trace_rays(org, d), b.trace_rays(org, d)
        assert (ha["prim"] >= 0).sum() > 100
        for key in ha:
            assert np.array_equal(ha[key].view(np.uint32), hb[key].view(np.uint32)), (key, k)
    a.destroy(), b.destroy()
