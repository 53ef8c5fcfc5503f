"""Moving emitters on the MI355X (k_light_refresh, k_lt_refit_level, k_lt_refit_top): the checks of tests/test_moving_emitters.py
on the device — the refreshed lights against the float64 model and, byte for byte, against the emulation (the work item has a
fixed shape: no library function, no contraction), the refit through the hook with the emulation's allowance, picking on the
refit tree, scheduling, the strict build against the strict emulation, and a two-context group."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
import test_moving_emitters as cpu
from test_moving_emitters import MOVE, SEQ_BASE, SIZES, check_picking, check_refit, check_refreshed, ctx_on, lamp_scene, move_lamp, refit_case, sequence, zeroed

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


def _rays(c):
    st = c.get_stats()
    return (st.primaryCount, st.secondaryCount, st.deepCount, st.shadowCount)


@pytest.mark.parametrize("n", SIZES)
def test_refresh_known_answer(pkg, make_hip, make_emu, n):
    scene = lamp_scene(pkg, n)
    scene.instances[scene.lamp_inst]["transform"] = MOVE
    given = zeroed(scene.area_lights)
    c = ctx_on(make_hip, scene, lights=given)
    got = c.read_area_lights()
    check_refreshed(got, given, scene, n)
    assert c.get_setting("lights_bound") == "%d" % n
    # the emulation's bytes: products and sums of a fixed shape, an IEEE square root
    assert ctx_on(make_emu, scene, lights=given).read_area_lights().tobytes() == got.tobytes()


def test_binding_rules_and_animation(pkg, make_hip):
    cpu.test_binding_rules(pkg, make_hip)
    cpu.test_lights_follow_pose_morph_and_instance(pkg, make_hip)


def test_off_means_off(pkg, make_hip):
    cpu.test_off_means_off(pkg, make_hip)


@pytest.mark.parametrize("mode", ["reference", "linear"])
def test_same_bytes_same_image(pkg, make_hip, mode):
    cpu.test_same_bytes_same_image(pkg, make_hip, mode)


@pytest.mark.parametrize("mode", ["reference", "linear"])
@pytest.mark.parametrize("kind", ["pose", "morph"])
def test_light_area_is_the_shading_record_area_after_a_deformation(pkg, make_hip, kind, mode):
    cpu.test_light_area_is_the_shading_record_area_after_a_deformation(pkg, make_hip, kind, mode)


@pytest.mark.parametrize("n", SIZES)
def test_refit_known_answer(pkg, make_hip, n):
    """The hook on the device, every n: the emulation's allowance (never one measured here)."""
    scene = lamp_scene(pkg, n)
    c = ctx_on(make_hip, scene, light_sampling="tree")
    nodes, area, bound = refit_case(pkg, c, scene, n)
    after = c.light_tree_refit(nodes, area, bound)
    excess = check_refit(nodes, after, area, bound, n, cpu.EXCESS_ALLOWED)
    print("n = %d: largest excess of a refitted cone over the float64 pairwise union on the device: %.3e rad (allowed %.3e)" % (n, excess, cpu.EXCESS_ALLOWED))
    assert c.light_tree_refit(nodes, area, bound).tobytes() == after.tobytes()


@pytest.mark.parametrize("strict", [False, True])
def test_picking_is_consistent_on_a_refit_tree(pkg, make_hip, strict):
    make = (lambda: pkg._binding.CoreBinding(_strict_hip(), "rfwhip_", 0, 0, 1)) if strict else make_hip
    scene, c = cpu.moved_tree_ctx(pkg, make, 65)
    assert check_picking(pkg, scene, c, 65) > 1000


def test_tree_after_refit_and_linear_have_the_same_expectation(pkg, make_hip):
    cpu.test_tree_after_refit_and_linear_have_the_same_expectation(pkg, make_hip)


def test_scheduling_changes_no_bit(pkg, make_hip):
    """render, move, update, render with frames in flight, under ring 1 / 2 / 4, streams 1 / 4, fuse 0 / 1, shadow_packets 0 / 1"""
    scene = lamp_scene(pkg, 65)
    refs = {}
    for extra in cpu.SEQ_MATRIX:
        settings = dict(SEQ_BASE, **extra)
        spp = settings["spp"]
        c = make_hip()
        img, rays = sequence(pkg, c, scene, settings, False)
        if spp not in refs:
            refs[spp] = sequence(pkg, make_hip(), scene, dict(SEQ_BASE, spp=spp, ring=1, streams=1), True)
        assert np.array_equal(img, refs[spp][0]) and rays == refs[spp][1], extra
        assert c.get_setting("light_tree_refits") == "1" and c.get_setting("lights_bound") == "65"


@pytest.mark.parametrize("mode", ["tree", "linear"])
def test_strict_hip_equals_strict_emulation_after_a_move(pkg, emu_strict_lib, mode):
    w, h = 96, 64
    out = []
    for lib in (_strict_hip(), emu_strict_lib):
        scene = lamp_scene(pkg, 65, w, h)
        c = ctx_on(lambda: pkg._binding.CoreBinding(lib, "rfwhip_", 0, 0, 1), scene, spp=8, max_depth=2, light_sampling=mode)
        move_lamp(c, scene, cpu.trs((0.3, 1.0, 0.2), 140.0, (1.0, 1.0, 1.0), (-2.5, 0.5, 1.5)))
        c.render_frame(scene.camera, pkg.RESET)
        tree = c.get_light_tree()[0].tobytes() if mode == "tree" else b""
        out.append((c.framebuffer(), _rays(c), c.read_area_lights().tobytes(), tree, c.get_setting("light_tree_refits")))
    hip, emu = out
    assert hip[4] == emu[4] == ("1" if mode == "tree" else "0")
    assert hip[2] == emu[2] and hip[3] == emu[3]
    differing = int((hip[0] != emu[0]).any(-1).sum())
    print("%s: strict HIP vs strict emulation after a move: %d of %d pixels differ; ray counts %s / %s" % (mode, differing, w * h, hip[1], emu[1]))
    assert differing == 0 and hip[1] == emu[1] and hip[0][..., :3].mean() > 1e-3


def test_two_context_group_on_one_device(pkg, make_hip):
    scene = lamp_scene(pkg, 65, 70, 51)
    ref, _ = sequence(pkg, make_hip(), scene, SEQ_BASE, False)
    g = pkg.render_group([0, 0], "peer")
    img, _ = sequence(pkg, g, scene, SEQ_BASE, False)
    lights = [c.read_area_lights().tobytes() for c in g.contexts]
    assert lights[0] == lights[1] and lights[0] != scene.area_lights.tobytes()
    assert [c.get_setting("lights_bound") for c in g.contexts] == ["65", "65"]
    assert [c.get_setting("light_tree_refits") for c in g.contexts] == ["1", "1"]
    g.destroy()
    assert np.array_equal(img, ref)
