"""Colour grading and dither on the device (k_display_graded, k_kat_grade; work items: csrc/display_grade.h): the CPU tier's known
answers on the HIP kernels, held to the same float64 model (tests/display_grade_model.py) within the same counted bounds — the
kernels and the emulation are each held to the model, not to each other.  Then one 1920 x 1080 frame with everything on, a group of
two contexts on one device, and the strict-arithmetic build against its emulation."""
import ctypes
import os

import numpy as np
import pytest

import display_grade_checks as ck
import display_grade_model as gm
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_defaults_equal_the_ungraded_bytes(make_hip):
    c = make_hip()
    c.init(70, 21)
    ck.defaults_are_the_ungraded_bytes(c, 70, 21)
    c.init(130, 35)
    ck.defaults_are_the_ungraded_bytes(c, 130, 35)


@pytest.mark.parametrize("size", gm.SIZES, ids=lambda s: "%dx%d" % s)
def test_stage_matches_the_model(make_hip, size):
    w, h = size
    c = make_hip()
    c.init(w, h)
    for name, ev in gm.VARIANTS:
        ck.stage_matches_the_model(c, w, h, name, ev)


def test_grade_colors(make_hip):
    c = make_hip()
    c.init(4, 4)
    ck.linear_known_answers(c)
    for n in (2, 3, 17, 33, 65):
        ck.lut_known_answers(c, n)


def test_lut_with_entries_outside_the_unit_cube(make_hip):
    c = make_hip()
    c.init(67, 19)
    ck.lut_outside_the_unit_cube(c, 67, 19)


def test_white_balance_maps_the_white_of_T_to_the_white_of_6500(make_hip):
    c = make_hip()
    c.init(4, 4)
    ck.white_balance_maps_white_to_white(c)


def test_dither(make_hip):
    c = make_hip()
    c.init(48, 32)
    ck.dither_known_answers(c)


def test_full_frame_with_everything_on(pkg, make_hip):
    """One 1920 x 1080 frame through read_display: grade, a 33^3 LUT, dither, auto exposure and bloom together.  The meter and bloom
    see the ungraded image: the model grades what rfwhip_bloom_image returns for the framebuffer under the meter's E."""
    w, h = 1920, 1080
    scene = pkg.scenes.cornell(w, h)
    c = make_hip()
    c.init(w, h)
    scene.upload(c)
    for k, v in (("integrator", "pt"), ("spp", 1), ("max_depth", 2)):
        c.set_setting(k, v)
    c.render_frame(scene.camera, pkg.RESET)
    ck.reset(c)
    g = gm.Grade(temperature=5200.0, slope=(1.1, 0.95, 1.05), offset=(0.01, 0.0, -0.02), power=(0.95, 1.0, 1.08), saturation=0.8,
                 lut=gm.look_lut(33), dither=1)
    g.apply(c)
    for k, v in (("display_grade", 1), ("display_exposure", "auto"), ("display_bloom", 1), ("display_fxaa", 0)):
        c.set_setting(k, v)
    b, k = scene.camera.brightness, scene.camera.contrast
    f32 = c.display("rgba32f")
    u8 = c.display("rgba8")  # (the same frame: no further step of the meter)
    E = c.meter()["exposure"]
    assert c.meter()["steps"] == 1 and E != 1.0
    bloomed = c.bloom_image(c.framebuffer(), E)
    model = gm.graded_texels(bloomed, g, E, b, k)
    share = gm.judge_pointwise(f32, bloomed, g, label="1080p rgba32f", texels=model)
    near = gm.judge_pointwise(u8, bloomed, g, label="1080p rgba8", texels=model)
    print("1920x1080: largest float deviation %.3f of the bound, %.3f %% of the bytes near a boundary" % (share, 100 * near))
    c.set_setting("display_fxaa", 1)
    a = np.clip(bloomed[..., 3], 0.0, 1.0)
    gm.judge_fxaa(c.display("rgba8"), f32[..., :3], a, g, label="1080p fxaa rgba8")


def test_group_of_two_on_one_device(pkg):
    lib = pkg.context.load_library()
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    g = gm.case("all")
    settings = dict(g.settings(), display_grade=1, display_exposure="auto", display_bloom=1, integrator="pt", spp=4, max_depth=2)

    def render(x):
        x.init(70, 51)
        scene.upload(x)
        for k, v in settings.items():
            x.set_setting(k, v)
        x.set_display_lut(g.lut)
        x.render_frame(scene.camera, pkg.RESET)
    one = pkg.RenderContext(device=0)
    render(one)
    want8, want32 = one.display("rgba8"), one.display("rgba32f")
    grp = pkg._binding.RenderGroup(lib, "rfwhip_", [0, 0], "peer")
    render(grp)
    assert np.array_equal(grp.display("rgba8"), want8)
    grp.present_display_async(0, "rgba32f")
    grp.present_display_async(1, "rgba8")
    assert np.array_equal(grp.present_display_wait(0).view(np.uint32), want32.view(np.uint32))
    assert np.array_equal(grp.present_display_wait(1), want8)
    grp.destroy()


def test_strict_hip_equals_strict_emulation_bit_for_bit(pkg):
    """The strict-arithmetic build (tests/test_strict_gpu.py's libraries) for the graded kernel: white balance, saturation, LUT, FXAA
    and dither, both formats.  CDL and the sRGB encoding call powf, which rt_strict_math.h does not restate: they stay out."""
    import build_emu
    from test_strict_gpu import STRICT_FLAGS
    strict_so = os.path.join(ROOT, "tests", "_strict", "librfwhip_strict.so")
    assert os.path.exists(strict_so), "build it with __graft_entry__.build() (build.py: build_strict)"
    libs = [ctypes.CDLL(strict_so), ctypes.CDLL(build_emu.build(defines=STRICT_FLAGS, tag="_strict"))]
    img = gm.image(130, 35)
    g = gm.Grade(temperature=4300.0, saturation=1.3, lut=gm.look_lut(17), dither=1)
    out = []
    for lib in libs:
        c = pkg._binding.CoreBinding(lib, "rfwhip_", 0, 0, 1)
        c.init(130, 35)
        ck.reset(c)
        g.apply(c)
        c.set_setting("display_grade", 1)
        c.set_setting("display_exposure_ev", 1)
        out.append((c.display_image(img, 0.05, 1.0, "rgba8"), c.display_image(img, 0.05, 1.0, "rgba32f")))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
