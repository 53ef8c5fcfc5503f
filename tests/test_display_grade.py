"""Colour grading and dither of the display stage (include/rfwhip.h, rfwhip_set_display_lut; csrc/display_grade.h), CPU tier: the
host-emulation build runs the work items of the HIP kernels.  Held to the float64 model of tests/display_grade_model.py within its
counted bounds, to the settings contract, and to the single context for groups."""
import ctypes

import numpy as np
import pytest

import display_grade_checks as ck
import display_grade_model as gm


def test_model_inputs_stay_inside_the_cap():
    """By the model alone: the seeded images hold the values the issue asks for, and for every case and size at most 1 % of the
    byte decisions lie within the counted bound of a boundary (judge_pointwise asserts the same in front of every comparison)."""
    for w, h in gm.SIZES[1:]:
        img = gm.test_image(w, h)
        assert np.isnan(img).sum() == 1 and np.isposinf(img).sum() == 1 and (img[..., :3] < 0).sum() == 1
        if w * h > 1000:
            assert np.nanmax(np.where(np.isfinite(img[..., :3]), img[..., :3], 0)) > 100.0
        for name, ev in gm.VARIANTS:
            for srgb_on in (False, True):
                share = gm.near_share(img, gm.case(name), None if ev == 0 else 2.0 ** ev, srgb_on)
                assert share <= gm.MAX_NEAR, (name, ev, srgb_on, w, h, share)
    assert np.abs(gm.wb_matrix(6500.0) - np.eye(3)).max() < 1e-15  # (an almost-identity: the host sets the flag instead)
    B = gm.bayer(16, 16)
    assert sorted(B.ravel()) == list(range(256))


def test_defaults_equal_the_ungraded_bytes(make_emu):
    c = make_emu()
    c.init(70, 21)
    ck.defaults_are_the_ungraded_bytes(c, 70, 21)


@pytest.mark.parametrize("size", gm.SIZES, ids=lambda s: "%dx%d" % s)
def test_stage_matches_the_model(make_emu, size):
    w, h = size
    c = make_emu()
    c.init(w, h)
    for name, ev in gm.VARIANTS:
        ck.stage_matches_the_model(c, w, h, name, ev)


def test_grade_colors_linear(make_emu):
    c = make_emu()
    c.init(4, 4)
    ck.linear_known_answers(c)


@pytest.mark.parametrize("n", [2, 3, 17, 33, 65])
def test_grade_colors_lut(make_emu, n):
    c = make_emu()
    c.init(4, 4)
    ck.lut_known_answers(c, n)


def test_lut_with_entries_outside_the_unit_cube(make_emu):
    c = make_emu()
    c.init(67, 19)
    ck.lut_outside_the_unit_cube(c, 67, 19)


def test_white_balance_maps_the_white_of_T_to_the_white_of_6500(make_emu):
    c = make_emu()
    c.init(4, 4)
    ck.white_balance_maps_white_to_white(c)


def test_dither(make_emu):
    c = make_emu()
    c.init(48, 32)
    ck.dither_known_answers(c)


def test_cube_parser(pkg, make_emu, tmp_path):
    c = make_emu()
    L = gm.random_lut(5)
    path = str(tmp_path / "look.cube")
    pkg.lut.write_cube(path, L, title="a look")
    c.load_cube(path)
    assert np.array_equal(c.get_display_lut().view(np.uint32), L.view(np.uint32))
    assert c.get_setting("display_lut") == "5"
    text = pkg.lut.cube_text(L)
    c.set_display_lut_cube("# a comment\n\n" + text.replace("DOMAIN_MIN 0 0 0\n", "").replace("DOMAIN_MAX 1 1 1\n", "") + "  \n")
    assert np.array_equal(c.get_display_lut(), L)
    body = "\n".join(text.split("\n")[4:])
    for bad, why in ((body, "in front of LUT_3D_SIZE"), ("# nothing\nTITLE \"empty\"\n", "no LUT_3D_SIZE"),
                     ("LUT_1D_SIZE 5\n" + body, "1D"),
                     ("LUT_3D_SIZE 5\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 2 2 2\n" + body, "domain"),
                     ("LUT_3D_SIZE 5\nDOMAIN_MIN -1 0 0\n" + body, "domain"),
                     ("LUT_3D_SIZE 5\n" + "\n".join(body.split("\n")[1:]), "124 entries"),
                     ("LUT_3D_SIZE 5\n" + body + "0 0 0\n", "more than"),
                     ("LUT_3D_SIZE 1\n0 0 0\n", "[2, 65]"),
                     ("LUT_3D_SIZE 66\n", "[2, 65]"),
                     ("LUT_3D_SIZE 5\nLUT_3D_SIZE 5\n" + body, "once"),
                     ("LUT_3D_SIZE 5\nLUT_3D_INPUT_RANGE 0 1\n" + body, "not a keyword"),
                     ("LUT_3D_SIZE 5\n" + body.replace("\n", " 1\n", 1), "three numbers"),
                     ("LUT_3D_SIZE 2\n" + "0 0 nan\n" * 8, "not finite")):
        with pytest.raises(RuntimeError) as e:
            c.set_display_lut_cube(bad)
        assert why in str(e.value), (why, str(e.value))
        assert np.array_equal(c.get_display_lut(), L)  # the old LUT stays


def test_lut_state(make_emu):
    c = make_emu()
    c.init(33, 9)
    ck.reset(c)
    img = gm.image(33, 9)
    assert c.get_display_lut() is None and c.get_setting("display_lut") == "0"
    c.set_setting("display_grade", 1)
    plain = c.display_image(img, 0.05, 1.0, "rgba8")
    L = gm.look_lut(9)
    c.set_display_lut(L)
    assert np.array_equal(c.get_display_lut(), L) and c.get_setting("display_lut") == "9"
    assert not np.array_equal(c.display_image(img, 0.05, 1.0, "rgba8"), plain)
    for bad in (np.full((2, 2, 2, 3), np.inf, np.float32), np.full((2, 2, 2, 3), np.nan, np.float32), np.zeros((66, 66, 66, 3), np.float32), np.zeros(3, np.float32)):
        with pytest.raises(RuntimeError):
            c.set_display_lut(bad)
        assert np.array_equal(c.get_display_lut(), L)
    c.init(33, 9)  # the LUT belongs to the context, not to the render target
    assert np.array_equal(c.get_display_lut(), L)
    c.set_display_lut(None)
    assert c.get_display_lut() is None
    assert np.array_equal(c.display_image(img, 0.05, 1.0, "rgba8"), plain)
    # display_grade = 0: the LUT is not applied
    c.set_display_lut(L)
    c.set_setting("display_grade", 0)
    assert np.array_equal(c.display_image(img, 0.05, 1.0, "rgba8"), plain)


def _render(pkg, c, scene, w, h, **settings):
    c.init(w, h)
    scene.upload(c)
    for k, v in dict(settings, integrator="pt", spp=4, max_depth=2).items():
        c.set_setting(k, v)
    c.render_frame(scene.camera, pkg.RESET)


@pytest.mark.parametrize("n", [2, 3])
def test_group_equals_the_single_context(pkg, make_emu, emu_lib, n):
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    g = gm.case("all")
    settings = dict(g.settings(), display_grade=1, display_exposure="auto", display_bloom=1)
    one = make_emu()
    _render(pkg, one, scene, 70, 51, **settings)
    one.set_display_lut(g.lut)
    want8, want32 = one.display("rgba8"), one.display("rgba32f")
    grp = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0] * n, "peer")
    _render(pkg, grp, scene, 70, 51, **settings)
    grp.set_display_lut(g.lut)
    assert np.array_equal(grp.contexts[0].get_display_lut(), g.lut) and grp.contexts[1].get_display_lut() is None  # root only
    assert np.array_equal(grp.display("rgba8"), want8)
    grp.present_display_async(0, "rgba32f")
    assert np.array_equal(grp.present_display_wait(0).view(np.uint32), want32.view(np.uint32))
    grp.set_display_lut_cube(pkg.lut.cube_text(gm.look_lut(3)))
    assert grp.contexts[0].get_setting("display_lut") == "3"
    grp.destroy()


def test_settings_and_errors(make_emu, emu_lib):
    c = make_emu()
    defaults = {"display_grade": "0", "display_wb_temperature": "6500", "display_grade_slope": "1 1 1", "display_grade_offset": "0 0 0",
                "display_grade_power": "1 1 1", "display_grade_saturation": "1", "display_dither": "0", "display_lut": "0"}
    for k, v in defaults.items():
        assert c.get_setting(k) == v, k
    for key, bad in (("display_grade", "2"), ("display_grade", "on"), ("display_dither", ""), ("display_dither", "yes"),
                     ("display_wb_temperature", "1666"), ("display_wb_temperature", "25001"), ("display_wb_temperature", "warm"),
                     ("display_wb_temperature", "nan"), ("display_wb_temperature", ""),
                     ("display_grade_slope", "-0.1"), ("display_grade_slope", "1 2"), ("display_grade_slope", "1 2 3 4"),
                     ("display_grade_slope", "inf"), ("display_grade_slope", "1 x 1"), ("display_grade_slope", ""),
                     ("display_grade_offset", "nan"), ("display_grade_offset", "0 0 inf"), ("display_grade_offset", "0,0,0"),
                     ("display_grade_power", "0"), ("display_grade_power", "1 -1 1"), ("display_grade_power", "inf"),
                     ("display_grade_saturation", "-0.01"), ("display_grade_saturation", "4.5"), ("display_grade_saturation", "nan"),
                     ("display_grade_saturation", "")):
        with pytest.raises(RuntimeError) as e:
            c.set_setting(key, bad)
        assert key + " must" in str(e.value), (key, bad, str(e.value))
        assert c.get_setting(key) == defaults[key], (key, bad)
    for key in ("display_lut", "display_grade_time"):
        with pytest.raises(RuntimeError):
            c.set_setting(key, "1")
    c.set_setting("display_grade_slope", "1.5")
    assert c.get_setting("display_grade_slope") == "1.5 1.5 1.5"
    c.set_setting("display_grade_offset", " 0.1  -0.2\t0 ")
    assert c.get_setting("display_grade_offset") == "0.1 -0.2 0"
    c.set_setting("display_wb_temperature", "1667")
    c.set_setting("display_wb_temperature", "25000")
    assert not any(k.startswith("display") for k in c.get_settings())
    # state: the hook needs a render target; a LUT does not
    cols = np.zeros((2, 3), np.float32)
    with pytest.raises(RuntimeError, match="no render target"):
        c.grade_colors(0, cols)
    c.set_display_lut(gm.look_lut(2))
    c.init(4, 4)
    with pytest.raises(RuntimeError, match="which must be"):
        c.grade_colors(2, cols)
    assert np.array_equal(c.grade_colors(1, np.float32([[np.nan, 2.0, -1.0]])), gm.look_lut(2)[0, 1, 0][None])  # clamped to the lattice
    lib = emu_lib
    fn = lib.rfwhip_grade_colors
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    assert fn(c._ctx, 0, 2, None, cols.ctypes.data) != 0 and fn(None, 0, 2, cols.ctypes.data, cols.ctypes.data) != 0
    assert fn(c._ctx, 0, 0, None, None) == 0
    get = lib.rfwhip_get_display_lut
    get.restype, get.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    small = np.zeros(5, np.float32)
    assert get(c._ctx, small.ctypes.data, small.size, None) != 0  # room for 5 floats, the LUT holds 24
    # stage_timing: the graded kernel is family 13
    c.set_setting("stage_timing", 1)
    c.set_setting("display_grade", 1)
    c.display_image(np.zeros((4, 4, 4), np.float32))
    c.wait()
    assert c.get_kernel_time("grade")[1] == 1 and c.get_kernel_time("display")[1] == 0
    assert c.get_setting("display_grade_time").split()[1] == "1"
