"""Colour grading through the plugin's virtual interface (tests/plugin/grade_host.cpp, compiled here): with RFWHIP_GRADE=1 and a
.cube file the test writes, the bytes hiprtReadDisplay returns are the bytes the Python host shows for the linear image the C ABI
gives for the same frame under the same settings; with the variables unset they are the ungraded display bytes; a value a variable
does not have, or a file that is not there, is refused."""
import os

import numpy as np
import pytest

import display_grade_model as gm
from plugin_hosts import build_host, run_host

pytestmark = pytest.mark.gpu
VARS = ("RFWHIP_GRADE", "RFWHIP_GRADE_TEMPERATURE", "RFWHIP_GRADE_SATURATION", "RFWHIP_GRADE_LUT", "RFWHIP_DITHER", "RFWHIP_BLOOM", "RFWHIP_EXPOSURE")


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    return build_host(pkg, tmp_path_factory, "grade_host")


def _run(host, out, **env):
    return run_host(host, out, drop=VARS, RFWHIP_DISPLAY="aces", **env)


def _images(r, out):
    assert r.returncode == 0, (r.stdout, r.stderr)
    w, h = (int(v) for v in r.stdout.split()[1:3])
    plugin = np.fromfile(os.path.join(out, "plugin.rgba8"), np.uint8).reshape(h, w, 4)
    plain = np.fromfile(os.path.join(out, "abi.rgba8"), np.uint8).reshape(h, w, 4)
    linear = np.fromfile(os.path.join(out, "abi.f32"), np.float32).reshape(h, w, 4)
    return plugin, plain, linear


def test_plugin_presents_the_python_hosts_bytes(pkg, make_hip, host, tmp_path):
    cube = str(tmp_path / "look.cube")
    pkg.lut.write_cube(cube, gm.look_lut(17), title="look")
    plugin, plain, linear = _images(_run(host, tmp_path, RFWHIP_GRADE="1", RFWHIP_GRADE_TEMPERATURE="4800", RFWHIP_GRADE_SATURATION="1.25",
                                         RFWHIP_GRADE_LUT=cube, RFWHIP_DITHER="1"), tmp_path)
    assert not np.array_equal(plugin, plain)
    h, w = linear.shape[:2]
    c = make_hip()
    c.init(w, h)
    for k, v in (("display_grade", 1), ("display_wb_temperature", 4800), ("display_grade_saturation", 1.25), ("display_dither", 1)):
        c.set_setting(k, v)
    c.load_cube(cube)
    assert np.array_equal(c.display_image(linear, 0.05, 1.0, "rgba8"), plugin)


@pytest.mark.parametrize("env", [{}, {"RFWHIP_GRADE": "0", "RFWHIP_DITHER": "0"}], ids=["unset", "0"])
def test_plugin_without_the_variables_is_unchanged(host, tmp_path, env):
    plugin, plain, _ = _images(_run(host, tmp_path, **env), tmp_path)
    assert np.array_equal(plugin, plain)


@pytest.mark.parametrize("env, text", [({"RFWHIP_GRADE": "yes"}, 'RFWHIP_GRADE must be "0" or "1"'),
                                       ({"RFWHIP_DITHER": "2"}, 'RFWHIP_DITHER must be "0" or "1"'),
                                       ({"RFWHIP_GRADE_TEMPERATURE": "900"}, "display_wb_temperature must"),
                                       ({"RFWHIP_GRADE_SATURATION": "9"}, "display_grade_saturation must"),
                                       ({"RFWHIP_GRADE_LUT": "/nonexistent/look.cube"}, "cannot read")],
                         ids=["grade", "dither", "temperature", "saturation", "lut"])
def test_plugin_refuses_what_the_settings_refuse(host, tmp_path, env, text):
    r = _run(host, tmp_path, **env)
    assert r.returncode == 5 and text in r.stderr, (r.returncode, r.stdout, r.stderr)
