"""Bloom through the plugin's virtual interface (tests/plugin/bloom_host.cpp, compiled here): with RFWHIP_BLOOM=1 beside
RFWHIP_DISPLAY the bytes hiprtReadDisplay returns are the float64 models' (bloom_model, then display_model) on the linear image the
C ABI gives for the same frame; with the variable unset, or "0", they are the C ABI's display bytes of a context that never touched
a display_bloom* setting; a value the variable does not have is refused."""
import os

import numpy as np
import pytest

import test_bloom as cpu
from plugin_hosts import build_host, run_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    return build_host(pkg, tmp_path_factory, "bloom_host")


def _run(host, out, **env):
    return run_host(host, out, drop=("RFWHIP_BLOOM",), RFWHIP_DISPLAY="aces", **env)


def _images(r, out):
    assert r.returncode == 0, (r.stdout, r.stderr)
    w, h = (int(v) for v in r.stdout.split()[1:3])
    plugin = np.fromfile(os.path.join(out, "plugin.rgba8"), np.uint8).reshape(h, w, 4)
    plain = np.fromfile(os.path.join(out, "abi.rgba8"), np.uint8).reshape(h, w, 4)
    linear = np.fromfile(os.path.join(out, "abi.f32"), np.float32).reshape(h, w, 4)
    return plugin, plain, linear


def test_plugin_blooms_the_display_image(host, tmp_path):
    plugin, plain, linear = _images(_run(host, tmp_path, RFWHIP_BLOOM="1"), tmp_path)
    assert linear[..., :3].max() > 2.0 and not np.array_equal(plugin, plain)
    cpu.judge_display(linear, 1.0, 0.05, 1.0, plugin, None, "plugin, RFWHIP_BLOOM=1")


@pytest.mark.parametrize("value", [None, "0"])
def test_plugin_without_the_variable_is_unchanged(host, tmp_path, value):
    env = {} if value is None else {"RFWHIP_BLOOM": value}
    plugin, plain, _ = _images(_run(host, tmp_path, **env), tmp_path)
    assert np.array_equal(plugin, plain)


def test_plugin_refuses_an_unknown_value(host, tmp_path):
    r = _run(host, tmp_path, RFWHIP_BLOOM="yes")
    assert r.returncode == 5 and 'RFWHIP_BLOOM must be "0" or "1"' in r.stderr, (r.returncode, r.stdout, r.stderr)
