"""The JPEG of the presented frame through the plugin's virtual interface (tests/plugin/jpeg_host.cpp, compiled here): what
hiprtReadJpeg returns is the numpy model's stream (tests/jpeg_model.py) of the bytes hiprtReadDisplay returns for the same frame,
under the settings the RFWHIP_JPEG_* variables name and under the defaults; a value a variable does not have is refused."""
import os

import numpy as np
import pytest

import jpeg_model as jm
from plugin_hosts import build_host, run_host

pytestmark = pytest.mark.gpu
VARS = ("RFWHIP_JPEG_QUALITY", "RFWHIP_JPEG_SUBSAMPLING", "RFWHIP_JPEG_RESTART", "RFWHIP_GRADE", "RFWHIP_BLOOM", "RFWHIP_EXPOSURE")


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    return build_host(pkg, tmp_path_factory, "jpeg_host")


def _run(host, out, **env):
    return run_host(host, out, drop=VARS, RFWHIP_DISPLAY="aces", **env)


def _check(r, out, quality, sub, ri):
    assert r.returncode == 0, (r.stdout, r.stderr)
    f = r.stdout.split()
    w, h, bound, n = int(f[1]), int(f[2]), int(f[4]), int(f[6])
    frame = np.fromfile(os.path.join(out, "plugin.rgba8"), np.uint8).reshape(h, w, 4)
    stream = open(os.path.join(out, "plugin.jpg"), "rb").read()
    assert len(stream) == n <= bound == jm.bound(w, h, sub, ri)
    assert stream == jm.encode(frame, quality, sub, ri)[0]


def test_plugin_hands_out_the_models_stream(host, tmp_path):
    _check(_run(host, tmp_path), tmp_path, 90, "420", 8)  # the defaults
    _check(_run(host, tmp_path, RFWHIP_JPEG_QUALITY="35", RFWHIP_JPEG_SUBSAMPLING="444", RFWHIP_JPEG_RESTART="3"), tmp_path, 35, "444", 3)


def test_plugin_refuses_what_the_settings_refuse(host, tmp_path):
    for env in (dict(RFWHIP_JPEG_QUALITY="0"), dict(RFWHIP_JPEG_QUALITY="best"), dict(RFWHIP_JPEG_SUBSAMPLING="422"),
                dict(RFWHIP_JPEG_RESTART="65536"), dict(RFWHIP_JPEG_RESTART="")):
        r = _run(host, tmp_path, **env)
        assert r.returncode == 5 and " must " in r.stderr, (env, r.returncode, r.stderr)
