"""The noise estimate on the device (k_resolve_noise, k_noise_merge, k_noise_tiles, k_noise_final; work items: csrc/noise.h): the
checks of tests/test_noise.py on the HIP kernels at the same small shapes, held to the float64 model of tests/noise_model.py (not
to the emulation), one full-size metric, a group of two contexts on one device, and the plugin's hiprtGetNoise."""
import numpy as np
import pytest

import noise_model as nm
import test_noise as tn
from plugin_hosts import build_host, run_host

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("spp", tn.SPPS)
def test_images_untouched(pkg, make_hip, spp):
    tn.check_images_untouched(pkg, make_hip, spp)


def test_step_update_on_given_samples(make_hip):
    nm.merge_cases(make_hip())


def test_end_to_end(pkg, make_hip):
    tn.check_end_to_end(pkg, make_hip)


@pytest.mark.parametrize("size", nm.SIZES, ids=lambda s: "%dx%d" % s)
def test_metric_on_given_moments(make_hip, size):
    c = make_hip()
    for kind in nm.KINDS:
        nm.check_metric(c, kind, *size)
    nm.check_metric(c, "straddle", *size, floor=0.1, threshold=0.2)


def test_full_size_metric(make_hip):
    """1920 x 1080: 60 x 135 tiles, more than the 256 threads of the final reduction fold in one round each."""
    c = make_hip()
    st = nm.check_metric(c, "straddle", 1920, 1080)
    assert st["pixels"] == 1920 * 1080
    nm.check_metric(c, "nonfinite", 1920, 1080)


def test_state_errors(pkg, make_hip):
    tn.check_state_errors(pkg, make_hip, None)


def test_render_until(pkg, make_hip):
    tn.check_render_until(pkg, make_hip)


def test_group_on_one_device_equals_the_single_context(pkg, make_hip):
    one = make_hip()
    scene = tn.setup(pkg, one, 3, 1, 130, 70)
    tn.frames(pkg, one, scene, 2)
    want = one.get_noise()
    g = pkg.render_group([0, 0], "peer")
    g.init(130, 70)
    scene.upload(g)
    for k, v in dict(integrator="pt", spp=3, noise_estimate=1).items():
        g.set_setting(k, v)
    g.render_frame(scene.camera, pkg.RESET)
    g.render_frame(scene.camera, pkg.CONVERGE)
    got = g.get_noise()
    assert np.array_equal(g.framebuffer(), one.framebuffer())
    g.destroy()
    for k in ("samples", "pixels", "converged", "max_error", "threshold"):
        assert got[k] == want[k], k
    assert abs(got["mean_error"] - want["mean_error"]) <= nm.gamma(256) * want["mean_error"]


@pytest.fixture(scope="module")
def plugin_host(pkg, tmp_path_factory):
    return build_host(pkg, tmp_path_factory, "noise_host")


@pytest.mark.parametrize("on", [1, 0])
def test_plugin_reports_the_noise(plugin_host, on):
    """HipRT.so behind the stand-in for rfw::system (tests/plugin/noise_host.cpp): with RFWHIP_NOISE=1 hiprtGetNoise refuses after
    the first sample and then answers with the C ABI's record of the same frames, byte for byte; without the variable it refuses."""
    r = run_host(plugin_host, drop=("RFWHIP_NOISE",), **({"RFWHIP_NOISE": "1"} if on else {}))
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    state_error = "4"  # RFWHIP_ERR_STATE
    assert out["on"] == str(on) and out["first"] == state_error
    if on:
        samples, pixels, converged, mean_e, max_e = out["stats"].split()
        assert out["last"] == "0" and out["equal"] == "1"
        assert (int(samples), int(pixels)) == (3, 96 * 64) and 0 <= int(converged) <= 96 * 64 and 0 < float(mean_e) <= float(max_e)
    else:
        assert out["last"] == state_error and out["equal"] == "0"
