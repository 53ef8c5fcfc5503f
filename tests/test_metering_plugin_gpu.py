"""The exposure meter through the plugin's virtual interface (tests/plugin/exposure_host.cpp, compiled here): with
RFWHIP_EXPOSURE=auto beside RFWHIP_DISPLAY, the bytes hiprtReadDisplay returns after every render_frame — with 2 frames in flight,
and with 1 — are the bytes the C ABI's rfwhip_group_read_display gives for the same frame, hiprtGetExposure reports one step per
frame and the C ABI's record, and a value the variable does not have is refused."""
import pytest

from plugin_hosts import build_host, run_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    return build_host(pkg, tmp_path_factory, "exposure_host")


def _run(host, **env):
    return run_host(host, RFWHIP_DISPLAY="aces", **env)


@pytest.mark.parametrize("in_flight", [2, 1])
def test_plugin_hands_out_the_c_abi_bytes_under_auto_exposure(host, in_flight):
    r = _run(host, RFWHIP_FRAMES_IN_FLIGHT=str(in_flight), RFWHIP_EXPOSURE="auto", RFWHIP_EXPOSURE_SPEED="0.5")
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    frames, _, equal = out["frames"].split()
    assert equal == frames == "5"
    assert out["steps"] == "5" and out["record_equal"] == "1" and out["varies"] == "1"
    assert float(out["exposure"]) != 1.0


def test_plugin_refuses_an_unknown_exposure_mode(host):
    r = _run(host, RFWHIP_EXPOSURE="bright")
    assert r.returncode == 5 and 'RFWHIP_EXPOSURE must be "auto" or "manual"' in r.stderr, (r.returncode, r.stdout, r.stderr)
