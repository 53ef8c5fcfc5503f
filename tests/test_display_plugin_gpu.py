"""The display stage through the plugin's virtual interface (tests/plugin/display_host.cpp, compiled here): with RFWHIP_DISPLAY
set, the bytes hiprtReadDisplay returns after every render_frame — with 2 frames in flight, and with 1 — are the bytes the C ABI's
rfwhip_group_read_display gives for the same frame."""
import pytest

from plugin_hosts import build_host, run_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    return build_host(pkg, tmp_path_factory, "display_host")


@pytest.mark.parametrize("mode,in_flight", [("aces", 2), ("aces", 1), ("none", 2)])
def test_plugin_hands_out_the_c_abi_display_bytes(host, mode, in_flight):
    r = run_host(host, RFWHIP_FRAMES_IN_FLIGHT=str(in_flight), RFWHIP_DISPLAY=mode)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    frames, _, equal = out["frames"].split()
    assert equal == frames == "5"
    assert out["varies"] == "1" and out["alpha_kept"] == "1"
