"""The denoiser through the plugin's virtual interface (tests/plugin/denoise_host.cpp, compiled here): get_settings lists the
reference's "DENOISE" key, set_setting("DENOISE", "1") is accepted, and every image render_frame hands out — with 1 and with 4
frames in flight — is the C ABI's denoised image of the same frame, bit for bit."""
import pytest

from plugin_hosts import build_host, run_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    return build_host(pkg, tmp_path_factory, "denoise_host")


@pytest.mark.parametrize("in_flight", [1, 4])
def test_plugin_hands_out_the_c_abi_denoised_image(host, in_flight):
    r = run_host(host, RFWHIP_FRAMES_IN_FLIGHT=str(in_flight))
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert out["listed"] == "1"
    frames, _, equal = out["frames"].split()
    assert equal == frames == "6"
    assert out["differs_from_raw"] == "1"  # (the scene is noisy at 1 spp: the filter changed the image)
