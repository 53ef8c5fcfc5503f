"""The denoiser's temporal stage through the plugin's virtual interface (tests/plugin/denoise_temporal_host.cpp, compiled here):
get_settings lists "DENOISE_TEMPORAL", and with DENOISE and DENOISE_TEMPORAL on, a moving camera and Reset every frame, every image
render_frame hands out — with 1 and with 4 frames in flight — is the C ABI's image of the same frame, bit for bit: the order in
which frames are presented drives the history."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    exe = str(tmp_path_factory.mktemp("plugin") / "denoise_temporal_host")
    src = os.path.join(ROOT, "tests", "plugin", "denoise_temporal_host.cpp")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "rendering-fw_amd", "csrc", "plugin"), src, "-o", exe, "-L" + lib_dir, "-lrfwhip",
                        "-Wl,-rpath," + lib_dir, "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    return exe, lib_dir


@pytest.mark.parametrize("in_flight", [1, 4])
def test_plugin_hands_out_the_c_abi_temporal_frames(host, in_flight):
    exe, lib_dir = host
    env = dict(os.environ, RFWHIP_FRAMES_IN_FLIGHT=str(in_flight))
    r = subprocess.run([exe, lib_dir], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert out["listed"] == "1"
    frames, _, equal = out["frames"].split()
    assert equal == frames == "6"
    assert out["differs_from_spatial"] == "1"  # (the history changed the last frame's image)
