"""The display stage through the plugin's virtual interface (tests/plugin/display_host.cpp, compiled here): with RFWHIP_DISPLAY
set, the bytes hiprtReadDisplay returns after every render_frame — with 2 frames in flight, and with 1 — are the bytes the C ABI's
rfwhip_group_read_display gives for the same frame."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    exe = str(tmp_path_factory.mktemp("plugin") / "display_host")
    src = os.path.join(ROOT, "tests", "plugin", "display_host.cpp")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "rendering-fw_amd", "csrc", "plugin"), src, "-o", exe, "-L" + lib_dir, "-lrfwhip",
                        "-Wl,-rpath," + lib_dir, "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    return exe, lib_dir


@pytest.mark.parametrize("mode,in_flight", [("aces", 2), ("aces", 1), ("none", 2)])
def test_plugin_hands_out_the_c_abi_display_bytes(host, mode, in_flight):
    exe, lib_dir = host
    if not os.path.exists(os.path.join(lib_dir, "HipRT.so")):
        pytest.skip("plugin not built")
    env = dict(os.environ, RFWHIP_FRAMES_IN_FLIGHT=str(in_flight), RFWHIP_DISPLAY=mode)
    r = subprocess.run([exe, lib_dir], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    frames, _, equal = out["frames"].split()
    assert equal == frames == "5"
    assert out["varies"] == "1" and out["alpha_kept"] == "1"
