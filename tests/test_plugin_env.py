"""The plugin's table of environment variables (csrc/plugin/HipRT.cpp, kEnv) without a GPU: HipRT.cpp built against the
host-emulation library, behind tests/plugin/bloom_host.cpp.  The constructor refuses a value before anything renders: one bad value
of every two-valued variable and an unreadable path of both file variables end the host with status 5 and the exact message; with
RFWHIP_DISPLAY alone the plugin's bytes are the C ABI's."""
import os
import subprocess

import pytest

from plugin_hosts import ROOT, build_host, run_host

VARS = ("RFWHIP_DISPLAY", "RFWHIP_EXPOSURE", "RFWHIP_EXPOSURE_SPEED", "RFWHIP_BLOOM", "RFWHIP_GRADE", "RFWHIP_GRADE_TEMPERATURE",
        "RFWHIP_GRADE_SATURATION", "RFWHIP_DITHER", "RFWHIP_GRADE_LUT", "RFWHIP_JPEG_QUALITY", "RFWHIP_JPEG_SUBSAMPLING",
        "RFWHIP_JPEG_RESTART", "RFWHIP_NOISE", "RFWHIP_SKY_TABLE", "RFWHIP_SKY_HDR", "RFWHIP_INTEGRATOR", "RFWHIP_DEVICES",
        "RFWHIP_DEVICE", "RFWHIP_TRANSPORT", "RFWHIP_FRAMES_IN_FLIGHT")


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    import build_emu
    emu = build_emu.build()
    plugin_dir = tmp_path_factory.mktemp("emu_plugin")
    lib = str(plugin_dir / "librfwhip_emu.so")  # (one name for the plugin and the host: one copy of the library in the process)
    os.symlink(emu, lib)
    csrc = os.path.join(ROOT, "rendering-fw_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(csrc, "plugin"), os.path.join(csrc, "plugin", "HipRT.cpp"), "-o", str(plugin_dir / "HipRT.so"),
                        lib, "-Wl,-rpath," + os.path.dirname(emu)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    return build_host(pkg, tmp_path_factory, "bloom_host", lib=lib)


@pytest.mark.parametrize("env, message", [
    ({"RFWHIP_DISPLAY": "filmic"}, 'HipRT: RFWHIP_DISPLAY must be "aces" or "none"'),
    ({"RFWHIP_EXPOSURE": "bright"}, 'HipRT: RFWHIP_EXPOSURE must be "auto" or "manual"'),
    ({"RFWHIP_BLOOM": "yes"}, 'HipRT: RFWHIP_BLOOM must be "0" or "1"'),
    ({"RFWHIP_GRADE": "yes"}, 'HipRT: RFWHIP_GRADE must be "0" or "1"'),
    ({"RFWHIP_DITHER": "2"}, 'HipRT: RFWHIP_DITHER must be "0" or "1"'),
    ({"RFWHIP_NOISE": "on"}, 'HipRT: RFWHIP_NOISE must be "0" or "1"'),
    ({"RFWHIP_GRADE_LUT": "/nonexistent/look.cube"}, "HipRT: RFWHIP_GRADE_LUT: cannot read /nonexistent/look.cube"),
    ({"RFWHIP_SKY_HDR": "/nonexistent/sky.hdr"}, "HipRT: RFWHIP_SKY_HDR: cannot read /nonexistent/sky.hdr"),
], ids=["display", "exposure", "bloom", "grade", "dither", "noise", "grade_lut", "sky_hdr"])
def test_constructor_refuses(host, tmp_path, env, message):
    r = run_host(host, tmp_path, drop=VARS, **dict({"RFWHIP_DISPLAY": "aces"}, **env))
    assert r.returncode == 5 and r.stderr == "exception: " + message + "\n", (r.returncode, r.stdout, r.stderr)
    assert r.stdout == "" and os.listdir(tmp_path) == []  # before anything renders


def test_display_alone_presents_the_c_abi_bytes(host, tmp_path):
    r = run_host(host, tmp_path, drop=VARS, RFWHIP_DISPLAY="aces")
    assert r.returncode == 0 and r.stdout == "size 96 64\n", (r.returncode, r.stdout, r.stderr)
    plugin, abi = (open(os.path.join(tmp_path, n), "rb").read() for n in ("plugin.rgba8", "abi.rgba8"))
    assert len(plugin) == 96 * 64 * 4 and plugin == abi and len(set(plugin[0::4])) > 2  # (an image, not one colour)
