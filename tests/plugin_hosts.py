"""How the tests build and start the stand-ins for rfw::system of tests/plugin/ (host_common.h has what they share)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host(pkg, tmp_path_factory, name, lib=None):
    """Compile tests/plugin/<name>.cpp against librfwhip.so beside the plugin — or against the library `lib`, by its path — and
    return (exe, lib_dir): lib_dir is where the program finds HipRT.so."""
    lib_dir = os.path.dirname(lib or pkg.LIB_PATH)
    exe = str(tmp_path_factory.mktemp("plugin") / name)
    src = os.path.join(ROOT, "tests", "plugin", name + ".cpp")
    link = [lib] if lib else ["-L" + lib_dir, "-lrfwhip"]
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "rendering-fw_amd", "csrc", "plugin"), src, "-o", exe] + link +
                       ["-Wl,-rpath," + lib_dir, "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    if not os.path.exists(os.path.join(lib_dir, "HipRT.so")):
        pytest.fail("the plugin is not built")
    return exe, lib_dir


def run_host(host, *args, drop=(), timeout=120, **env):
    """Start the program on its plugin's directory (and args): the inherited environment without the variables of `drop`, under env."""
    exe, lib_dir = host
    base = {k: v for k, v in os.environ.items() if k not in drop}
    return subprocess.run([exe, lib_dir] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=timeout, env=dict(base, **env))
