"""The primary wave's entry snapshot on the device (k_primary_entry, the start of k_primary_packet's walk; csrc/primary_entry.h): what
tests/test_primary_entry.py checks on the emulation, on the HIP library.  A start point never decides a closest hit, so a render with
primary_entry = 1 equals one with 0 value for value: primary hit records and framebuffer, number of differing values 0."""
import numpy as np
import pytest

from test_primary_entry import context, fresh, passes, render

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def ordered_everywhere(monkeypatch):
    monkeypatch.setenv("RFWHIP_PRIMARY_ORDER", "1")  # (the snapshot rides on the ordered table; small frames have none by the rule)


def differing(a, b):
    n = int((a["image"].view(np.uint32) != b["image"].view(np.uint32)).sum())
    for k in a["hits"]:
        n += int((a["hits"][k].view(np.uint32) != b["hits"][k].view(np.uint32)).sum())
    return n


@pytest.mark.parametrize("w,h,spp", [(64, 32, 64), (72, 40, 8)])  # one pixel per wave; g = 8 with remainder tiles
def test_on_equals_off(pkg, make_hip, w, h, spp):
    scene = pkg.scenes.terrain(n=32, width=w, height_px=h)
    out = []
    for entry in (0, 1):
        c = context(make_hip, scene, w, h, spp, spp, primary_entry=entry, max_depth=2)
        out.append(render(c, scene.camera, pkg, calls=2))
        assert c.get_setting("primary_entry_on") == str(entry) and passes(c) == entry
        c.destroy()
    assert (out[0]["hits"]["prim"] >= 0).any() and (out[0]["hits"]["prim"] < 0).any()
    assert out[0]["counts"] == out[1]["counts"]
    assert differing(out[1], out[0]) == 0


def test_a_camera_that_only_rotates_reruns_the_pass(pkg, make_hip):
    w, h = 64, 32
    scene = pkg.scenes.terrain(n=32, width=w, height_px=h)
    cam = scene.camera
    c = context(make_hip, scene, w, h, 64, 64)
    render(c, cam, pkg)
    d = np.asarray(cam.direction, np.float64) + (0.2, -0.05, 0.0)
    cam.direction = tuple(float(x) for x in d / np.linalg.norm(d))
    got = render(c, cam, pkg)
    assert passes(c) == 2 and c.get_kernel_time("primary_order")[1] == 1
    c.destroy()
    assert differing(got, fresh(pkg, make_hip, scene, cam, w, h)) == 0


def test_a_refit_reruns_the_pass(pkg, make_hip):
    w, h, rings, seg = 64, 32, 24, 16
    scene = pkg.scenes.skinned_tube(0.0, rings=rings, seg=seg, width=w, height=h)
    v, idx, vn, joints, weights = pkg.scenes.skinned_tube_rig(rings, seg)
    scene.meshes[0]["triangles"] = pkg.scenes.make_triangles(v, idx, normals=vn, material=scene.meshes[0]["triangles"]["material"][0])

    def pose(c):
        c.set_mesh_skin(0, joints, weights, vn)
        c.pose_mesh(0, pkg.scenes.skinned_tube_joint_matrices(3.0))
        c.update()
    c = context(make_hip, scene, w, h, 64, 64)
    c.set_mesh_skin(0, joints, weights, vn)
    before = render(c, scene.camera, pkg)
    c.pose_mesh(0, pkg.scenes.skinned_tube_joint_matrices(3.0))
    c.update()
    got = render(c, scene.camera, pkg)
    assert passes(c) == 2 and c.get_setting("primary_entry_on") == "1"
    c.destroy()
    assert differing(got, before) > 0
    assert differing(got, fresh(pkg, make_hip, scene, scene.camera, w, h, prepare=pose)) == 0


def test_device_equals_the_emulation(pkg, make_hip):
    """480 x 270 on a 128-cell terrain, 8 samples per pixel in groups of 8, primary wave only, snapshot on: the hit records of the
    device and of the emulation bit for bit.  The pair that can agree to the bit is the strict-arithmetic one (tests/test_strict_gpu.py:
    the same sources without fma contraction, v_rcp and the fast transcendental functions — the shipped kernels differ from the
    emulation by that arithmetic alone); the shipped library's differences are printed (MI355X, against the plain emulation: prim 0,
    inst 0, t 7434, u 7407, v 7443 of 129 600 values)."""
    import ctypes
    import os
    import build_emu
    from conftest import ROOT
    from test_strict_gpu import STRICT_FLAGS
    w, h = 480, 270
    scene = pkg.scenes.terrain(n=128, width=w, height_px=h)
    strict_so = os.path.join(ROOT, "tests", "_strict", "librfwhip_strict.so")
    assert os.path.exists(strict_so), "build it with __graft_entry__.build() (build.py: build_strict)"
    libs = {"strict device": ctypes.CDLL(strict_so), "strict emulation": ctypes.CDLL(build_emu.build(defines=STRICT_FLAGS, tag="_strict"))}
    hits = {}
    for name in ("strict device", "strict emulation", "device"):
        make = make_hip if name == "device" else (lambda: pkg._binding.CoreBinding(libs[name], "rfwhip_", 0, 0, 1))
        c = context(make, scene, w, h, 8, 8, primary_entry=1, max_depth=0)
        c.render_frame(scene.camera, pkg.RESET)
        assert c.get_setting("primary_entry_on") == "1" and passes(c) == 1
        hits[name] = c.primary_hits()
        c.destroy()
    assert (hits["strict device"]["prim"] >= 0).any()

    def diff(a, b):
        return {k: int((hits[a][k].view(np.uint32) != hits[b][k].view(np.uint32)).sum()) for k in hits[a]}
    n = diff("strict device", "strict emulation")
    shipped = diff("device", "strict emulation")
    print("differing hit values, strict device against strict emulation:", n, "shipped device against strict emulation:", shipped)
    assert sum(n.values()) == 0
