"""GPU tier of test_bvh4: the same exact checks of the traversed tree on librfwhip.so, at every size up to 65 537
triangles, on the 1 M-triangle bench terrain, and across the multi-mesh rebase; then host- and device-built trees must give
the same closest hit for every ray.  In each test the structural checker runs before any ray is traced, so a malformed
tree fails an assertion instead of reaching a traversal kernel."""
import time

import numpy as np
import pytest

from test_bvh4 import (KINDS, SIZES, build, check_mesh, expected_builder, huge_case, rebase_case, refit_case, rig_case,
                       same_hits, soup, soup_case, soup_scene)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("builder", ["host", "device"])
def test_sizes_gpu(pkg, make_hip, builder):
    for n in SIZES:
        soup_case(pkg, make_hip, "uniform", n, builder)
    for n in (1, 2, 3, 4):
        soup_case(pkg, make_hip, "uniform", n, builder)   # builder=device: built on the host by design


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("builder", ["host", "device"])
def test_geometry_gpu(pkg, make_hip, kind, builder):
    sizes = {"comb": (7, 129, 257, 600), "identical": (7, 129, 600, 4097)}.get(kind, (7, 129, 600, 4097, 65537))
    for n in sizes:
        soup_case(pkg, make_hip, kind, n, builder)


def test_huge_coordinates_gpu(pkg, make_hip):
    huge_case(pkg, make_hip, 65537)


def test_rebase_multi_mesh_gpu(pkg, make_hip):
    rebase_case(pkg, make_hip, (300, 70000, 5), 100000)


@pytest.mark.parametrize("builder", ["host", "device"])
def test_refit_gpu(pkg, make_hip, builder):
    refit_case(pkg, make_hip, builder)


@pytest.mark.parametrize("rig", ["skin", "morph"])
@pytest.mark.parametrize("builder", ["host", "device"])
def test_device_posed_rigs_gpu(pkg, make_hip, rig, builder):
    rig_case(pkg, make_hip, rig, builder)


@pytest.mark.parametrize("kind", KINDS + ["huge"])
def test_hits_do_not_depend_on_the_builder_gpu(pkg, make_hip, kind):
    n = {"comb": 257, "identical": 600, "signed_zero": 20001}.get(kind, 65537)   # (where builder=device builds on the device)
    verts = soup(kind, np.random.default_rng(3), n)
    same_hits(pkg, make_hip, soup_scene(pkg, verts), verts, 200000, kind)


def test_bench_terrain_device_built_gpu(pkg, make_hip):
    """The bench mesh (scenes.terrain(): 1 002 528 triangles) with builder=device: built on the device — no fallback — and
    exact under the checker; then the same 200 k aimed rays hit the same triangles at the same t through the host-built
    tree."""
    s = pkg.scenes.terrain(width=16, height_px=16, lights=False)
    m = s.meshes[0]
    dev = build(make_hip, s, "device")
    t0 = time.perf_counter()
    b = check_mesh(dev, s, 0, "device")
    dt = time.perf_counter() - t0
    print("\nbench terrain, builder=device: %d triangles, device_built=%s, n4_count=%d, stack_need=%d, checker %.2f s"
          % (b["tri_count"], b["device_built"], b["n4_count"], b["stack_need"], dt))
    assert b["device_built"] and b["tri_count"] == len(m["triangles"])
    del dev
    hit, ties = same_hits(pkg, make_hip, s, m["vertices"][:, :3][np.asarray(m["indices"]).reshape(-1)], 200000)
    print("bench terrain: %.3f of the rays hit, %d ties settled on different primitives" % (hit, ties))
    assert hit > 0.5
