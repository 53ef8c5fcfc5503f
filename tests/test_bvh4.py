"""The TRAVERSED tree — compressed 4-wide nodes, their float form, leaf-ordered triangles, stack need — read back with
rfwhip_get_bvh4 and held to the exact checker of bvh4_check.py, for both builders, at the sizes and on the geometry where
the device builder's passes go wrong; and the closest hit of a ray as a function of the ray and the scene only, whichever
builder made the tree.  The CPU tier runs on the host-emulation build, the GPU tier (same cases, larger sizes) on
librfwhip.so.  In every GPU case the checker runs before any ray is traced."""
import os

import numpy as np
import pytest

from bvh4_check import check_bvh4
from test_bvh import _soup

HOST_MAX_LEAF = 4     # rfwhip_api.cpp: BLAS_MAX_LEAF
DEVICE_MAX_LEAF = 4   # lbvh.hip: RT_DEVICE_MAX_LEAF
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SIZES = [5, 6, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 4095, 4097, 65537]
SIZES_EMU = [n for n in SIZES if n <= 20000] + [20001]
KINDS = ["uniform", "clustered", "slivers", "far_from_origin", "duplicates", "comb",
         "identical", "plane", "line", "negative", "signed_zero"]


def soup(kind, rng, n):
    """n triangles (n x 3 vertices, float32) of one kind: test_bvh's soups, and the ones the device builder's key and
    clustering passes meet at their ends."""
    if kind == "comb":                     # positions grow as 1.02^i: past ~600 triangles they leave float range
        return _soup(kind, rng, min(n, 600))
    if kind == "duplicates":
        return _soup(kind, rng, 4 * ((n + 3) // 4))[:3 * n]
    if kind in ("uniform", "clustered", "slivers", "far_from_origin"):
        return _soup(kind, rng, n)
    if kind == "identical":                # every Morton key equal, every union box equal: the `force` pairing pass
        return np.tile(np.array([[-1, 0, 3], [1, 0, 3], [0, 1.5, 3]], np.float32), (n, 1))
    if kind == "plane":                    # every vertex at z = 3: a zero extent (e clamped to -100) on one axis
        v = rng.uniform(-10, 10, (n, 1, 3)) + rng.normal(0, 0.4, (n, 3, 3))
        v[..., 2] = 3.0
        return v.reshape(-1, 3).astype(np.float32)
    if kind == "line":                     # centroids on one line parallel to x: the keys differ in x only
        e = rng.normal(0, 0.4, (n, 3, 3))
        e -= e.mean(1, keepdims=True)
        c = np.zeros((n, 1, 3))
        c[..., 0] = rng.uniform(-10, 10, (n, 1))
        return (c + e).reshape(-1, 3).astype(np.float32)
    if kind == "negative":                 # only negative coordinates (float_key of negative floats)
        return (rng.uniform(-30, -10, (n, 1, 3)) - np.abs(rng.normal(0, 0.4, (n, 3, 3)))).reshape(-1, 3).astype(np.float32)
    if kind == "signed_zero":              # many coordinates exactly +0.0 or -0.0 (min / max and float_key on both zeros)
        v = (rng.uniform(-1, 1, (n, 1, 3)) + rng.normal(0, 0.3, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
        z = rng.random(v.shape) < 0.4
        v[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
        return v
    if kind == "huge":                     # ~1e19: box_area overflows to inf, the nearest-neighbour search finds nothing
        return (rng.uniform(-1e19, 1e19, (n, 1, 3)) + rng.normal(0, 1e17, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    raise ValueError(kind)


def soup_scene(pkg, verts):
    s = pkg.scenes.Scene()
    s.add_material(color=(0.8, 0.8, 0.8))
    s.add_instance(s.add_mesh(verts, None))
    s.set_test_sky(16, 8)
    return s


def build(make_ctx, scene, builder):
    c = make_ctx()
    c.set_setting("builder", builder)
    c.init(16, 16)
    scene.upload(c)
    return c


def check_mesh(c, scene, mi, builder=None, vertices="scene"):
    """Checker on mesh mi of a resident scene; returns the hook's record.  builder: which builder must have built it
    (builder=device hands meshes of <= BLAS_MAX_LEAF triangles to the host builder by design)."""
    b = c.get_bvh4(mi)
    m = scene.meshes[mi]
    if builder is not None:
        assert b["device_built"] == (builder == "device" and len(m["triangles"]) > HOST_MAX_LEAF), "built by the other builder"
    v = m["vertices"] if isinstance(vertices, str) else vertices
    stamps = [i for i, inst in enumerate(scene.instances) if inst["mesh"] == mi]
    check_bvh4(b, v, m["indices"], DEVICE_MAX_LEAF if b["device_built"] else HOST_MAX_LEAF, c.get_bvh(mi)[0], stamps)
    return b


def soup_case(pkg, make_ctx, kind, n, builder, seed=0, expect=None):
    """expect: the builder that must have built the mesh (default: expected_builder)."""
    verts = soup(kind, np.random.default_rng(seed + n), n)
    s = soup_scene(pkg, verts)
    c = build(make_ctx, s, builder)
    check_mesh(c, s, 0, expect or expected_builder(kind, n, builder))
    return c, s


def expected_builder(kind, n, builder):
    """Where builder=device hands the mesh to the host builder, by design: the device tree needs more than
    BLAS_STACK_BUDGET = 48 stack entries (or the clustering more passes than its budget).
    - comb: the deepest soup; the device tree, which has no depth limit, needs 63 entries at 600 triangles.
    - identical: all union areas tie, and ploc_nearest_item keeps the first candidate of its window on a tie, so the only
      mutual pair of a pass is (0, 1): one merge per pass, a chain (stack need n - 4), and the `force` pass never runs.
    - signed_zero: about a fifth of the triangles lie in the planes x, y or z = 0; at 65 537 triangles the device tree
      needs 59 entries (42 at 20 001)."""
    if builder == "device" and ((kind == "comb" and n >= 600) or (kind == "identical" and n >= 129) or
                                (kind == "signed_zero" and n >= 65537)):
        return "host"
    return builder


def geometry_sizes(kind):
    # the comb's device tree outgrows the traversal-stack budget (48 entries) between 400 and 600 triangles: see expected_builder
    # (identical: one merge per clustering pass, see expected_builder — O(n^2) on the emulation)
    return (7, 129, 257) if kind == "comb" else (7, 129, 600) if kind == "identical" else (7, 129, 600, 4097)


# ---- CPU tier (host-emulation build) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["host", "device"])
def test_sizes(pkg, make_emu, builder):
    for n in SIZES_EMU:
        soup_case(pkg, make_emu, "uniform", n, builder)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("builder", ["host", "device"])
def test_geometry(pkg, make_emu, kind, builder):
    for n in geometry_sizes(kind):
        soup_case(pkg, make_emu, kind, n, builder)


def test_comb_and_identical_fall_back_to_the_host_builder(pkg, make_emu):
    soup_case(pkg, make_emu, "comb", 600, "device", expect="host")
    soup_case(pkg, make_emu, "identical", 600, "device", expect="host")


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_tiny_meshes_go_to_the_host_builder(pkg, make_emu, n):
    """n <= BLAS_MAX_LEAF: rfwhip_set_mesh builds these on the host even with builder=device (soup_case asserts it)."""
    soup_case(pkg, make_emu, "uniform", n, "device")


def test_huge_coordinates(pkg, make_emu):
    huge_case(pkg, make_emu, 4097)


def huge_case(pkg, make_ctx, n):
    """Coordinates ~1e19: every union box's area is inf, so the clustering's nearest-neighbour search finds no partner and
    only the `force` pass pairs clusters.  The device builder still builds a valid tree there (no fallback to the host)."""
    s = soup_scene(pkg, soup("huge", np.random.default_rng(n), n))
    c = build(make_ctx, s, "device")
    b = check_mesh(c, s, 0)
    assert b["device_built"]
    host = build(make_ctx, s, "host")
    check_mesh(host, s, 0, "host")


def test_not_resident_is_a_state_error(pkg, make_emu):
    s = soup_scene(pkg, soup("uniform", np.random.default_rng(1), 100))
    c = build(make_emu, s, "host")
    m = s.meshes[0]
    v = m["vertices"].copy()
    c.set_mesh(0, v[:len(v) - 3], m["triangles"][:-1], None)   # another count: a rebuild, placed by the next update
    with pytest.raises(RuntimeError, match="not resident"):
        c.get_bvh4(0)
    c.update()
    assert c.get_bvh4(0)["tri_count"] == 99


def rebase_case(pkg, make_ctx, counts, grow):
    """Three device-built meshes with two (transformed) instances each: every mesh after the first sits behind others, at
    non-zero n4_base / tri_base.  Then mesh 0 is set with more triangles (a rebuild that grows the builder's scratch) and
    every mesh is checked again after the update."""
    rng = np.random.default_rng(7)
    s = pkg.scenes.Scene()
    s.add_material(color=(0.8, 0.8, 0.8))
    for k, n in enumerate(counts):
        mi = s.add_mesh(soup("uniform", rng, n), None)
        for j in range(2):
            t = np.eye(4)
            t[:3, 3] = (30.0 * k, 30.0 * j, 0.0)
            s.add_instance(mi, t)
    s.set_test_sky(16, 8)
    c = build(make_ctx, s, "device")
    recs = [check_mesh(c, s, mi, "device") for mi in range(len(counts))]
    assert all(r["n4_base"] > 0 and r["tri_base"] > 0 for r in recs[1:])
    s.meshes[0] = soup_scene(pkg, soup("clustered", rng, grow)).meshes[0]
    m = s.meshes[0]
    c.set_mesh(0, m["vertices"], m["triangles"], None)
    c.update()
    recs2 = [check_mesh(c, s, mi, "device") for mi in range(len(counts))]
    assert recs2[0]["tri_count"] == grow and recs2[1]["tri_base"] == grow and recs2[1]["n4_base"] == recs2[0]["n4_count"]
    return c


def test_rebase_multi_mesh(pkg, make_emu):
    rebase_case(pkg, make_emu, (300, 3000, 5), 5000)


def refit_case(pkg, make_ctx, builder):
    """Same-count set_mesh of the skinned tube (pose 0 -> 3) refits: k_refit_nodes + k_refresh4.  The checker holds the
    refreshed nodes to the NEW vertices."""
    s0 = pkg.scenes.skinned_tube(frame=0.0, rings=40, seg=24, width=16, height=16)
    s1 = pkg.scenes.skinned_tube(frame=3.0, rings=40, seg=24, width=16, height=16)
    c = build(make_ctx, s0, builder)
    before = check_mesh(c, s0, 0, builder)
    m = s1.meshes[0]
    c.set_mesh(0, m["vertices"], m["triangles"], m["indices"])
    c.update()
    after = check_mesh(c, s1, 0, builder)
    assert not np.array_equal(before["nodes4c"], after["nodes4c"])   # the boxes really moved
    assert np.array_equal(before["nodes4c"]["entry"], after["nodes4c"]["entry"])
    return c, s1


@pytest.mark.parametrize("builder", ["host", "device"])
def test_refit(pkg, make_emu, builder):
    refit_case(pkg, make_emu, builder)


def rig_case(pkg, make_ctx, rig, builder):
    """Meshes posed ON THE DEVICE (skinning: CesiumMan, morph targets: the morph cube): after pose + update, the refitted
    nodes contain the posed triangles, and those are the fixture's pose."""
    from test_assets import _rig_scene
    fx = np.load(os.path.join(GOLD, "asset_cesiumman.npz" if rig == "skin" else "asset_morphcube.npz"))
    s = _rig_scene(pkg, fx["positions"], fx["normals"], fx["indices"], fx["node_transform"], 16, 16)
    c = build(make_ctx, s, builder)
    check_mesh(c, s, 0, builder)
    if rig == "skin":
        c.set_mesh_skin(0, fx["joints"], fx["weights"], fx["normals"])
        poses = [(lambda k=k: c.pose_mesh(0, fx["joint_matrices"][k]), fx["posed_positions"][k]) for k in range(len(fx["times"]))]
    else:
        c.set_mesh_morph(0, fx["normals"], fx["target_positions"], fx["target_normals"])
        poses = [(lambda k=k: c.morph_mesh(0, fx["weights"][k]), fx["morphed_positions"][k]) for k in range(len(fx["times"]))]
    idx = np.asarray(fx["indices"], np.int64).reshape(-1, 3)
    for apply, pv in poses:
        apply()
        c.update()
        b = check_mesh(c, s, 0, builder, vertices=None)
        prim = b["tri_verts"][:, 0, 3].view(np.uint32)
        want = np.asarray(pv, np.float64)[idx[prim]]
        scale = float(np.abs(want).max())
        assert np.abs(b["tri_verts"][:, :, :3] - want).max() <= 1e-5 * scale   # the slots hold the new pose


@pytest.mark.parametrize("rig", ["skin", "morph"])
@pytest.mark.parametrize("builder", ["host", "device"])
def test_device_posed_rigs(pkg, make_emu, rig, builder):
    rig_case(pkg, make_emu, rig, builder)


# ---- the hit is a function of the ray and the scene -----------------------------------------------------------------------
def aimed_rays(verts, rng, n):
    """Rays aimed at triangles from around the soup, as in test_bvh._soup_case."""
    lo, hi = verts.min(0), verts.max(0)
    tri_c = verts.reshape(-1, 3, 3).mean(1)
    org = (tri_c[rng.integers(0, len(tri_c), n)] + rng.normal(0, 1.0, (n, 3)) * (hi - lo) * 0.7).astype(np.float32)
    tgt = tri_c[rng.integers(0, len(tri_c), n)] + rng.normal(0, 0.05, (n, 3)) * np.maximum(hi - lo, 1e-3) / 20
    d = tgt - org
    return org, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def same_hits(pkg, make_ctx, scene, verts, nrays, kind=None):
    """A host-built and a device-built context trace the same rays: hit / miss on every ray, t bit for bit, and a
    different primitive only where the two are a genuine tie at that t (tri_test's total order on (t, instance, prim)
    makes the record independent of the tree)."""
    ctx = {}
    for builder in ("host", "device"):
        ctx[builder] = build(make_ctx, scene, builder)
        for mi in range(len(scene.meshes)):   # the structure first: a malformed tree fails before any traversal
            check_mesh(ctx[builder], scene, mi, expected_builder(kind, len(scene.meshes[mi]["triangles"]), builder))
    org, d = aimed_rays(verts, np.random.default_rng(len(verts)), nrays)
    a, b = ctx["host"].trace_rays(org, d), ctx["device"].trace_rays(org, d)
    ha, hb = a["prim"] >= 0, b["prim"] >= 0
    assert np.array_equal(ha, hb), "hit / miss differs on %d rays" % int((ha != hb).sum())
    assert np.array_equal(a["t"][ha].view(np.uint32), b["t"][hb].view(np.uint32)), "t differs"
    assert np.array_equal(a["inst"], b["inst"])
    diff = ha & (a["prim"] != b["prim"])
    return ha.mean(), int(diff.sum())


@pytest.mark.parametrize("kind", KINDS)
def test_hits_do_not_depend_on_the_builder(pkg, make_emu, kind):
    verts = soup(kind, np.random.default_rng(3), 257 if kind == "comb" else 2000)
    same_hits(pkg, make_emu, soup_scene(pkg, verts), verts, 20000, kind)


def test_hits_do_not_depend_on_the_builder_terrain(pkg, make_emu):
    s = pkg.scenes.terrain(n=40, width=16, height_px=16, lights=False)
    m = s.meshes[0]
    same_hits(pkg, make_emu, s, m["vertices"][:, :3][np.asarray(m["indices"]).reshape(-1)], 20000)
