"""The primary wave's entry snapshot (csrc/primary_entry.h; settings `primary_entry` / `primary_entry_on`, kernel family 16), CPU
tier, through the host-emulation library.

1. The RECORDS of a render, read back with the camera-ordered table they were made from (rfwhip_emu_primary_entry, an entry of the
   emulation libraries only), against the float64 model of tests/primary_entry_model.py: entry words and order, word for word — and
   COVERAGE: from the root, with 260 (g = 64) rays per pixel of every group, the jitter corners 0 and nextafter(1, 0) among them,
   every node and leaf an exact per-ray slab test enters lies under an entry of the group's record or was expanded by the pass.
   Allowed number of uncovered nodes: 0.  Cameras: the scene's own, grazing over the terrain, inside a box, looking away from
   everything (empty records), and so far away that the scene is smaller than a pixel.
2. RENDERS with the snapshot on against off: a start point never decides a closest hit, so hit records, images and per-depth counts
   are bit-equal — sample groups 1, 8 and 64, remainder tiles, two strip-interleaved ranks, instances (left unexpanded), an
   instance that moves between calls.
3. INVALIDATION: a camera that only rotates, a refit and a resize each rerun the pass and give a fresh context's image; a lens and
   count_traversal fall back to the root (primary_entry_on = 0).
4. The RULE of primary_entry = -1: records from 720 paths per record on, and for smaller calls from the second call with the same
   view on."""
import ctypes
import os
import sys

import numpy as np
import pytest

import primary_entry_model as model
import traversal_scenes as ts
from test_primary_order import same, scenes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
CW, CH = 16, 12  # coverage frames: 2 x 2 tiles, the right and the bottom ones partly outside the image


@pytest.fixture(autouse=True)
def ordered_everywhere(monkeypatch):
    monkeypatch.setenv("RFWHIP_PRIMARY_ORDER", "1")  # (the snapshot rides on the ordered table; small frames have none by the rule)


def passes(c):
    return c.get_kernel_time("primary_entry")[1]


def snapshot(c):
    """(view, W, H, g, root, K, ordered table, records) of the context's last snapshot"""
    fn = c._fn("emu_primary_entry")
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    info = np.zeros(36, np.uint32)
    assert fn(c._ctx, info.ctypes.data, None, 0, None, 0) == 0
    assert info[35] == 1
    nodes, rec = np.zeros(int(info[34]), model.NODE4F), np.zeros((int(info[33]), int(info[32])), np.uint32)
    assert fn(c._ctx, info.ctypes.data, nodes.ctypes.data, nodes.nbytes, rec.ctypes.data, rec.size) == 0
    f = info[:14].view(np.float32)
    view = model.View(f[0:3], f[3:6], f[6:9], f[9:12], f[12], f[13])
    return view, int(info[14]), int(info[15]), 1 << int(info[18]), int(info[24]), int(info[32]), nodes, rec


def context(make, scene, w, h, spp, group=64, **settings):
    c = make()
    c.init(w, h)
    for k, v in settings.items():
        if k == "flat_instances":
            c.set_setting(k, v)
    scene.upload(c)
    # (primary_entry = 1: records for every view; the rule of -1 has a test of its own)
    for k, v in {**dict(integrator="pt", spp=spp, sample_group=group, max_depth=1, primary_entry=1), **settings}.items():
        if k != "flat_instances":  # (a scene setting: it goes in front of the upload)
            c.set_setting(k, v)
    return c


def camera(pkg, w, h, origin, target):
    cam = pkg.Camera(aperture=0.0, FOV=40.0, focalDistance=5.0)
    cam.resize(w, h)
    cam.look_at(origin, target)
    return cam


def coverage_cases(pkg):
    terrain = pkg.scenes.terrain(n=16, width=CW, height_px=CH)
    torture = ts.torture(pkg)
    box = (-10.0, 1.0, 8.0)  # the centre of "outer_box" (and of "inner_box" inside it)
    return {
        "terrain_own": (terrain, terrain.camera, {}),
        "terrain_grazing": (terrain, camera(pkg, CW, CH, (2.0, 4.0, -62.0), (0.0, 3.6, 50.0)), {}),
        "torture_flat": (torture, camera(pkg, CW, CH, (2.0, 6.0, -24.0), (2.0, 0.5, 4.0)), {"flat_instances": 1}),
        "torture_instances": (torture, camera(pkg, CW, CH, (2.0, 6.0, -24.0), (2.0, 0.5, 4.0)), {"flat_instances": 0}),
        "inside_a_box": (torture, camera(pkg, CW, CH, box, (box[0] + 1.0, box[1] + 0.2, box[2] + 0.3)), {"flat_instances": 1}),
        "looking_away": (torture, camera(pkg, CW, CH, (0.0, 40.0, 0.0), (3.0, 80.0, 5.0)), {"flat_instances": 1}),
        "smaller_than_a_pixel": (torture, camera(pkg, CW, CH, (1.2e5, 0.9e5, -1.6e5), (0.0, 0.0, 5.0)), {"flat_instances": 0}),
    }


@pytest.mark.parametrize("name,group", [("terrain_own", 64), ("terrain_own", 8), ("terrain_grazing", 64), ("torture_flat", 64), ("torture_instances", 64),
                                        ("inside_a_box", 64), ("inside_a_box", 8), ("looking_away", 64), ("smaller_than_a_pixel", 64)])
def test_records_equal_the_model_and_cover_every_ray(pkg, make_emu, name, group):
    scene, cam, settings = coverage_cases(pkg)[name]
    c = context(make_emu, scene, CW, CH, group, group, **settings)
    c.render_frame(cam, pkg.RESET)
    assert c.get_setting("primary_entry_on") == "1" and passes(c) == 1
    view, w, h, g, root, K, nodes, rec = snapshot(c)
    c.destroy()
    assert (w, h, g) == (CW, CH, group) and len(rec) == model.groups_of(w, h, g) and K == 8
    rng = np.random.default_rng(5)
    uncovered = entered = used = deepest = 0
    for grp in range(len(rec)):
        pixels = model.group_pixels(w, h, g, grp)
        want, expanded = model.record(nodes, root, view, pixels, K)
        assert [int(x) for x in rec[grp]] == want, (name, grp)
        used += sum(x != model.ENTRY_DONE for x in want)
        deepest = max(deepest, len(expanded))
        if pixels:
            bad, seen = model.coverage(nodes, root, view, want, expanded, model.rays(view, pixels, 256 if g == 64 else 60, rng))
            uncovered, entered = uncovered + bad, entered + seen
    print(name, group, "records", len(rec), "words used", used, "nodes entered", entered, "uncovered", uncovered)
    assert uncovered == 0
    if name == "looking_away":
        assert used == 0  # every record is empty: every ray misses
    else:
        assert used > 0
    if name.startswith("terrain"):
        assert deepest >= 3  # the walk went well below the root somewhere


# ---- renders: on against off ------------------------------------------------------------------------------------------------------
def render(c, cam, pkg, calls=1, local=False):
    for k in range(calls):
        c.render_frame(cam, pkg.RESET if k == 0 else pkg.CONVERGE)
    st = c.get_stats()
    if local:  # one rank of several: its own strips (the emulation's device memory is host memory)
        img = np.zeros((c.local_rows(), c.width, 4), np.float32)
        c.read_local_framebuffer_device(img.ctypes.data)
        return {"image": img, "hits": {}, "counts": (st.primaryCount, st.secondaryCount, st.deepCount, st.shadowCount), "lit": bool((img[..., :3] > 0).any())}
    return {"image": c.framebuffer(), "hits": c.primary_hits(), "counts": (st.primaryCount, st.secondaryCount, st.deepCount, st.shadowCount)}


def on_off(pkg, make, scene, w, h, spp, group, cam=None, calls=1, local=False, **settings):
    out = []
    for entry in (0, 1):
        c = context(make, scene, w, h, spp, group, primary_entry=entry, **settings)
        out.append(render(c, cam or scene.camera, pkg, calls, local))
        assert c.get_setting("primary_entry_on") == str(entry)
        assert passes(c) == entry
        c.destroy()
    assert out[0]["lit"] if local else (out[0]["hits"]["prim"] >= 0).any()
    same(out[1], out[0])


@pytest.mark.parametrize("group", [8, 64])
def test_on_equals_off_with_remainder_tiles(pkg, make_emu, group):
    on_off(pkg, make_emu, pkg.scenes.terrain(n=32, width=44, height_px=27), 44, 27, 64, group, calls=2)


def test_on_equals_off_with_single_samples(pkg):
    """g = 1: a wave is an 8 x 8 tile of one sample.  Frames that small take the one-ray-per-lane kernel by the packet rule, so this
    library is built with the rule's threshold at one path slot."""
    import build_emu
    lib = ctypes.CDLL(build_emu.build(defines=("-DRT_PRIMARY_PACKET_MIN=1u",), tag="_packet1"))
    on_off(pkg, lambda: pkg._binding.CoreBinding(lib, "rfwhip_", 0, 0, 1), pkg.scenes.terrain(n=32, width=44, height_px=27), 44, 27, 3, 1)


@pytest.mark.parametrize("rank", [0, 1])
def test_on_equals_off_on_two_strips(pkg, make_emu, rank):
    on_off(pkg, lambda: make_emu(rank, 2), pkg.scenes.terrain(n=32, width=44, height_px=40), 44, 40, 64, 64, local=True)


@pytest.mark.parametrize("name", ["cornell_instances", "terrain_inside"])
def test_on_equals_off_with_instances_and_inside_the_bounds(pkg, make_emu, name):
    on_off(pkg, make_emu, scenes(pkg)[name](), 96, 64, 64, 64)


def test_on_equals_off_with_a_moving_instance(pkg, make_emu):
    scene = ts.torture(pkg)
    cam = camera(pkg, 40, 24, (2.0, 6.0, -24.0), (2.0, 0.5, 4.0))
    out = []
    for entry in (0, 1):
        c = context(make_emu, scene, 40, 24, 64, 64, primary_entry=entry, flat_instances=0)
        frames = [render(c, cam, pkg)]
        i = scene.parts["rotated"]
        c.set_instance(i, scene.instances[i]["mesh"] if isinstance(scene.instances[i], dict) else scene.instances[i][0], ts.translate(1.5, 0.4, 1.0) @ ts.rotation((1, 2, 3), 80.0))
        c.update()
        frames.append(render(c, cam, pkg))
        assert passes(c) == 2 * entry  # (the tree over the instances was rebuilt: new table, new records)
        c.destroy()
        out.append(frames)
    assert out[0][0]["hits"]["t"].tobytes() != out[0][1]["hits"]["t"].tobytes()  # (the scene is unlit: the hit records show the move)
    for a, b in zip(out[1], out[0]):
        same(a, b)


# ---- invalidation -----------------------------------------------------------------------------------------------------------------
W, H = 40, 24


def fresh(pkg, make_emu, scene, cam, w=W, h=H, prepare=None):
    c = context(make_emu, scene, w, h, 64, 64, primary_entry=0)
    if prepare:
        prepare(c)
    out = render(c, cam, pkg)
    c.destroy()
    return out


def test_a_camera_that_only_rotates_reruns_the_pass(pkg, make_emu):
    scene = pkg.scenes.terrain(n=32, width=W, height_px=H)
    cam = scene.camera
    c = context(make_emu, scene, W, H, 64, 64)
    render(c, cam, pkg)
    render(c, cam, pkg)
    assert passes(c) == 1 and c.get_kernel_time("primary_order")[1] == 1
    d = np.asarray(cam.direction, np.float64) + (0.2, -0.05, 0.0)
    cam.direction = tuple(float(x) for x in d / np.linalg.norm(d))
    got = render(c, cam, pkg)
    assert passes(c) == 2 and c.get_kernel_time("primary_order")[1] == 1  # (the position's bits are the same: the ordered table stays)
    c.destroy()
    same(got, fresh(pkg, make_emu, scene, cam))


def test_a_refit_reruns_the_pass(pkg, make_emu):
    rings, seg = 24, 16
    scene = pkg.scenes.skinned_tube(0.0, rings=rings, seg=seg, width=W, height=H)
    v, idx, vn, joints, weights = pkg.scenes.skinned_tube_rig(rings, seg)
    scene.meshes[0]["triangles"] = pkg.scenes.make_triangles(v, idx, normals=vn, material=scene.meshes[0]["triangles"]["material"][0])

    def pose(c):
        c.set_mesh_skin(0, joints, weights, vn)
        c.pose_mesh(0, pkg.scenes.skinned_tube_joint_matrices(3.0))
        c.update()
    c = context(make_emu, scene, W, H, 64, 64)
    c.set_mesh_skin(0, joints, weights, vn)
    before = render(c, scene.camera, pkg)
    assert passes(c) == 1
    c.pose_mesh(0, pkg.scenes.skinned_tube_joint_matrices(3.0))
    c.update()
    got = render(c, scene.camera, pkg)
    assert passes(c) == 2 and c.get_setting("primary_entry_on") == "1"
    c.destroy()
    assert got["image"].tobytes() != before["image"].tobytes()
    same(got, fresh(pkg, make_emu, scene, scene.camera, prepare=pose))


def test_a_resize_reruns_the_pass(pkg, make_emu):
    scene = pkg.scenes.terrain(n=32, width=W, height_px=H)
    c = context(make_emu, scene, W, H, 64, 64)
    render(c, scene.camera, pkg)
    w2, h2 = 28, 36
    c.init(w2, h2)
    scene.camera.resize(w2, h2)
    got = render(c, scene.camera, pkg)
    assert passes(c) == 2 and c.get_setting("primary_entry_on") == "1"
    c.destroy()
    same(got, fresh(pkg, make_emu, scene, scene.camera, w2, h2))


def test_a_lens_and_the_traversal_counters_start_at_the_root(pkg, make_emu):
    scene = pkg.scenes.terrain(n=32, width=W, height_px=H)
    c = context(make_emu, scene, W, H, 64, 64, primary_entry=1)
    assert c.get_setting("primary_entry") == "1"
    scene.camera.aperture = 0.05
    lens = render(c, scene.camera, pkg)
    assert c.get_setting("primary_entry_on") == "0" and passes(c) == 0
    scene.camera.aperture = 0.0
    render(c, scene.camera, pkg)
    assert c.get_setting("primary_entry_on") == "1" and passes(c) == 1
    c.set_setting("count_traversal", 1)
    counted = render(c, scene.camera, pkg)
    assert c.get_setting("primary_entry_on") == "0" and passes(c) == 1
    c.destroy()
    r = context(make_emu, scene, W, H, 64, 64, primary_entry=0, count_traversal=1)
    same(counted, render(r, scene.camera, pkg))
    scene.camera.aperture = 0.05
    same(lens, render(r, scene.camera, pkg))
    r.destroy()


def test_the_rule_waits_for_a_view_at_rest_or_a_large_call(pkg, make_emu):
    scene = pkg.scenes.terrain(n=32, width=16, height_px=8)
    cam = scene.camera
    c = context(make_emu, scene, 16, 8, 64, 64, primary_entry=-1)  # 64 paths per record
    seen = []
    for turn in (0.0, 0.0, 0.0, 0.1, 0.2, 0.2):
        cam.direction = tuple(float(x) for x in np.asarray([turn, -0.25, 1.0]) / np.linalg.norm([turn, -0.25, 1.0]))
        c.render_frame(cam, pkg.RESET)
        seen.append((c.get_setting("primary_entry_on"), passes(c)))
    # the first call of a view starts at the root; the second makes the records, the third reuses them; a camera that turns has none
    assert seen == [("0", 0), ("1", 1), ("1", 1), ("0", 1), ("0", 1), ("1", 2)]
    c.set_setting("spp", 768)  # 768 paths per record: worth a pass of its own
    cam.direction = (0.0, 0.0, 1.0)
    c.render_frame(cam, pkg.RESET)
    assert (c.get_setting("primary_entry_on"), passes(c)) == ("1", 3)
    c.destroy()
