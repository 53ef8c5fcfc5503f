"""The primary wave's camera-ordered node table (csrc/primary_order.h; include/rfwhip.h, kernel family 11), CPU tier, through the
host-emulation library.

1. The ordering ITEM against the float64 model of tests/primary_order_model.py, through rfwhip_emu_order4f (an entry of the emulation
   libraries only).  On a grid of 1/8 in [-8, 8] every difference, square and sum of three squares is exact in float32 (< 2^24 in
   units of 1/64), so the float32 item and the float64 model compute the SAME keys and the tables must agree byte for byte, ties
   included; on arbitrary float32 planes the table must be a permutation sorted under the float64 keys up to the rounding of a
   float32 sum of three squares (relative 4 x 2^-24, taken as 1e-6).
2. RENDERS with RFWHIP_PRIMARY_ORDER=1 against the one-ray-per-lane primary wave (refill=7) of the same library: child order never
   decides a closest hit, so images, primary hits and per-depth counts are bit-equal.
3. The PASS COUNT (get_kernel_time("primary_order")): one pass per distinct camera position, one more after a refit, none with =0."""
import ctypes

import numpy as np
import pytest

import primary_order_model as model

W, H, SPP = 96, 64, 64
_REF = {}


@pytest.fixture
def order4f(emu_lib):
    fn = emu_lib.rfwhip_emu_order4f
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int]

    def run(nodes, origin, ordered=1):
        nodes = np.ascontiguousarray(nodes)
        out = np.zeros_like(nodes)
        c = np.asarray(origin, np.float32)
        assert fn(nodes.ctypes.data, out.ctypes.data, len(nodes), c.ctypes.data, ordered) == 0
        return out
    return run


def children(nodes):
    """(n, 4, 8) words: a child's six planes, entry and pad side by side."""
    return np.concatenate([np.moveaxis(nodes["lo"], 1, 2).view(np.uint32), np.moveaxis(nodes["hi"], 1, 2).view(np.uint32),
                           nodes["entry"][..., None], nodes["pad"][..., None]], -1)


def grid_nodes(rng, n):
    nodes = model.random_nodes(rng, n, grid=8)
    # exact ties: a child repeated under another entry (d2 and the centre distance tie: the slot decides), and boxes that share
    # their nearest face (d2 ties: the centre decides)
    for i in range(0, n, 3):
        a, b = rng.choice(4, 2, replace=False)
        nodes["lo"][i][:, b], nodes["hi"][i][:, b] = nodes["lo"][i][:, a], nodes["hi"][i][:, a]
    for i in range(1, n, 3):
        a, b = rng.choice(4, 2, replace=False)
        nodes["lo"][i][:, b] = nodes["lo"][i][:, a]
        nodes["hi"][i][:, b] = np.maximum(nodes["lo"][i][:, a], nodes["hi"][i][:, b])
    return nodes


def test_item_equals_the_model_on_exact_keys(order4f):
    rng = np.random.default_rng(1)
    nodes = grid_nodes(rng, 1500)
    origins = [np.round(rng.uniform(-9, 9, 3) * 8) / 8 for _ in range(3)]
    origins.append((nodes[5]["lo"][:, 0] + nodes[5]["hi"][:, 0]) * 0.5)  # inside a box (its centre) ...
    origins.append(nodes[7]["lo"][:, 1].astype(np.float64))              # ... and on a corner
    origins.append(np.zeros(3))                                          # inside most boxes: d2 = 0 ties
    ties = 0
    for c in origins:
        got, want = order4f(nodes, c), model.order(nodes, c)
        assert got.tobytes() == want.tobytes(), c
        assert order4f(nodes, c).tobytes() == got.tobytes()  # the same table on a second run
        for n in nodes[:200]:
            e, d2, dc2 = model.keys(n, c)
            ties += len({d2[j] for j in range(4) if not e[j]}) < int((~e).sum())  # two live children at one distance
    assert ties > 50  # (the cases the tie rules exist for did occur)
    assert order4f(nodes, origins[0], ordered=0).tobytes() == nodes.tobytes()


def test_item_on_arbitrary_planes(order4f):
    rng = np.random.default_rng(2)
    nodes = model.random_nodes(rng, 3000)
    for c in (rng.uniform(-9, 9, 3), nodes[3]["lo"][:, 2] * 0.25 + nodes[3]["hi"][:, 2] * 0.75, (100.0, -50.0, 3.0)):
        c = np.asarray(c, np.float32)
        got = order4f(nodes, c)
        a, b = children(nodes), children(got)
        # a permutation of the children, planes and entry together; nothing else of the node
        key = lambda x: np.sort(np.ascontiguousarray(x).view([("", np.uint32)] * 8).reshape(len(x), 4), 1)
        assert (key(a) == key(b)).all()
        for n in got:
            e, d2, dc2 = model.keys(n, c)
            live = int((~e).sum())
            assert not e[:live].any() and e[live:].all()  # unused slots last ...
            for j in range(live, 4):                      # ... still unused
                assert n["entry"][j] == model.ENTRY_EMPTY or (n["lo"][:, j] > n["hi"][:, j]).any()
            for j in range(live - 1):
                assert d2[j] <= d2[j + 1] * (1 + 1e-6) + 1e-30, (n, c)
                if d2[j] == d2[j + 1] == 0.0:
                    assert dc2[j] <= dc2[j + 1] * (1 + 1e-6), (n, c)
        # unused slots keep their slot order
        for n_in, n_out in zip(nodes[:500], got[:500]):
            e_in = model.keys(n_in, c)[0]
            want = children(n_in[None])[0][e_in]
            assert (children(n_out[None])[0][4 - len(want):] == want).all()


# ---- renders ----------------------------------------------------------------------------------------------------------------------
def scenes(pkg):
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import golden_scenes

    def terrain_inside():
        s = pkg.scenes.terrain(n=32, width=W, height_px=H)
        s.camera.look_at((3.0, 2.5, -8.0), (20.0, 0.5, 30.0))  # inside the terrain's bounds (|x|, |z| <= 50, y within its relief)
        return s
    return {"terrain": lambda: pkg.scenes.terrain(n=32, width=W, height_px=H), "cornell_instances": lambda: golden_scenes.cornell_pt(pkg, W, H),
            "cornell_lens": lambda: golden_scenes.cornell_lens(pkg, W, H), "terrain_inside": terrain_inside}


def render(make, scene, monkeypatch, order, refill, spp=SPP, calls=1):
    monkeypatch.setenv("RFWHIP_PRIMARY_ORDER", order)
    c = make()
    c.init(W, H)
    scene.upload(c)
    for k, v in (("integrator", "pt"), ("spp", spp), ("refill", refill)):
        c.set_setting(k, v)
    for k in range(calls):
        c.render_frame(scene.camera, pkg_status(k))
    st = c.get_stats()
    out = {"image": c.framebuffer(), "hits": c.primary_hits(), "counts": (st.primaryCount, st.secondaryCount, st.deepCount, st.shadowCount),
           "passes": c.get_kernel_time("primary_order")[1]}
    c.destroy()
    return out


def pkg_status(k):
    return 0 if k == 0 else 1  # RFW_RESET, RFW_CONVERGE


def same(a, b):
    assert a["image"].tobytes() == b["image"].tobytes()
    for k in a["hits"]:
        assert a["hits"][k].tobytes() == b["hits"][k].tobytes(), k
    assert a["counts"] == b["counts"]


@pytest.mark.parametrize("name", ["terrain", "cornell_instances", "cornell_lens", "terrain_inside"])
def test_ordered_render_equals_the_per_lane_primary_wave(pkg, make_emu, monkeypatch, name):
    assert (pkg.RESET, pkg.CONVERGE) == (0, 1)
    scene = scenes(pkg)[name]()
    if name not in _REF:
        _REF[name] = render(make_emu, scene, monkeypatch, "0", 7)
    ref = _REF[name]
    got = render(make_emu, scene, monkeypatch, "1", 15)
    assert ref["passes"] == 0 and got["passes"] == 1
    assert ref["counts"][0] > 0 and (ref["hits"]["prim"] >= 0).any()
    same(got, ref)


def small(pkg, make_emu, monkeypatch, order, scene=None):
    monkeypatch.setenv("RFWHIP_PRIMARY_ORDER", order)
    scene = scene or pkg.scenes.cornell(32, 16, geometric_emitter=True)
    c = make_emu()
    c.init(32, 16)
    scene.upload(c)
    for k, v in (("integrator", "pt"), ("spp", 2)):
        c.set_setting(k, v)
    return c, scene


def passes(c):
    return c.get_kernel_time("primary_order")[1]


def test_one_pass_per_camera_position(pkg, make_emu, monkeypatch):
    c, scene = small(pkg, make_emu, monkeypatch, "1")
    cam = scene.camera
    a, b = cam.position, (cam.position[0] + 0.5, cam.position[1], cam.position[2] - 1.0)
    seen = []
    for pos in (a, a, b, b, a):
        cam.position = pos
        c.render_frame(cam, pkg.RESET)
        seen.append(passes(c))
    assert seen == [1, 1, 2, 2, 3]
    c.render_frame(cam, pkg.CONVERGE)
    cam.direction = (0.1, 0.0, 0.995)  # (the position's bits decide, nothing else of the camera)
    c.render_frame(cam, pkg.RESET)
    assert passes(c) == 3
    c.destroy()


def test_switched_off_and_small_calls_keep_the_sorting_kernel(pkg, make_emu, monkeypatch):
    c, scene = small(pkg, make_emu, monkeypatch, "0")
    c.render_frame(scene.camera, pkg.RESET)
    assert passes(c) == 0
    c.destroy()
    monkeypatch.delenv("RFWHIP_PRIMARY_ORDER")
    # by the rule: 32 x 16 x 2 path slots are fewer than the bytes a pass over this table moves
    c = make_emu()
    c.init(32, 16)
    big = pkg.scenes.terrain(n=32, width=32, height_px=16)
    big.upload(c)
    for k, v in (("integrator", "pt"), ("spp", 2)):
        c.set_setting(k, v)
    c.render_frame(big.camera, pkg.RESET)
    assert passes(c) == 0
    c.destroy()
    # ... and 96 x 64 x 64 are more than those of the Cornell box's
    c = make_emu()
    c.init(W, H)
    s = pkg.scenes.cornell(W, H, geometric_emitter=True)
    s.upload(c)
    for k, v in (("integrator", "pt"), ("spp", 64), ("max_depth", 0)):
        c.set_setting(k, v)
    c.render_frame(s.camera, pkg.RESET)
    assert passes(c) == 1
    c.destroy()


def test_a_refit_reruns_the_pass(pkg, make_emu, monkeypatch):
    rings, seg = 24, 16
    scene = pkg.scenes.skinned_tube(0.0, rings=rings, seg=seg, width=32, height=16)
    v, idx, vn, joints, weights = pkg.scenes.skinned_tube_rig(rings, seg)
    scene.meshes[0]["triangles"] = pkg.scenes.make_triangles(v, idx, normals=vn, material=scene.meshes[0]["triangles"]["material"][0])
    c, _ = small(pkg, make_emu, monkeypatch, "1", scene)
    c.set_mesh_skin(0, joints, weights, vn)
    c.render_frame(scene.camera, pkg.RESET)
    c.render_frame(scene.camera, pkg.RESET)
    assert passes(c) == 1
    c.pose_mesh(0, pkg.scenes.skinned_tube_joint_matrices(3.0))
    c.update()
    c.render_frame(scene.camera, pkg.RESET)
    img = c.framebuffer()
    assert passes(c) == 2
    c.destroy()
    # ... and the posed image is the per-lane kernels'
    r, _ = small(pkg, make_emu, monkeypatch, "0", scene)
    r.set_setting("refill", 7)
    r.set_mesh_skin(0, joints, weights, vn)
    r.pose_mesh(0, pkg.scenes.skinned_tube_joint_matrices(3.0))
    r.update()
    r.render_frame(scene.camera, pkg.RESET)
    assert r.framebuffer().tobytes() == img.tobytes()
    r.destroy()
