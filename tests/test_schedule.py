"""The same image under every legal schedule of the streams (CPU tier).

In the default emulation library every stream is immediate, so a missing stream wait cannot change an emulated image.  This
module loads the deferred-stream variant (tests/emu/build_emu.py with -DRFWHIP_EMU_STREAMS=1, csrc/emu_streams.h): every
launch, copy and event record is queued on its stream and runs only when a sync point needs it, in an order a policy picks
among the operations whose stream waits are satisfied — `late` (latest first: independent work as late as the dependencies
allow), `random` with a seed, or `eager` (latest first over everything enqueued, as a device runs independent work early:
an overwrite that should wait for an earlier reader).  A missing wait then changes the image deterministically.  Every case is compared bit for
bit with the `inorder` image of one ring entry and one stream."""
import copy
import ctypes

import numpy as np
import pytest

import denoise_temporal_model as M
import handoff_cases as H

INORDER, LATE, RANDOM, EAGER = 0, 1, 2, 3
# (eager: latest first over everything enqueued, needed by the sync point or not — a reader that a later writer must wait for)
POLICIES = [("late", LATE, 0), ("random-7", RANDOM, 7), ("random-1234", RANDOM, 1234), ("random-99991", RANDOM, 99991),
            ("eager", EAGER, 0)]
POLICY_IDS = [p[0] for p in POLICIES]


@pytest.fixture(scope="module")
def lib():
    import build_emu
    lib = ctypes.CDLL(build_emu.build(defines=("-DRFWHIP_EMU_STREAMS=1",), tag="_streams"))
    lib.rfwhip_emu_set_schedule.restype, lib.rfwhip_emu_set_schedule.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_uint]
    u64p = ctypes.POINTER(ctypes.c_ulonglong)
    lib.rfwhip_emu_schedule_stats.restype, lib.rfwhip_emu_schedule_stats.argtypes = ctypes.c_int, [u64p, u64p, u64p]
    yield lib
    lib.rfwhip_emu_set_schedule(INORDER, 0)


@pytest.fixture
def make_s(pkg, lib):
    def factory(rank=0, world=1):
        return pkg._binding.CoreBinding(lib, "rfwhip_", 0, rank, world)
    return factory


def _schedule(lib, policy, seed=0):
    assert lib.rfwhip_emu_set_schedule(policy, seed) == 0


def _stats(lib):
    ran, ooo, sp = ctypes.c_ulonglong(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
    assert lib.rfwhip_emu_schedule_stats(ctypes.byref(ran), ctypes.byref(ooo), ctypes.byref(sp)) == 0
    return {"ran": ran.value, "out_of_order": ooo.value, "shadow_packet_launches": sp.value}


def _pipelined(pkg, ctx, scene, w, h, settings, calls, wait_every):
    ctx.init(w, h)
    scene.upload(ctx)
    for k, v in settings.items():
        ctx.set_setting(k, v)
    for f in range(calls):
        ctx.render_async(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
        if wait_every and (f + 1) % wait_every == 0:
            ctx.wait()
    ctx.wait()
    return ctx.framebuffer()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# test_emu_parity.py::test_image_is_independent_of_how_calls_are_scheduled, row for row
MATRIX = (({"ring": 2}, 0), ({"ring": 4}, 0), ({"ring": 4}, 3), ({"ring": 4, "overlap": 1}, 0),
          ({"streams": 4, "sub_batch_paths": 1}, 0), ({"streams": 3, "sub_batch_paths": 1, "overlap": 1}, 2),
          ({"sample_group": 1}, 0), ({"sample_group": 2, "ring": 2}, 0), ({"sample_group": 64}, 1),
          ({"sample_group": 4, "streams": 2, "sub_batch_paths": 1}, 0),
          ({"fuse": 0}, 0), ({"fuse": 0, "ring": 4, "overlap": 1}, 0), ({"fuse": 0, "ring": 2}, 2),
          ({"refill": 7, "sample_group": 64}, 0), ({"refill": 0}, 0))


def test_inorder_equals_the_immediate_library(pkg, make_emu, make_s, lib):
    """`inorder` runs what a sync needs in the order the host issued it: the default library's images, bit for bit, and no
    operation ever runs ahead of an earlier one."""
    scene = pkg.scenes.cornell(64, 48)
    _schedule(lib, INORDER)
    for settings, wait_every in (({"integrator": "pt", "spp": 4, "max_depth": 2, "ring": 4}, 0),
                                 ({"integrator": "parity", "spp": 4, "streams": 4, "sub_batch_paths": 1}, 0),
                                 ({"integrator": "pt", "spp": 16, "max_depth": 3, "shadow_packets": 1, "fuse": 0, "ring": 2}, 0),
                                 ({"integrator": "pt", "spp": 4, "max_depth": 2, "denoise": 1}, 1)):
        a = _pipelined(pkg, make_emu(), scene, 64, 48, settings, 4, wait_every)
        b = _pipelined(pkg, make_s(), scene, 64, 48, settings, 4, wait_every)
        assert np.array_equal(_bits(a), _bits(b)), settings
    st = _stats(lib)
    assert st["ran"] > 0 and st["out_of_order"] == 0, st


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
@pytest.mark.parametrize("integrator", ["pt", "parity"])
def test_the_scheduling_matrix_under_every_schedule(pkg, make_s, lib, integrator, policy):
    name, pol, seed = policy
    scene = pkg.scenes.cornell(64, 48)
    base = {"integrator": integrator, "spp": 4, "max_depth": 2}
    _schedule(lib, INORDER)
    ref = _pipelined(pkg, make_s(), scene, 64, 48, dict(base, ring=1, streams=1), 6, 1)
    for extra, wait_every in MATRIX:
        _schedule(lib, pol, seed)
        img = _pipelined(pkg, make_s(), scene, 64, 48, dict(base, **extra), 6, wait_every)
        assert np.array_equal(img, ref), "%s: %s %s, wait_every=%d" % (name, integrator, extra, wait_every)


# the packet form of the depth-0 connection wave (sample groups >= 8): (settings, wait after every `wait_every` calls, spp)
PACKET_ROWS = (({"ring": 1}, 1, 16), ({"ring": 2}, 0, 16), ({"ring": 4}, 0, 16),
               ({"streams": 2, "sub_batch_paths": 1}, 0, 16), ({"streams": 4, "sub_batch_paths": 1}, 1, 32),
               ({"overlap": 0}, 1, 16), ({"overlap": 0, "ring": 4}, 0, 16), ({"overlap": 1, "ring": 2}, 0, 16))
PACKET_CALLS = 3


def _takes_packets(fuse, extra, wait_every):
    """Does some call of the row take the packet form?  Not on the side stream (`side` in rfwhip_render): a call that is not
    fused runs its connections there when overlap = 1, or by default when it is one sub-batch and nothing else is in flight."""
    overlap = extra.get("overlap", -1)
    fused = fuse == 1 and overlap != 1
    subs = extra.get("streams", 1)
    pipelined = wait_every != 1  # (every call after the first, when the row does not wait after each)
    side = not fused and (overlap == 1 or (overlap < 0 and subs == 1 and not pipelined))
    return not side


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
@pytest.mark.parametrize("fuse", [0, 1])
def test_shadow_packets_under_every_schedule(pkg, make_s, lib, fuse, policy):
    """spp 16 (32 for four sub-batches: 8 samples each), shadow_packets = 1: the depth-0 connection wave as packets, on the
    sub-batch's connection stream (shadow_side 1) or its own (0), fused or not, waited / pipelined / cut into sub-batches."""
    name, pol, seed = policy
    scene = pkg.scenes.cornell(64, 48)
    refs = {}
    for max_depth in (2, 3):
        for shadow_side in (0, 1):
            for extra, wait_every, spp in PACKET_ROWS:
                base = {"integrator": "pt", "spp": spp, "max_depth": max_depth, "shadow_packets": 1}
                if (spp, max_depth) not in refs:
                    _schedule(lib, INORDER)
                    refs[spp, max_depth] = _pipelined(pkg, make_s(), scene, 64, 48, dict(base, ring=1, streams=1), PACKET_CALLS, 1)
                settings = dict(base, fuse=fuse, shadow_side=shadow_side, **extra)
                _schedule(lib, pol, seed)
                c = make_s()
                img = _pipelined(pkg, c, scene, 64, 48, settings, PACKET_CALLS, wait_every)
                st = _stats(lib)
                row = "%s: %s, wait_every=%d" % (name, settings, wait_every)
                assert np.array_equal(img, refs[spp, max_depth]), row
                assert c.get_setting("shadow_packets_on") == "1", row
                if _takes_packets(fuse, extra, wait_every):
                    assert st["shadow_packet_launches"] > 0, "%s: the packet form never ran %s" % (row, st)
                else:
                    assert st["shadow_packet_launches"] == 0, "%s: the packet form ran on the side-stream path %s" % (row, st)


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
def test_changing_the_batch_size_between_pipelined_calls(pkg, make_s, lib, policy):
    """spp 2, 4, 2 in three pipelined calls: the ring is re-laid out behind a synchronisation."""
    name, pol, seed = policy
    scene = pkg.scenes.cornell(64, 48)
    out = []
    for p, s in ((INORDER, 0), (pol, seed)):
        _schedule(lib, p, s)
        a = make_s()
        a.init(64, 48)
        scene.upload(a)
        a.set_setting("integrator", "pt")
        a.set_setting("shadow_packets", 1)
        for k, spp in enumerate((2, 4, 8, 16, 2)):
            a.set_setting("spp", spp)
            a.render_async(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
        a.wait()
        out.append(a.framebuffer())
    assert np.array_equal(out[0], out[1]), name


def _group(pkg, lib, n):
    return pkg._binding.RenderGroup(lib, "rfwhip_", [0] * n, "peer")


def _setup(pkg, target, scene, w, h, settings):
    target.init(w, h)
    scene.upload(target)
    for k, v in settings.items():
        target.set_setting(k, v)


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
@pytest.mark.parametrize("n", [2, 3, 5])
def test_groups_under_every_schedule(pkg, make_s, lib, n, policy):
    name, pol, seed = policy
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    settings = {"integrator": "pt", "spp": 4, "max_depth": 2}
    _schedule(lib, INORDER)
    ref = make_s()
    _setup(pkg, ref, scene, 70, 51, settings)
    want = []
    for f in range(2):
        ref.render_frame(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
        want.append(ref.framebuffer())
    _schedule(lib, pol, seed)
    g = _group(pkg, lib, n)
    _setup(pkg, g, scene, 70, 51, settings)
    for f in range(2):
        g.render_async(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
    g.wait()
    assert np.array_equal(g.framebuffer(), want[1]), (name, n)
    assert np.array_equal(g.framebuffer(), want[1]), (name, n, "second gather")
    g.destroy()


def _moving_cameras(scene, frames):
    cams = []
    for k in range(frames):
        cam = copy.deepcopy(scene.camera)
        x, y, z = cam.position
        cam.position = (x + 0.35 * k, y + 0.11 * (k % 3), z + 0.2 * k)
        cams.append(cam)
    return cams


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
@pytest.mark.parametrize("n", [2, 4])
def test_frames_in_flight_under_every_schedule(pkg, make_s, lib, n, policy):
    """render(k), present_async(k % n), present_wait((k + 1) % n): the image handed out is frame k - n + 1's, bit for bit —
    a converging series with a still camera, then a new camera and a RESET every frame (strips of two frames would tear)."""
    name, pol, seed = policy
    w, h, frames = 64, 48, 7
    for moving in (False, True):
        scene = pkg.scenes.terrain(n=24, width=w, height_px=h) if moving else pkg.scenes.cornell(w, h, geometric_emitter=True)
        cams = _moving_cameras(scene, frames) if moving else [scene.camera] * frames
        status = [pkg.RESET if (moving or k == 0) else pkg.CONVERGE for k in range(frames)]
        settings = {"integrator": "pt", "spp": 1, "max_depth": 2}
        _schedule(lib, INORDER)
        ref = make_s()
        _setup(pkg, ref, scene, w, h, settings)
        want = []
        for k in range(frames):
            ref.render_frame(cams[k], status[k])
            want.append(ref.framebuffer())
        assert not np.array_equal(want[0], want[1])
        _schedule(lib, pol, seed)
        g = _group(pkg, lib, 3 if moving else 2)
        _setup(pkg, g, scene, w, h, settings)
        for k in range(frames):
            g.render_async(cams[k], status[k])
            g.present_async(k % n)
            if k >= n - 1:
                assert np.array_equal(g.present_wait((k + 1) % n), want[k - n + 1]), (name, moving, k)
        for k in range(frames - n + 1, frames):
            assert np.array_equal(g.present_wait(k % n), want[k]), (name, moving, k)
        g.destroy()


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
@pytest.mark.parametrize("n", [2, 3, 5])
def test_denoised_groups_under_every_schedule(pkg, make_s, lib, n, policy):
    name, pol, seed = policy
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    settings = {"integrator": "pt", "spp": 4, "max_depth": 2, "denoise": 1}
    _schedule(lib, INORDER)
    ref = make_s()
    _setup(pkg, ref, scene, 70, 51, settings)
    want = []
    for f in range(2):
        ref.render_frame(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
        want.append(ref.framebuffer())
    ref.set_setting("denoise", 0)
    raw = ref.framebuffer()
    _schedule(lib, pol, seed)
    g = _group(pkg, lib, n)
    _setup(pkg, g, scene, 70, 51, settings)
    for f in range(2):
        g.render_frame(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
        assert np.array_equal(g.framebuffer(), want[f]), (name, n, f)
    assert np.array_equal(g.framebuffer(), want[1]), (name, n, "repeated read")
    # strip-local reads are never denoised; the root's de-interleave of them is the raw image (numpy buffers stand in for device
    # memory: the two hooks synchronise the context's stream before they return)
    lr = g.contexts[0].local_rows()
    gathered = np.zeros((n, lr, 70, 4), np.float32)
    for r, ctx in enumerate(g.contexts):
        ctx.read_local_framebuffer_device(gathered[r].ctypes.data)
    full = np.zeros((51, 70, 4), np.float32)
    g.contexts[0].deinterleave_device(gathered.ctypes.data, full.ctypes.data)
    assert np.array_equal(full, raw), (name, n)
    g.destroy()


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
@pytest.mark.parametrize("n", [2, 3])
def test_temporal_denoised_groups_under_every_schedule(pkg, make_s, lib, n, policy):
    name, pol, seed = policy
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    settings = {"integrator": "pt", "spp": 1, "max_depth": 2, "denoise": 1, "denoise_temporal": 1}
    cams = [M.panned(scene.camera, 0.4 * f) for f in range(5)]
    _schedule(lib, INORDER)
    ref = make_s()
    _setup(pkg, ref, scene, 70, 51, settings)
    want = []
    for cam in cams:
        ref.render_frame(cam, pkg.RESET)
        want.append(ref.framebuffer())
    again = ref.framebuffer()
    assert np.array_equal(_bits(again), _bits(want[-1]))
    _schedule(lib, pol, seed)
    g = _group(pkg, lib, n)
    _setup(pkg, g, scene, 70, 51, settings)
    for f, cam in enumerate(cams):
        g.render_frame(cam, pkg.RESET)
        assert np.array_equal(_bits(g.framebuffer()), _bits(want[f])), (name, n, f)
    # repeated reads of an unchanged scene (the two history sets)
    assert np.array_equal(_bits(g.framebuffer()), _bits(want[-1])), (name, n, "repeated read")
    assert np.array_equal(_bits(g.framebuffer()), _bits(want[-1])), (name, n, "third read")
    g.destroy()


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
@pytest.mark.parametrize("n", [2, 3])
def test_displayed_groups_under_every_schedule(pkg, make_s, lib, n, policy):
    """The display stage with auto exposure, bloom, grading through a LUT, and the JPEG encoder, enqueued on the root's gather
    stream with two frames in flight: every image and every JPEG stream is the single context's for that frame."""
    name, pol, seed = policy
    scene, extra = H.scene(pkg), {"display_exposure": "auto"}
    _schedule(lib, INORDER)
    want = H.reference(pkg, make_s(), scene, extra, 6)
    _schedule(lib, pol, seed)
    g = _group(pkg, lib, n)
    H.setup(g, scene, extra)
    H.displayed_group(pkg, g, scene, want)
    g.destroy()


@pytest.mark.parametrize("policy", POLICIES, ids=POLICY_IDS)
def test_one_context_on_two_streams_under_every_schedule(pkg, make_s, lib, policy):
    """A group of one: the meter, bloom, the graded display kernel and the encoder of one context on its gather stream and on
    its own stream in turn (manual exposure: under `auto` a stream call and a host read step the meter differently)."""
    name, pol, seed = policy
    scene, extra = H.scene(pkg), {"display_exposure_ev": 0.5}
    _schedule(lib, INORDER)
    want = H.reference(pkg, make_s(), scene, extra, 4)
    _schedule(lib, pol, seed)
    g = _group(pkg, lib, 1)
    H.setup(g, scene, extra)
    H.one_context_two_streams(pkg, g, scene, want)
    g.destroy()


def test_the_late_schedule_reorders(pkg, make_s, lib):
    """Not vacuous: under `late` a pipelined ring-4 series and a group with frames in flight run operations ahead of
    earlier ones (and under `inorder` nothing does)."""
    scene = pkg.scenes.cornell(64, 48)
    settings = {"integrator": "pt", "spp": 16, "max_depth": 3, "shadow_packets": 1, "ring": 4}
    for pol in (INORDER, LATE):
        _schedule(lib, pol)
        _pipelined(pkg, make_s(), scene, 64, 48, settings, 4, 0)
        st = _stats(lib)
        assert st["shadow_packet_launches"] > 0
        assert (st["out_of_order"] > 0) == (pol == LATE), (pol, st)
    for pol in (INORDER, LATE):
        _schedule(lib, pol)
        g = _group(pkg, lib, 2)
        _setup(pkg, g, scene, 64, 48, {"integrator": "pt", "spp": 1, "max_depth": 2})
        for k in range(4):
            g.render_async(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
            g.present_async(k % 2)
            if k >= 1:
                g.present_wait((k + 1) % 2)
        g.wait()
        st = _stats(lib)
        assert (st["out_of_order"] > 0) == (pol == LATE), (pol, st)
        g.destroy()
