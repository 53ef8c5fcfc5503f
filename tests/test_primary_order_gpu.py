"""The primary wave's camera-ordered node table on the device (k_order4f, k_primary_packet<.., true>; csrc/primary_order.h): what
tests/test_primary_order.py checks on the emulation, on the HIP library.  Child order never decides a closest hit, so a render with
RFWHIP_PRIMARY_ORDER=1 is bit-equal to the one-ray-per-lane primary wave (refill=7) and to the packet form that sorts for itself
(RFWHIP_PRIMARY_ORDER=0): images, primary hits, per-depth counts.  96 x 64, 64 samples per pixel in one call."""
import numpy as np
import pytest

from test_primary_order import W, H, passes, render, same, scenes

pytestmark = pytest.mark.gpu
_REF = {}


@pytest.mark.parametrize("name", ["terrain", "cornell_instances", "cornell_lens", "terrain_inside"])
def test_ordered_render_equals_per_lane_and_sorting_kernels(pkg, make_hip, monkeypatch, name):
    scene = scenes(pkg)[name]()
    if name not in _REF:
        _REF[name] = render(make_hip, scene, monkeypatch, "0", 7), render(make_hip, scene, monkeypatch, "0", 15)
    lane, sorting = _REF[name]
    got = render(make_hip, scene, monkeypatch, "1", 15)
    assert lane["passes"] == 0 and sorting["passes"] == 0 and got["passes"] == 1
    assert lane["counts"][0] > 0 and (lane["hits"]["prim"] >= 0).any()
    same(got, lane)
    same(got, sorting)


def context(pkg, make_hip, monkeypatch, order, spp=64):
    monkeypatch.setenv("RFWHIP_PRIMARY_ORDER", order)
    scene = pkg.scenes.terrain(n=32, width=W, height_px=H)
    c = make_hip()
    c.init(W, H)
    scene.upload(c)
    for k, v in (("integrator", "pt"), ("spp", spp)):
        c.set_setting(k, v)
    return c, scene


def test_pipelined_calls_with_a_moving_camera(pkg, make_hip, monkeypatch):
    """Two calls enqueued without a wait in between, the camera moved for the second: the rewrite of the table for the second call
    is ordered behind the first call's primary wave, which still reads it.  Each image is the sorting kernel's of the same camera."""
    c, scene = context(pkg, make_hip, monkeypatch, "1")
    r, _ = context(pkg, make_hip, monkeypatch, "0")
    cam = scene.camera
    a, b = cam.position, (cam.position[0] + 7.0, cam.position[1] - 4.0, cam.position[2] + 30.0)
    want = {}
    for pos in (a, b):
        cam.position = pos
        r.render_frame(cam, pkg.RESET)
        want[pos] = r.framebuffer(), r.primary_hits()
    # (a RESET clears the accumulator: the image read after the second call is the second camera's alone; the first call's is
    # checked through the accumulated pair below)
    cam.position = a
    c.render_async(cam, pkg.RESET)
    cam.position = b
    c.render_async(cam, pkg.RESET)
    c.wait()
    assert passes(c) == 2
    assert c.framebuffer().tobytes() == want[b][0].tobytes()
    for k, v in c.primary_hits().items():
        assert v.tobytes() == want[b][1][k].tobytes(), k
    # the first call's samples, kept: RESET at a, CONVERGE at b, against the same pair on the sorting kernel
    for ctx in (c, r):
        cam.position = a
        ctx.render_async(cam, pkg.RESET)
        cam.position = b
        ctx.render_async(cam, pkg.CONVERGE)
        ctx.wait()
    assert c.framebuffer().tobytes() == r.framebuffer().tobytes()
    assert passes(c) == 4 and passes(r) == 0
    c.destroy(), r.destroy()


def test_pass_counts(pkg, make_hip, monkeypatch):
    c, scene = context(pkg, make_hip, monkeypatch, "1", spp=2)
    cam = scene.camera
    a, b = cam.position, (cam.position[0] + 0.5, cam.position[1], cam.position[2] - 1.0)
    seen = []
    for pos in (a, a, b, b, a):
        cam.position = pos
        c.render_frame(cam, pkg.RESET)
        seen.append(passes(c))
    assert seen == [1, 1, 2, 2, 3]
    c.set_setting("stage_timing", 1)  # (the milliseconds need the stage timers; the count does not)
    cam.position = b
    c.render_frame(cam, pkg.RESET)
    ms, n = c.get_kernel_time("primary_order")
    assert n == 4 and ms > 0.0
    c.destroy()
    r, scene = context(pkg, make_hip, monkeypatch, "0", spp=2)
    r.render_frame(scene.camera, pkg.RESET)
    assert passes(r) == 0
    r.destroy()
