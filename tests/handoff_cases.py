"""The display stage, the meter, bloom, grading and the JPEG encoder on streams that are not the context's own: what
tests/test_schedule.py replays under every schedule of the emulated streams and tests/test_display_gpu.py runs on the device.
A group's present_display_async / present_jpeg_async enqueue these stages on the root's gather stream; the reference is one
context that renders the same frames and reads display("rgba8") and display_jpeg() after each."""
import numpy as np

import display_grade_model as gm

W, H = 70, 51
SETTINGS = {"integrator": "pt", "spp": 1, "max_depth": 2, "display_bloom": 1, "display_grade": 1,
            "display_wb_temperature": 5000, "display_jpeg_restart": 2}


def scene(pkg):
    return pkg.scenes.terrain(n=24, width=W, height_px=H)


def setup(target, sc, extra):
    target.init(W, H)
    sc.upload(target)
    for k, v in dict(SETTINGS, **extra).items():
        target.set_setting(k, v)
    target.set_display_lut(gm.random_lut(5))


def _status(pkg, k):
    return pkg.RESET if k == 0 else pkg.CONVERGE


def reference(pkg, ctx, sc, extra, frames):
    """[(display("rgba8"), display_jpeg())] of `frames` frames, a RESET first and then CONVERGE."""
    setup(ctx, sc, extra)
    want = []
    for k in range(frames):
        ctx.render_frame(sc.camera, _status(pkg, k))
        want.append((ctx.display("rgba8"), ctx.display_jpeg()))
    return want


def displayed_group(pkg, g, sc, want):
    """Frames in flight through two slots: even frames as display images, odd frames as JPEG streams."""
    for k in range(len(want)):
        slot = k % 2
        g.render_async(sc.camera, _status(pkg, k))
        if k >= 2:  # the slot's earlier frame, k - 2: the same kind as this one
            _check_slot(g, slot, k - 2, want)
        if k % 2 == 0:
            g.present_display_async(slot, "rgba8")
        else:
            g.present_jpeg_async(slot)
    for k in range(len(want) - 2, len(want)):
        _check_slot(g, k % 2, k, want)


def _check_slot(g, slot, k, want):
    if k % 2 == 0:
        assert np.array_equal(g.present_display_wait(slot), want[k][0]), "display image of frame %d" % k
    else:
        assert g.present_jpeg_wait(slot) == want[k][1], "JPEG stream of frame %d" % k


def one_context_two_streams(pkg, g, sc, want, ev=0.5):
    """A group of one: every stage runs on the gather stream and again on the context's own stream within one frame, and a
    setting changed away and back marks the manual exposure record stale while both are enqueued."""
    c = g.contexts[0]
    for k in range(len(want)):
        g.render_async(sc.camera, _status(pkg, k))
        g.present_display_async(0, "rgba8")
        own = c.display("rgba8")
        g.present_jpeg_async(1)
        own_jpeg = c.display_jpeg()
        g.set_setting("display_exposure_ev", ev + 1.0)
        g.set_setting("display_exposure_ev", ev)
        slot = g.present_display_wait(0).copy()
        slot_jpeg = g.present_jpeg_wait(1)
        assert np.array_equal(slot, want[k][0]), "frame %d: display image on the gather stream" % k
        assert np.array_equal(own, want[k][0]), "frame %d: display image on the context's stream" % k
        assert slot_jpeg == want[k][1], "frame %d: JPEG stream on the gather stream" % k
        assert own_jpeg == want[k][1], "frame %d: JPEG stream on the context's stream" % k
