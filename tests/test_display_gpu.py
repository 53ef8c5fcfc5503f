"""The display stage on the device (k_display, kernels.hip; work item: csrc/display.h): the LDS tile, its halo and the ragged
edges against the float64 model of tests/display_model.py, the rendered frame on HIP and in the emulation (each held to the model
on its own framebuffer: the two are not required to agree bit for bit), one full-size image, and the group, comm and
stream-ordered entry points against the single context."""
import numpy as np
import pytest

import display_model as dm
import handoff_cases as H

pytestmark = pytest.mark.gpu


def _set(c, tonemap="aces", fxaa=1, srgb=0):
    c.set_setting("display_tonemap", tonemap)
    c.set_setting("display_fxaa", fxaa)
    c.set_setting("display_srgb", srgb)


def _judge_both(c, img, tonemap, fxaa, srgb, label):
    m = dm.display(img, 0.05, 1.0, tonemap, bool(fxaa), bool(srgb))
    f = c.display_image(img, 0.05, 1.0, "rgba32f")
    print("%s: float max |err| %.3g" % (label, float(np.abs(f - m["out"]).max())))
    ef = dm.judge(f, m, bool(srgb), label=label + " rgba32f")
    eb = dm.judge(c.display_image(img, 0.05, 1.0, "rgba8"), m, bool(srgb), label=label + " rgba8")
    print("%s: excused %d / %d of %d" % (label, ef, eb, img.shape[0] * img.shape[1]))


@pytest.mark.parametrize("size", dm.SIZES, ids=lambda s: "%dx%d" % s)
def test_display_image_matches_the_model(make_hip, size):
    """1 x 1 and 5 x 3: smaller than the halo, every tap clamps; 37 x 23: one ragged tile; 130 x 70: 3 x 5 tiles, the last ones
    partial in x and y."""
    w, h = size
    c = make_hip()
    c.init(w, h)
    for kind in dm.KINDS:
        img = dm.image(kind, w, h)
        for fxaa in (1, 0):
            _set(c, "aces", fxaa, 0)
            _judge_both(c, img, "aces", fxaa, 0, "%s %dx%d fxaa=%d" % (kind, w, h, fxaa))
    img = dm.image("noise", w, h)
    _set(c, "aces", 1, 1)
    _judge_both(c, img, "aces", 1, 1, "noise %dx%d srgb" % (w, h))
    _set(c, "none", 1, 0)
    _judge_both(c, img, "none", 1, 0, "noise %dx%d none" % (w, h))


def _render(pkg, c, scene, w, h, spp=4, **settings):
    c.init(w, h)
    scene.upload(c)
    c.set_setting("integrator", "pt")
    c.set_setting("spp", spp)
    for k, v in settings.items():
        c.set_setting(k, v)
    c.render_frame(scene.camera, pkg.RESET)
    return c


@pytest.mark.parametrize("which", ["hip", "emu"])
def test_rendered_frame(pkg, make_hip, make_emu, which):
    scene = pkg.scenes.cornell(96, 64)
    c = _render(pkg, (make_hip if which == "hip" else make_emu)(), scene, 96, 64)
    for denoise in (0, 1):
        c.set_setting("denoise", denoise)
        fb = c.framebuffer()
        m = dm.display(fb, scene.camera.brightness, scene.camera.contrast)
        dm.judge(c.display("rgba32f"), m, label="%s denoise=%d rgba32f" % (which, denoise))
        dm.judge(c.display("rgba8"), m, label="%s denoise=%d rgba8" % (which, denoise))
        assert np.array_equal(c.framebuffer().view(np.uint32), fb.view(np.uint32))


def test_full_size_image(make_hip):
    w, h = 1920, 1080
    c = make_hip()
    c.init(w, h)
    img = dm.image("stripes", w, h)
    m = dm.display(img, 0.05, 1.0)
    f = c.display_image(img, 0.05, 1.0, "rgba32f")
    print("1920x1080 stripes: float max |err| %.3g" % float(np.abs(f - m["out"]).max()))
    print("excused %d" % dm.judge(f, m, label="1920x1080 rgba32f"))
    dm.judge(c.display_image(img, 0.05, 1.0, "rgba8"), m, label="1920x1080 rgba8")


def test_group_on_one_device_equals_the_single_context(pkg, make_hip):
    scene = pkg.scenes.terrain(n=24, width=130, height_px=70)
    frames = 4
    one = make_hip()
    want = []
    for k in range(frames):
        if k == 0:
            _render(pkg, one, scene, 130, 70, spp=2, max_depth=2)
        else:
            one.render_frame(scene.camera, pkg.CONVERGE)
        want.append(one.display("rgba8"))
    g = pkg.render_group([0, 0], "peer")
    g.init(130, 70)
    scene.upload(g)
    for k, v in {"integrator": "pt", "spp": 2, "max_depth": 2}.items():
        g.set_setting(k, v)
    # three frames in flight through the display slots
    n = 3
    for k in range(frames):
        g.render_async(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
        g.present_display_async(k % n, "rgba8")
        if k >= n - 1:
            assert np.array_equal(g.present_display_wait((k + 1) % n), want[k - n + 1]), k
    for k in range(frames - n + 1, frames):
        assert np.array_equal(g.present_display_wait(k % n), want[k]), k
    assert np.array_equal(g.display("rgba8"), want[-1])
    assert np.array_equal(g.display("rgba32f"), one.display("rgba32f"))
    g.destroy()


def test_one_rank_comm_gather_then_display_on_the_callers_stream(pkg, make_hip):
    import torch
    scene = pkg.scenes.cornell(130, 70, geometric_emitter=True)
    ref = _render(pkg, make_hip(), scene, 130, 70)
    c = _render(pkg, make_hip(), scene, 130, 70)
    comm = pkg.RenderComm(c, None)
    full = torch.zeros((70, 130, 4), dtype=torch.float32, device="cuda:0")
    out8 = torch.zeros((70, 130, 4), dtype=torch.uint8, device="cuda:0")
    out32 = torch.zeros((70, 130, 4), dtype=torch.float32, device="cuda:0")
    comm.gather(full.data_ptr())
    comm.wait()
    stream = torch.cuda.current_stream().cuda_stream
    comm.display(full.data_ptr(), out8.data_ptr(), "rgba8", stream)
    comm.display(full.data_ptr(), out32.data_ptr(), "rgba32f", stream)
    torch.cuda.synchronize()
    assert np.array_equal(full.cpu().numpy(), ref.framebuffer())
    assert np.array_equal(out8.cpu().numpy(), ref.display("rgba8"))
    assert np.array_equal(out32.cpu().numpy(), ref.display("rgba32f"))
    # the device read of a plain context is the same image
    dev = torch.zeros((70, 130, 4), dtype=torch.uint8, device="cuda:0")
    ref.read_display_device(dev.data_ptr(), "rgba8")
    assert np.array_equal(dev.cpu().numpy(), ref.display("rgba8"))
    comm.destroy()


def test_one_context_on_two_streams(pkg):
    """tests/test_schedule.py's case of the same name on the device: a group of one runs the meter, bloom, the graded display
    kernel and the JPEG encoder on its gather stream and on the context's own stream within every frame."""
    scene, extra = H.scene(pkg), {"display_exposure_ev": 0.5}
    want = H.reference(pkg, pkg.RenderContext(device=0), scene, extra, 4)
    g = pkg._binding.RenderGroup(pkg.load_library(), "rfwhip_", [0], "peer")
    H.setup(g, scene, extra)
    H.one_context_two_streams(pkg, g, scene, want)
    g.destroy()
