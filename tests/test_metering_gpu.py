"""The exposure meter on the device (k_meter_hist, k_meter_reduce, k_kat_meter, k_display_exposed; work items: csrc/metering.h):
the CPU tier's known answers, histograms, posed histograms and adaptation on HIP, held to the same float64 model
(tests/metering_model.py) — and against the emulation: histogram and `excluded` integer for integer, lambda, l_target and l bit for
bit.  E goes through exp2f, the device's and the host's: each lies within its counted bound of 2^l, so the two lie within
EXP2_ULPS + 1 ulp of each other; bit equality of E is NOT covered (the strict build has no exp2 of its own).  Then one full-size
image, the rendered frame, the group with three display slots in flight, and the one-rank comm with the display on the caller's
stream."""
import numpy as np
import pytest

import display_model as dm
import metering_model as mm
import test_metering as cpu

pytestmark = pytest.mark.gpu

BIT_EQUAL = ("log2_luminance", "log2_target", "log2_exposure", "valid", "excluded", "steps")


def same_step(hip, emu, label=""):
    """Two records of the same step: everything but E bit for bit, E within (EXP2_ULPS + 1) 2^-23 relative.  Returns E's share of that."""
    for k in BIT_EQUAL:
        assert np.array([hip[k]]).tobytes() == np.array([emu[k]]).tobytes(), "%s: %s differs, %r vs %r" % (label, k, hip[k], emu[k])
    r = abs(hip["exposure"] - emu["exposure"]) / ((mm.EXP2_ULPS + 1.0) * 2.0 ** -23 * emu["exposure"])
    assert r <= 1.0, "%s: E %r vs %r" % (label, hip["exposure"], emu["exposure"])
    return r


def test_meter_bin_known_answers(make_hip):
    c = make_hip()
    c.init(4, 4)
    cpu.check_meter_bin(c)


@pytest.mark.parametrize("size", mm.SIZES, ids=lambda s: "%dx%d" % s)
def test_histogram_matches_the_model_and_the_emulation(make_hip, make_emu, size):
    w, h = size
    c, e = make_hip(), make_emu()
    worst = 0.0
    for x in (c, e):
        x.init(w, h)
        cpu._auto(x)
    print("%dx%d: at most %d ambiguous pixels" % (w, h, cpu.check_histograms(c, w, h)))
    for kind in mm.KINDS + ("centres", "constant", "excluded"):
        img = (mm.bin_centres(w, h)[0] if kind == "centres" else mm.constant(w, h) if kind == "constant" else
               mm.all_excluded(w, h) if kind == "excluded" else dm.image(kind, w, h))
        for x in (c, e):
            x.meter_reset()
        (rh, bh), (re, be) = c.meter_image(img), e.meter_image(img)
        assert np.array_equal(bh, be), kind
        worst = max(worst, same_step(rh, re, "%s %dx%d" % (kind, w, h)))
        assert rh["steps"] == (1 if rh["valid"] else 0) and (kind != "excluded" or rh["valid"] == 0)
    print("%dx%d: E hip vs emulation, largest share of the bound %.3g" % (w, h, worst))


def test_reduce_on_posed_histograms(make_hip, make_emu):
    c, e = make_hip(), make_emu()
    c.init(8, 8), e.init(8, 8)
    print("posed histograms: largest error / bound %.3g" % cpu.check_posed(c))
    for label, bins, settings in cpu.posed_histograms():
        for x in (c, e):
            for k, v in mm.DEFAULTS.items():
                x.set_setting(k, v)
            cpu._auto(x, **settings)
            x.meter_reset()
        same_step(c.meter_from_histogram(bins, 5), e.meter_from_histogram(bins, 5), label)


def test_adaptation(make_hip, make_emu):
    w, h = 37, 23
    c, e = make_hip(), make_emu()
    c.init(w, h), e.init(w, h)
    print("adaptation: largest error / bound %.3g" % cpu.check_adaptation(c, w, h))
    a, b = dm.image("noise", w, h), 8.0 * dm.image("stripes", w, h)
    for x in (c, e):
        cpu._auto(x, speed=0.5)
        x.meter_reset()
    for k, img in enumerate((a, b, b, b)):
        same_step(c.meter_image(img)[0], e.meter_image(img)[0], "step %d" % k)


def test_full_size_image(make_hip, make_emu):
    """1920 x 1080: 1013 partial records — more than the reduce has threads per bin, several rounds of its fold."""
    w, h = 1920, 1080
    c, e = make_hip(), make_emu()
    c.init(w, h), e.init(w, h)
    cpu._auto(c), cpu._auto(e)
    img = dm.image("noise", w, h)
    rec, bins = c.meter_image(img)
    print("1920x1080 noise: %d ambiguous pixels" % mm.judge_histogram(bins, rec["excluded"], mm.histogram(img), "1920x1080 noise"))
    print("largest error / bound %.3g" % mm.judge_record(rec, bins, None, None, "1920x1080 noise"))
    re, be = e.meter_image(img)
    assert np.array_equal(bins, be)
    same_step(rec, re, "1920x1080 noise")
    rec, bins = c.meter_image(mm.constant(w, h))
    assert bins.max() == w * h and int(bins.sum()) == w * h


@pytest.mark.parametrize("which", ["hip", "emu"])
def test_rendered_frame_and_the_step_rule(pkg, make_hip, make_emu, which):
    print("cornell on %s: largest error / bound %.3g" % (which, cpu.check_rendered_frame(pkg, (make_hip if which == "hip" else make_emu)())))


def test_displayed_image_matches_the_model(make_hip):
    c = make_hip()
    c.init(130, 70)
    cpu.check_displayed_image(c, 130, 70)


def test_group_on_one_device_equals_the_single_context(pkg):
    cpu.check_group(pkg, pkg.context.load_library(), 2)


def test_one_rank_comm_gather_then_display_on_the_callers_stream(pkg, make_hip):
    import torch
    scene = pkg.scenes.cornell(130, 70, geometric_emitter=True)
    ref = cpu._render(pkg, make_hip(), scene, 130, 70)
    c = cpu._render(pkg, make_hip(), scene, 130, 70)
    for x in (ref, c):
        cpu._auto(x, speed=0.5)
    comm = pkg.RenderComm(c, None)
    full = torch.zeros((70, 130, 4), dtype=torch.float32, device="cuda:0")
    out8 = torch.zeros((70, 130, 4), dtype=torch.uint8, device="cuda:0")
    out32 = torch.zeros((70, 130, 4), dtype=torch.float32, device="cuda:0")
    comm.gather(full.data_ptr())
    comm.wait()
    stream = torch.cuda.current_stream().cuda_stream
    comm.display(full.data_ptr(), out8.data_ptr(), "rgba8", stream)   # every call is a step, on the caller's stream
    comm.display(full.data_ptr(), out32.data_ptr(), "rgba32f", stream)
    rec = c.meter()  # (waits for the steps on the caller's stream)
    torch.cuda.synchronize()
    fb = ref.framebuffer()
    b, k = scene.camera.brightness, scene.camera.contrast
    assert np.array_equal(out8.cpu().numpy(), ref.display_image(fb, b, k, "rgba8"))
    assert np.array_equal(out32.cpu().numpy(), ref.display_image(fb, b, k, "rgba32f"))
    assert rec == ref.meter() and rec["steps"] == 2
    comm.destroy()
