"""Bloom on the device (k_bloom_down0, k_bloom_down, k_bloom_up, k_bloom_apply; work items: csrc/bloom.h): the CPU tier's sizes,
inputs and parameter sets on the HIP kernels, held to the same float64 model (tests/bloom_model.py) within the same counted bound —
the kernels and the emulation are each held to the model, not to each other (the compiler contracts a x b + c differently on the two
sides).  Then one 1920 x 1080 image, the display routes, the group with three display slots in flight, and rfwhip_display_stream on
two streams in turn."""
import numpy as np
import pytest

import bloom_model as bm
import display_model as dm
import test_bloom as cpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size", bm.SIZES, ids=lambda s: "%dx%d" % s)
def test_chain_matches_the_model(make_hip, size):
    w, h = size
    c = make_hip()
    c.init(w, h)
    print("%dx%d: largest error / bound %.3g" % (w, h, cpu.check_against_model(c, cpu.inputs(w, h), "%dx%d" % (w, h))))


def test_rendered_frame_matches_the_model(pkg, make_hip):
    c = make_hip()
    cpu._render(pkg, c)
    print("cornell: largest error / bound %.3g" % cpu.check_against_model(c, [("cornell", c.framebuffer())], "96x64"))


def test_known_answers_and_invariants(make_hip):
    c = make_hip()
    c.init(63, 17)
    cpu.check_known_answers(c, 63, 17)
    cpu.check_invariants(c, 63, 17)
    c.init(130, 70)
    cpu.check_invariants(c, 130, 70)


def test_full_size_image(make_hip):
    """1920 x 1080: 30 x 68 workgroups at level 1, levels of odd sizes (135, 68, 34, 17 rows), all six levels."""
    w, h = 1920, 1080
    c = make_hip()
    c.init(w, h)
    img = bm.lognormal(w, h)
    cpu._set(c)
    out = c.bloom_image(img, 1.0)
    m = bm.chain(img, 1.0)
    assert m["levels"] == 6
    print("1920x1080: largest error / bound %.3g" % bm.judge(out, cpu._levels(c, 6), m, img, "1920x1080 lognormal"))


def test_display_routes(pkg, make_hip):
    print("cornell: tolerance on the displayed values %.3g" % cpu.check_display_routes(pkg, make_hip(), make_hip()))


def test_off_means_off(pkg, make_hip):
    c = make_hip()
    cpu._render(pkg, c, 48, 32, 1)
    c.set_setting("stage_timing", 1)
    plain = c.display("rgba8")
    c.set_setting("display_bloom", 1)
    bloomed = c.display("rgba8")
    assert c.get_kernel_time("bloom", reset=True)[1] == 2 * bm.level_count(48, 32, 6)  # one count per launch of the chain
    c.set_setting("display_bloom", 0)
    assert np.array_equal(c.display("rgba8"), plain) and not np.array_equal(bloomed, plain)
    assert c.get_kernel_time("bloom")[1] == 0


def test_group_present_loop_with_three_frames_in_flight(pkg):
    cpu.check_group(pkg, pkg.context.load_library(), 2)


def test_display_stream_on_two_streams_in_turn(make_hip):
    """The pyramid and the bloomed image belong to the context: a call on another stream than the previous one waits for that
    chain and its display kernel.  Six calls alternating between two streams and two images give the single-stream bytes."""
    import torch
    w, h = 640, 360
    c, ref = make_hip(), make_hip()
    for x in (c, ref):
        x.init(w, h)
        x.set_setting("display_bloom", 1)
        x.set_setting("display_bloom_threshold", 0.5)
    imgs = [bm.lognormal(w, h, seed=5), bm.lognormal(w, h, seed=6)]
    want = [ref.display_image(img, 0.05, 1.0, "rgba8") for img in imgs]  # (no render yet: the reference's default camera values)
    assert not np.array_equal(want[0], want[1])
    dev = [torch.from_numpy(img).to("cuda:0") for img in imgs]
    streams = [torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")]
    outs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0") for _ in range(6)]
    torch.cuda.synchronize()
    for k in range(6):
        c.display_stream(dev[k & 1].data_ptr(), outs[k].data_ptr(), "rgba8", streams[k & 1].cuda_stream)
    torch.cuda.synchronize()
    for k in range(6):
        assert np.array_equal(outs[k].cpu().numpy(), want[k & 1]), k
