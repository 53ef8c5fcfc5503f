"""Baseline JPEG on the device (k_jpeg_blocks, k_jpeg_entropy, k_jpeg_offsets, k_jpeg_pack; csrc/display_jpeg.h): the CPU tier's
matrix on the HIP kernels, byte for byte against the numpy model (tests/jpeg_model.py); a rendered 480 x 270 frame against the full
model; one 1920 x 1080 frame — the coefficients against the vectorised model, the marker walk, and the stream byte for byte against
the emulation library's, which is held to the model at the small sizes; a group with three frames in flight; a one-rank comm
through rfwhip_display_jpeg_stream on the caller's stream."""
import ctypes

import numpy as np
import pytest

import display_jpeg_checks as ck
import jpeg_model as jm
from test_display_jpeg import SPECIAL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size", jm.SIZES, ids=lambda s: "%dx%d" % s)
def test_stream_matches_the_model(make_hip, size):
    w, h = size
    c = make_hip()
    c.init(w, h)
    for name, quality, sub, ri in ck.matrix(w, h):
        ck.stream_matches_the_model(c, name, w, h, quality, sub, ri)


def test_special_inputs_match_the_model(make_hip):
    c = make_hip()
    for case in SPECIAL:
        c.init(case[1], case[2])
        ck.stream_matches_the_model(c, *case)


def test_cap_one_byte_short(make_hip):
    c = make_hip()
    c.init(67, 35)
    ck.cap_one_byte_short_is_refused(c, "noise", 67, 35, 90, "420", 8)


def _render(pkg, c, scene, w, h, **settings):
    c.init(w, h)
    scene.upload(c)
    for k, v in dict({"integrator": "pt", "spp": 1, "max_depth": 2}, **settings).items():
        c.set_setting(k, v)
    c.render_frame(scene.camera, pkg.RESET)
    return c


def test_rendered_frame_against_the_full_model(pkg, make_hip):
    """480 x 270 of the terrain: display_jpeg() is the model's stream of display() of the same frame, which is the same bytes before
    and after; then "444" at quality 100 with Ri = 1: 2040 intervals."""
    w, h = 480, 270
    c = _render(pkg, make_hip(), pkg.scenes.terrain(n=48, width=w, height_px=h), w, h)
    before = c.display("rgba8")
    stream = c.display_jpeg()
    assert stream == jm.encode(before, 90, "420", 8)[0]
    assert np.array_equal(c.display("rgba8"), before)
    ck.configure(c, 100, "444", 1)
    want, facts = jm.encode(before, 100, "444", 1)
    assert facts["intervals"] == 60 * 34
    assert c.display_jpeg() == want and c.jpeg_record()["stuffed_bytes"] == facts["stuffed"]


def test_full_size_frame(pkg, make_hip, emu_lib):
    w, h = 1920, 1080
    c = _render(pkg, make_hip(), pkg.scenes.terrain(n=48, width=w, height_px=h), w, h)
    frame = c.display("rgba8")
    emu = pkg._binding.CoreBinding(emu_lib, "rfwhip_", 0, 0, 1)
    emu.init(w, h)
    for quality, sub, ri in ((90, "420", 8), (100, "444", 8), (25, "444", 65535)):
        ck.configure(c, quality, sub, ri)
        ck.configure(emu, quality, sub, ri)
        stream = c.display_jpeg()
        # 1. the coefficients against the vectorised numpy DCT and quantisation
        assert np.array_equal(c.jpeg_coefficients(), jm.coefficients(frame, quality, sub)), (quality, sub)
        # 2. the marker walk: the header's fields, every RSTn in sequence, EOI last, nothing else inside the scan
        info = jm.walk(stream)
        g = jm.geometry(w, h, sub, ri)
        assert (info["w"], info["h"], info["sub"], info["ri"]) == (w, h, sub, ri) and len(info["intervals"]) == g["intervals"]
        assert stream[:jm.HEADER_BYTES] == jm.header(w, h, quality, sub, ri)
        rec = c.jpeg_record()
        assert rec["bytes"] == len(stream) and rec["blocks"] == g["blocks"] and rec["overflow"] == 0
        assert sum(len(x) for x in info["intervals"]) + rec["stuffed_bytes"] + 2 * g["intervals"] + jm.HEADER_BYTES == len(stream)
        # 3. byte for byte the emulation's stream
        assert stream == emu.jpeg_image(frame), (quality, sub, ri)
        print("1920x1080 q%d %s Ri %d: %d bytes, %d stuffed" % (quality, sub, ri, len(stream), rec["stuffed_bytes"]))


def test_group_with_three_frames_in_flight(pkg, make_hip):
    scene = pkg.scenes.terrain(n=24, width=130, height_px=70)
    frames = 4
    one = make_hip()
    want = []
    for k in range(frames):
        if k == 0:
            _render(pkg, one, scene, 130, 70, spp=2)
        else:
            one.render_frame(scene.camera, pkg.CONVERGE)
        want.append(one.display_jpeg())
    assert len(set(want)) == frames
    g = pkg.render_group([0, 0], "peer")
    g.init(130, 70)
    scene.upload(g)
    for k, v in {"integrator": "pt", "spp": 2, "max_depth": 2}.items():
        g.set_setting(k, v)
    n = 3
    for k in range(frames):
        g.render_async(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
        g.present_jpeg_async(k % n)
        if k >= n - 1:
            assert g.present_jpeg_wait((k + 1) % n) == want[k - n + 1], k
    for k in range(frames - n + 1, frames):
        assert g.present_jpeg_wait(k % n) == want[k], k
    assert g.display_jpeg() == want[-1]
    with pytest.raises(RuntimeError, match="holds a JPEG stream"):
        g.present_display_wait(0)
    g.destroy()


def test_one_rank_comm_then_jpeg_on_the_callers_stream(pkg, make_hip):
    import torch
    w, h = 130, 70
    scene = pkg.scenes.cornell(w, h, geometric_emitter=True)
    ref = _render(pkg, make_hip(), scene, w, h)
    c = _render(pkg, make_hip(), scene, w, h)
    want = ref.display_jpeg()
    comm = pkg.RenderComm(c, None)
    full = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    out8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    cap = c.jpeg_bound()
    jpg = torch.full((cap + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    rec = torch.zeros((8,), dtype=torch.int32, device="cuda:0")
    comm.gather(full.data_ptr())
    comm.wait()
    stream = torch.cuda.current_stream().cuda_stream
    comm.display(full.data_ptr(), out8.data_ptr(), "rgba8", stream)
    comm.display_jpeg(out8.data_ptr(), jpg.data_ptr(), cap, rec.data_ptr(), stream)
    torch.cuda.synchronize()
    r = rec.cpu().numpy()
    assert r[0] == len(want) and r[5] == 0 and r[6] == jm.HEADER_BYTES
    host = jpg.cpu().numpy()
    assert bytes(host[:len(want)]) == want and (host[cap:] == 0xA5).all()
    # a capacity below the stream: the flag, the length, and nothing behind the header
    jpg.fill_(0xA5)
    comm.display_jpeg(out8.data_ptr(), jpg.data_ptr(), len(want) - 1, rec.data_ptr(), stream)
    torch.cuda.synchronize()
    r, host = rec.cpu().numpy(), jpg.cpu().numpy()
    assert r[0] == len(want) and r[5] == 1 and (host[jm.HEADER_BYTES:] == 0xA5).all()
    with pytest.raises(RuntimeError, match="does not hold the header"):
        comm.display_jpeg(out8.data_ptr(), jpg.data_ptr(), 100, rec.data_ptr(), stream)
    comm.destroy()


def test_feature_off_changes_nothing(pkg, make_hip):
    """display() before and after a JPEG call; the settings untouched, the record empty until the first stream."""
    c = _render(pkg, make_hip(), pkg.scenes.cornell(130, 70), 130, 70)
    assert c.get_setting("display_jpeg_bytes") == "0"
    before8, before32 = c.display("rgba8"), c.display("rgba32f")
    c.display_jpeg()
    assert np.array_equal(c.display("rgba8"), before8) and np.array_equal(c.display("rgba32f").view(np.uint32), before32.view(np.uint32))
