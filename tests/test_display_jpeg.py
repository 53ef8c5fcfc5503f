"""Baseline JPEG of the display image (include/rfwhip.h, rfwhip_read_display_jpeg; csrc/display_jpeg.h), CPU tier: the host-emulation
build runs the work items of the HIP kernels.  The stream is defined in integers, so the emulation is held to the numpy model of
tests/jpeg_model.py byte for byte; the model is held to Pillow — its streams decode there, its own decoder agrees with Pillow's, and
its quality is within 0.5 dB of Pillow's own encoder."""
import io

import numpy as np
import pytest
from PIL import Image  # (a requirement of this tier: the model's streams are only as good as an independent decoder says)

import display_jpeg_checks as ck
import jpeg_model as jm

# |model decoder - Pillow's decoder| per channel value, the largest seen on the streams below: Pillow's decoder is libjpeg's, whose
# integer inverse DCT is within 1 of the exact one per sample, the same again in the fixed-point colour conversion, and a chroma
# sample off by one moves blue by 1.772 and red by 1.402
DECODER_AGREEMENT = 3
# our PSNR may lie this far below that of Pillow's encoder (another DCT, another downsampler): DESIGN.md section 21
PSNR_MARGIN_DB = 0.5


def _pillow(stream):
    return np.array(Image.open(io.BytesIO(stream)).convert("RGB"))


def test_the_model_shows_what_the_cases_are_for():
    """Preconditions, by the model alone, before any code under test runs: every property a case stands for occurs in its stream."""
    facts = lambda *a: ck.model(*a)[2]  # noqa: E731
    assert facts("noise", 130, 70, 100, "444", 8)["stuffed"] >= 100
    for sub in jm.SUBS:
        assert facts("black_white", 130, 70, 100, sub, 8)["dc_category"] == 11
        assert facts("cosine", 67, 35, 90, sub, 8)["zrl"] >= 100
    assert facts("checker", 130, 70, 100, "444", 8)["ac_category"] == 10
    assert facts("cosine", 67, 35, 90, "444", 8)["eob_free"] >= 40  # blocks whose coefficient 63 is non-zero: no EOB
    f = facts("smooth", 67, 35, 90, "444", 1)
    assert f["intervals"] == 45 and f["intervals"] > 5 * 8  # the marker number wraps more than five times
    f = facts("smooth", 67, 35, 90, "420", 11)
    assert f["mcus"] == 15 and f["intervals"] == 2  # 11 + 4: a short last interval
    assert facts("smooth", 130, 70, 90, "420", 11)["interval_blocks"] == 66  # more than one chunk of 64 blocks
    f = facts("noise", 130, 70, 90, "444", 65535)
    assert f["intervals"] == 1 and f["interval_blocks"] == 459
    f = facts("worst_case", 130, 70, 100, "444", 65535)
    assert f["block_bits"] >= 960  # (58 % of the 1658 bits a slot allows per block; jm.worst_case says why no image gets near 100 %)
    stream = ck.model("noise", 130, 70, 90, "444", 65535)[1]
    assert stream.count(b"\xff\xd0") == 0 and jm.walk(stream)["markers"] == []


@pytest.mark.parametrize("size", jm.SIZES, ids=lambda s: "%dx%d" % s)
def test_stream_matches_the_model(make_emu, size):
    w, h = size
    c = make_emu()
    c.init(w, h)
    for name, quality, sub, ri in ck.matrix(w, h):
        ck.stream_matches_the_model(c, name, w, h, quality, sub, ri)


SPECIAL = [("black_white", 130, 70, 100, "444", 8), ("black_white", 130, 70, 100, "420", 1), ("checker", 130, 70, 100, "444", 8),
           ("cosine", 67, 35, 90, "444", 8), ("cosine", 67, 35, 90, "420", 11), ("noise", 130, 70, 100, "444", 8),
           ("worst_case", 130, 70, 100, "444", 65535), ("worst_case", 130, 70, 100, "420", 11), ("smooth", 130, 70, 90, "420", 11)]


@pytest.mark.parametrize("case", SPECIAL, ids=lambda s: "-".join(str(x) for x in s))
def test_special_inputs_match_the_model(make_emu, case):
    c = make_emu()
    c.init(case[1], case[2])
    ck.stream_matches_the_model(c, *case)


def test_cap_one_byte_short(make_emu):
    c = make_emu()
    c.init(67, 35)
    ck.cap_one_byte_short_is_refused(c, "noise", 67, 35, 90, "420", 8)
    ck.cap_one_byte_short_is_refused(c, "smooth", 67, 35, 25, "444", 1)


PILLOW_CASES = [(name, w, h, q, sub, ri) for (name, w, h) in (("q_noise130x70", 130, 70), ("q_smooth130x70", 130, 70), ("q_smooth67x35", 67, 35),
                                                               ("q_one", 1, 1), ("q_7x5", 7, 5), ("q_bw", 72, 40))
                for q in (25, 90, 100) for sub in jm.SUBS for ri in (1, 8)]


def test_model_streams_decode_in_pillow_and_the_decoders_agree():
    worst = 0
    for case in PILLOW_CASES + SPECIAL:
        stream = ck.model(*case)[1]
        theirs, ours = _pillow(stream), jm.decode(stream)
        assert theirs.shape == ours.shape == (case[2], case[1], 3), case
        d = int(np.abs(theirs.astype(int) - ours.astype(int)).max())
        worst = max(worst, d)
        assert d <= DECODER_AGREEMENT, (case, d)
        assert np.array_equal(jm.decode_coefficients(jm.walk(stream)), ck.model(*case)[3]), case  # the model's own round trip
    print("largest |model decoder - Pillow| = %d" % worst)


def test_quality_is_pillows():
    """On the model's streams (byte identity carries it to the device): PSNR against the input, both streams decoded by Pillow, is at
    most PSNR_MARGIN_DB below that of Pillow's own encoder at the same quality and subsampling, on the six images the margin was
    specified on (jm.quality_image).  Measured: between -0.08 and +0.17 dB on every image of more than 35 pixels.  On the 7 x 5 image
    at quality 100 the error is the rounding of 105 samples and the difference is that sample's: +1.50 dB ("444") and -0.17 dB ("420")
    on this image, -0.97 dB ("444") on another draw of the same recipe (jm.smooth(7, 5)) — DESIGN.md section 21."""
    worst, sizes = 99.0, []
    for name, w, h, q, sub, ri in PILLOW_CASES:
        if ri != 8:
            continue
        img, stream = ck.model(name, w, h, q, sub, ri)[:2]
        rgb = img[..., :3]
        b = io.BytesIO()
        Image.fromarray(rgb).save(b, "JPEG", quality=q, subsampling=0 if sub == "444" else 2, optimize=False)
        ours, theirs = jm.psnr(_pillow(stream), rgb), jm.psnr(_pillow(b.getvalue()), rgb)
        print("%-12s %3dx%-3d q%-3d %s  ours %6.2f dB %6d B   Pillow %6.2f dB %6d B" % (name, w, h, q, sub, ours, len(stream), theirs, len(b.getvalue())))
        worst = min(worst, ours - theirs)
        if len(stream) > 1024:
            sizes.append(len(stream) / len(b.getvalue()) - 1.0)
        assert ours >= theirs - PSNR_MARGIN_DB, (name, w, h, q, sub, ours, theirs)
    print("worst ours - Pillow's = %.2f dB; sizes above 1 KB %+.1f %% .. %+.1f %%" % (worst, 100 * min(sizes), 100 * max(sizes)))


def _render(pkg, c, scene, w, h):
    c.init(w, h)
    scene.upload(c)
    for k, v in (("integrator", "pt"), ("spp", 4), ("max_depth", 2)):
        c.set_setting(k, v)
    c.render_frame(scene.camera, pkg.RESET)


def test_render_path(pkg, make_emu, tmp_path):
    """The Cornell frame: display_jpeg() is the model's stream of display() of the same frame, decodes to that frame, and
    display() is the same bytes before and after."""
    w, h = 70, 51
    c = make_emu()
    _render(pkg, c, pkg.scenes.cornell(w, h), w, h)
    before = c.display("rgba8")
    stream = c.display_jpeg()
    assert stream == jm.encode(before, 90, "420", 8)[0]
    assert np.array_equal(c.display("rgba8"), before)
    decoded = _pillow(stream)
    # (a stream of another frame, or with two channels exchanged, scores below 15 dB on this image; quality 90 scores above 30)
    assert jm.psnr(decoded, before[..., :3]) > 30.0, jm.psnr(decoded, before[..., :3])
    path = str(tmp_path / "frame.jpg")
    assert c.save_jpeg(path) == len(stream) and open(path, "rb").read() == stream
    assert Image.open(path).size == (w, h)
    assert c.get_setting("display_jpeg_bytes") == str(len(stream))


@pytest.mark.parametrize("n", [2, 3])
def test_group_equals_the_single_context(pkg, make_emu, emu_lib, n):
    w, h = 70, 51
    scene = pkg.scenes.terrain(n=24, width=w, height_px=h)
    one = make_emu()
    _render(pkg, one, scene, w, h)
    want = one.display_jpeg()
    want8 = one.display("rgba8")
    grp = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0] * n, "peer")
    _render(pkg, grp, scene, w, h)
    assert grp.display_jpeg() == want
    grp.present_jpeg_async(0)
    grp.present_display_async(1, "rgba8")
    grp.present_async(2)
    assert grp.present_jpeg_wait(0) == want
    assert np.array_equal(grp.present_display_wait(1), want8)
    # a slot remembers which of the three kinds it holds
    for slot, calls in ((0, (grp.present_wait, grp.present_display_wait)), (1, (grp.present_wait, grp.present_jpeg_wait)),
                        (2, (grp.present_display_wait, grp.present_jpeg_wait))):
        for call in calls:
            with pytest.raises(RuntimeError, match="slot %d holds" % slot):
                call(slot)
    with pytest.raises(RuntimeError, match="nothing was presented"):
        grp.present_jpeg_wait(3)
    with pytest.raises(RuntimeError, match="%d bytes" % len(want)):
        grp.present_jpeg_wait(0, cap=len(want) - 1)
    assert grp.present_jpeg_wait(0, cap=len(want)) == want  # (the slot stays presented)
    # the root's settings are the group's
    grp.set_setting("display_jpeg_quality", 25)
    one.set_setting("display_jpeg_quality", 25)
    assert grp.display_jpeg() == one.display_jpeg()
    grp.destroy()


def test_settings_and_errors(make_emu):
    c = make_emu()
    defaults = {"display_jpeg_quality": "90", "display_jpeg_subsampling": "420", "display_jpeg_restart": "8", "display_jpeg_bytes": "0"}
    for k, v in defaults.items():
        assert c.get_setting(k) == v, k
    for key, bad in (("display_jpeg_quality", "0"), ("display_jpeg_quality", "101"), ("display_jpeg_quality", "-1"), ("display_jpeg_quality", ""),
                     ("display_jpeg_quality", "90.5"), ("display_jpeg_quality", "high"), ("display_jpeg_subsampling", "422"),
                     ("display_jpeg_subsampling", ""), ("display_jpeg_subsampling", "4:2:0"), ("display_jpeg_restart", "0"),
                     ("display_jpeg_restart", "65536"), ("display_jpeg_restart", "8 "), ("display_jpeg_restart", "x")):
        with pytest.raises(RuntimeError) as e:
            c.set_setting(key, bad)
        assert key + " must" in str(e.value), (key, bad, str(e.value))
        assert c.get_setting(key) == defaults[key], (key, bad)
    for key in ("display_jpeg_bytes", "display_jpeg_time"):
        with pytest.raises(RuntimeError):
            c.set_setting(key, "1")
    for key, good in (("display_jpeg_quality", "1"), ("display_jpeg_quality", "100"), ("display_jpeg_subsampling", "444"),
                      ("display_jpeg_restart", "1"), ("display_jpeg_restart", "65535")):
        c.set_setting(key, good)
        assert c.get_setting(key) == good
    assert not any(k.startswith("display") for k in c.get_settings())
    # state: everything needs a render target
    for call in (c.jpeg_bound, c.display_jpeg, c.jpeg_coefficients, c.jpeg_record, lambda: c.jpeg_image(np.zeros((0, 0, 4), np.uint8))):
        with pytest.raises((RuntimeError, ValueError)):
            call()
    c.init(9, 9)
    with pytest.raises(RuntimeError, match="nothing has been encoded"):
        c.jpeg_coefficients()
    with pytest.raises(RuntimeError, match="no stream"):
        c.jpeg_record()
    # stage_timing: the four kernels are family 14, one count each
    c.set_setting("stage_timing", 1)
    c.jpeg_image(jm.noise(9, 9))
    c.wait()
    assert c.get_kernel_time("jpeg")[1] == 4 and c.get_setting("display_jpeg_time").split()[4:] == ["1"] * 4
    assert c.get_kernel_time("jpeg", reset=True)[1] == 4 and c.get_kernel_time("jpeg")[1] == 0
    assert c.get_setting("display_jpeg_time").split()[4:] == ["0"] * 4
