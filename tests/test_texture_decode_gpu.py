"""Image textures on the HIP kernels (csrc/texture_decode.h, kernel family 15): the checks of tests/test_texture_decode.py through the
same module (tests/texture_decode_checks.py), at the smallest shapes that can still go wrong, and one full-size image against the
emulation library, which the CPU tier holds to the model at the small sizes."""
import numpy as np
import pytest

import jpeg_model as jm
import texture_decode_checks as ck
import texture_decode_model as tm

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip(make_hip):
    c = make_hip()
    yield c
    c.destroy()


# 1 x 1; sizes that are no multiple of the MCU; chroma planes 1, 2 and 3 columns wide (4:2:0 at widths 2, 4 and 5); 130 x 70 at 4:4:4
# with Ri = 1: 153 intervals, two full waves and a ragged third; Ri larger than the image: one lane at work
CASES = [("noise", 1, 1, 90, "444", 1), ("noise", 1, 1, 90, "420", 8), ("smooth", 7, 5, 90, "420", 1), ("noise", 17, 9, 100, "444", 11),
         ("smooth", 2, 3, 90, "420", 1), ("noise", 4, 9, 90, "420", 8), ("smooth", 5, 4, 1, "420", 1), ("noise", 33, 17, 90, "420", 8),
         ("noise", 130, 70, 90, "444", 1), ("smooth", 67, 35, 100, "420", 65535)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-q%d-%s-ri%d" % c)
def test_the_kernels_are_the_model(hip, case):
    ck.jm_case_matches(hip, *case)
    if case[1:3] == (130, 70):
        assert hip.texture_record()["intervals"] == 153


def test_the_kernels_decode_the_golden_streams(hip):
    """Pillow's streams: grey, 4:2:2, optimised Huffman tables, and streams without DRI on both paths."""
    without_dri = 0
    for name, stream, _ in ck.golden_streams():
        ck.decode_matches_the_model(hip, stream, name)
        without_dri += not tm.decode_cached(stream)[2]["ri"]
    assert without_dri >= 8


@pytest.mark.parametrize("size", ck.MIP_SIZES, ids=lambda s: "%dx%d" % s)
def test_mips(hip, size):
    ck.mips_match(hip, *size)


def test_a_device_built_chain_is_what_the_sampler_walks(hip, pkg):
    ck.sampler_walks_the_chain(hip, pkg)


def test_modifiers(hip):
    ck.modifiers_match(hip, ck.jpeg_case("smooth", 17, 9, 90, "420", 8)[1])


def test_mixed_table_is_all_or_nothing(hip, pkg):
    """The corrupt middle streams here are the ones the host refuses before any launch."""
    bad = [s for _, s, _, scan in ck.malformed() if not scan]
    ck.mixed_table(hip, pkg, ck.jpeg_case("noise", 17, 9, 90, "420", 1)[1], bad)


def test_malformed_headers_are_refused_before_any_launch(hip):
    hip.set_setting("stage_timing", 1)
    for name, stream, code, scan in ck.malformed():
        if not scan:
            ck.refused_with_nothing_written(hip, name, stream, code)
    hip.init(8, 8)
    hip.wait()
    assert hip.get_kernel_time("texture_decode")[1] == 0


@pytest.mark.parametrize("name", ["a run past coefficient 63", "an interval cut short"])
def test_a_corrupt_scan_is_flagged_by_the_kernel(hip, name):
    """Two scan-level entries, once each, on the device path: the same work items passed the host sanitizers over the same streams
    (test_texture_decode.py, test_sanitized_stand_alone_program); every read is bounded by the interval, every index by 63."""
    (stream, code), = [(s, c) for n, s, c, _ in ck.malformed() if n == name]
    hip.set_setting("texture_entropy", "device")
    assert "corrupt" in ck.refused_with_nothing_written(hip, name, stream, code)
    assert hip.texture_record()["errors"] != 0 and hip.texture_record()["path"] == ck.PATH_DEVICE


def test_front_ends_load_images(make_hip, pkg, tmp_path):
    gltf, obj = ck.write_quad_files(tmp_path)
    for load, path in ((pkg.gltf.load_scene, gltf), (pkg.obj.load_scene, obj)):
        c = make_hip()
        ck.renders_red_over_blue(c, pkg, load(path, load_images=True)[0])
        c.destroy()


def test_full_size_texture(hip, make_emu):
    """1024 x 1024, encoded by the device's own encoder at Ri = 128 (4096 MCUs of 4:2:0: 32 intervals), decoded by the kernels: byte for byte the
    emulation library's decode; its mip chain is the vectorised model's."""
    img = jm.smooth(1024, 1024)
    hip.init(1024, 1024)
    for key, value in (("display_jpeg_quality", 90), ("display_jpeg_subsampling", "420"), ("display_jpeg_restart", 128)):
        hip.set_setting(key, value)
    stream = hip.jpeg_image(img)
    emu = make_emu()
    want = emu.decode_image(stream)
    got = hip.decode_image(stream)
    assert np.array_equal(got, want), "%d texels differ" % int((got != want).any(-1).sum())
    assert np.array_equal(hip.texture_coefficients(), emu.texture_coefficients())
    assert hip.texture_record() == dict(emu.texture_record()) and hip.texture_record()["intervals"] == 32
    hip.set_textures([{"kind": "jpeg", "data": stream, "flags": tm.FLIP_ROWS | tm.LINEARIZE_SRGB}])
    assert np.array_equal(hip.read_texture(0), tm.chain(tm.modify(want, tm.FLIP_ROWS | tm.LINEARIZE_SRGB)))
    emu.destroy()


def test_a_group_decodes_a_replica_per_member(pkg):
    g = pkg.render_group([0, 0, 0], transport="peer")
    stream, px = ck.jpeg_case("noise", 33, 17, 90, "420", 1)[1], ck.noise_rgba(9, 7)
    g.set_textures([{"kind": "jpeg", "data": stream, "flags": 0}, {"kind": "rgba8", "data": px, "flags": tm.FLIP_ROWS}])
    want = [tm.chain(tm.decode_cached(stream)[0]), tm.chain(tm.modify(px, tm.FLIP_ROWS))]
    for c in g.contexts:
        for i in range(2):
            assert np.array_equal(c.read_texture(i), want[i]), i
    with pytest.raises(RuntimeError, match="texture 0"):
        g.set_textures([{"kind": "jpeg", "data": stream[:100], "flags": 0}])
    for c in g.contexts:
        assert np.array_equal(c.read_texture(1), want[1])
    g.destroy()
