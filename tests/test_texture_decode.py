"""Image textures on the CPU tier (include/rfwhip.h, rfwhip_set_texture_sources; csrc/texture_decode.h): the numpy model is held to
Pillow's stored decodes byte for byte, the host emulation of the work items to the model — on both entropy paths — and the parser and
the work items to the host sanitizers in a stand-alone program.  The HIP kernels run the same checks in test_texture_decode_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_model as jm
import texture_decode_checks as ck
import texture_decode_model as tm
from conftest import ROOT


@pytest.fixture
def emu(make_emu):
    c = make_emu()
    yield c
    c.destroy()


# ---- 1. the model is Pillow ------------------------------------------------------------------------------------------------
def test_the_model_is_pillow():
    streams = ck.golden_streams()
    assert len(streams) >= 24
    seen = set()
    for name, stream, want in streams:
        got, _, info = tm.decode_cached(stream)
        assert np.array_equal(got[..., :3], want), (name, "the model differs from Pillow's decode by up to %d"
                                                   % int(np.abs(got[..., :3].astype(int) - want).max()))
        assert (got[..., 3] == 255).all()
        seen.add((info["ncomp"], info["hs"], info["vs"], bool(info["ri"])))
    # the file holds what it is meant to hold: grey, 4:4:4, 4:2:2 and 4:2:0, each with and without restart intervals
    assert seen == {(n, hs, vs, r) for (n, hs, vs) in ((1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)) for r in (False, True)}, seen
    for name in ("unsupported_progressive", "unsupported_440"):
        with pytest.raises(tm.Unsupported):
            tm.decode(ck.golden()[name].tobytes())


def test_the_png_reader_is_pillow(pkg, emu_lib):
    g = ck.golden()
    names = [k[4:] for k in g if k.startswith("png_") and k != "png_interlaced"]
    assert len(names) == 5
    for n in names:
        assert np.array_equal(pkg.images.decode_png(g["png_" + n].tobytes(), emu_lib), g["rgba_" + n]), n
    with pytest.raises(ValueError, match="interlaced"):
        pkg.images.decode_png(g["png_interlaced"].tobytes(), emu_lib)
    with pytest.raises(ValueError, match="signature"):
        pkg.images.decode_png(b"\xff\xd8 not a png", emu_lib)
    # a file of None / Sub / Up rows alone stays in numpy; its pixels are those of the per-byte helper
    px = ck.noise_rgba(9, 6)
    assert np.array_equal(pkg.images.decode_png(ck.png_bytes(px), emu_lib), px)


# ---- 2. the library is the model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", jm.SIZES + [(33, 17), (5, 4), (4, 9), (2, 3)], ids=lambda s: "%dx%d" % s)
def test_the_library_is_the_model(emu, size):
    for name, w, h, quality, sub, ri in ck.matrix():
        if (w, h) == size:
            ck.jm_case_matches(emu, name, w, h, quality, sub, ri)


def test_the_library_decodes_the_golden_streams(emu, pkg, emu_lib):
    for name, stream, want in ck.golden_streams():
        ck.decode_matches_the_model(emu, stream, name)
        info = pkg.images.image_info(stream, emu_lib)
        w = tm.walk(stream)
        assert info["supported"] and (info["width"], info["height"], info["components"], info["h_sampling"], info["v_sampling"]) == \
            (w["w"], w["h"], w["ncomp"], w["hs"], w["vs"]), name
        assert info["restart_interval"] == w["ri"] and info["intervals"] == len(w["intervals"]), name
    for name, form in (("unsupported_progressive", "progressive"), ("unsupported_440", "sampling factors 1 x 2")):
        stream = ck.golden()[name].tobytes()
        info = pkg.images.image_info(stream, emu_lib)
        assert not info["supported"] and form in info["reason"] and (info["width"], info["height"]) == (33, 17), info
        assert form in ck.refused_with_nothing_written(emu, name, stream, ck.UNSUPPORTED)


# ---- 3. mips ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ck.MIP_SIZES, ids=lambda s: "%dx%d" % s)
def test_mips(emu, size):
    ck.mips_match(emu, *size)


def test_a_device_built_chain_is_what_the_sampler_walks(emu, pkg):
    ck.sampler_walks_the_chain(emu, pkg)


# ---- 4. modifiers ----------------------------------------------------------------------------------------------------------
def test_modifiers(emu):
    ck.modifiers_match(emu, ck.jpeg_case("smooth", 17, 9, 90, "420", 8)[1])
    with pytest.raises(RuntimeError, match="two linearisations"):
        emu.decode_image(ck.jpeg_case("smooth", 17, 9, 90, "420", 8)[1], tm.LINEARIZE_REFERENCE | tm.LINEARIZE_SRGB)


# ---- 5. a mixed table ------------------------------------------------------------------------------------------------------
def test_mixed_table_is_all_or_nothing(emu, pkg):
    bad = [s for _, s, _, _ in ck.malformed()]
    ck.mixed_table(emu, pkg, ck.jpeg_case("noise", 17, 9, 90, "420", 1)[1], bad)


def test_a_group_decodes_a_replica_per_member(pkg, emu_lib):
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0, 0, 0], "peer")
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


# ---- 6. malformed input ----------------------------------------------------------------------------------------------------
def test_malformed_streams_are_refused(emu):
    for mode in ("auto", "host", "device"):
        emu.set_setting("texture_entropy", mode)
        for name, stream, code, _ in ck.malformed():
            ck.refused_with_nothing_written(emu, name, stream, code)


def test_settings(emu):
    assert emu.get_setting("texture_entropy") == "auto"
    with pytest.raises(RuntimeError, match="texture_entropy must"):
        emu.set_setting("texture_entropy", "gpu")
    with pytest.raises(RuntimeError):
        emu.set_setting("texture_decode_time", "1")
    assert "texture_entropy" not in emu.get_settings() and "texture_decode_time" not in emu.get_settings()
    with pytest.raises(RuntimeError, match="nothing has been decoded"):
        emu.texture_coefficients()
    # stage_timing: a decode on the device path is six launches of family 15, on the host path four
    emu.init(8, 8)
    emu.set_setting("stage_timing", 1)
    stream = ck.jpeg_case("noise", 17, 9, 90, "420", 1)[1]
    emu.set_textures([{"kind": "jpeg", "data": stream, "flags": 0}])
    emu.wait()
    assert emu.get_kernel_time("texture_decode")[1] == 6 and emu.get_setting("texture_decode_time").split()[6:] == ["1"] * 6
    assert emu.get_kernel_time("texture_decode", reset=True)[1] == 6 and emu.get_kernel_time("texture_decode")[1] == 0
    emu.set_setting("texture_entropy", "host")
    emu.decode_image(stream)
    emu.wait()
    assert emu.get_setting("texture_decode_time").split()[6:] == ["0", "0", "1", "1", "0", "1"]


def test_sanitized_stand_alone_program(tmp_path):
    """The parser and the work items over exactly-sized heap arrays under AddressSanitizer and UBSan, in a child process."""
    gxx = shutil.which("g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if not gxx or subprocess.run([gxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ or its sanitizer runtime is not installed here")
    exe = tmp_path / "texdec_san"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g"] + flags + ["-I" + os.path.join(ROOT, "rendering-fw_amd", "csrc"),
                        os.path.join(ROOT, "tests", "texdec_san_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files, expect = [], []
    for k, (name, stream, code, scan) in enumerate(ck.malformed()):
        files.append(tmp_path / ("bad%02d.jpg" % k))
        files[-1].write_bytes(stream)
        expect.append((name, 0 if scan else code, scan))
    for k, (name, stream, _) in enumerate(ck.golden_streams()):
        files.append(tmp_path / ("good%02d.jpg" % k))
        files[-1].write_bytes(stream)
        expect.append((name, 0, False))
    r = subprocess.run([str(exe)] + [str(f) for f in files], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files)
    for line, (name, code, scan) in zip(lines, expect):
        got_code, errors = int(line.split()[1]), int(line.split()[2])
        assert got_code == code and (errors != 0) == scan, (name, line)


# ---- 7. the front ends -----------------------------------------------------------------------------------------------------
def test_front_ends_load_images(make_emu, pkg, tmp_path):
    gltf, obj = ck.write_quad_files(tmp_path)
    for load, path in ((pkg.gltf.load_scene, gltf), (pkg.obj.load_scene, obj)):
        plain, with_images = load(path)[0], load(path, load_images=True)[0]
        assert plain.textures == [] and plain.host_materials[0]["texture"] == -1  # the default: today's scene
        assert len(with_images.textures) == 1 and with_images.host_materials[0]["texture"] == 0
        assert plain.host_materials[0] == dict(with_images.host_materials[0], texture=-1, normalmap=-1)
        c = make_emu()
        ck.renders_red_over_blue(c, pkg, with_images)
        c.destroy()


# ---- 8. the reference's own asset (container only) ---------------------------------------------------------------------------
def test_cesium_man_texture(emu):
    path = "/root/reference/assets/models/CesiumMan/CesiumMan.jpg"
    if not os.path.exists(path):
        pytest.skip("reference checkout absent: the golden streams alone")
    Image = pytest.importorskip("PIL.Image")
    with open(path, "rb") as f:
        stream = f.read()
    want = np.asarray(Image.open(path).convert("RGB"))
    got = emu.decode_image(stream)
    assert got.shape == (1024, 1024, 4) and np.array_equal(got[..., :3], want)
    rec = emu.texture_record()
    assert rec["errors"] == 0 and rec["path"] == ck.PATH_DEVICE and rec["intervals"] == 128, rec
