"""The sky's loaders on the CPU tier (include/rfwhip.h, rfwhip_set_sky_hdr and sky_table=device; csrc/sky_load.h): the host emulation
of the work items is held to the numpy model of tests/sky_load_model.py — Radiance files bit for bit, alias tables by judging rules
whose bounds are counted from the number formats and the sums' shapes — and the header walk and the work items to the host sanitizers
in a stand-alone program.  The HIP kernels run the same checks in test_sky_load_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sky_load_checks as ck
import sky_load_model as sm
from conftest import ROOT


@pytest.fixture
def emu(make_emu):
    c = make_emu()
    yield c
    c.destroy()


# ---- 1. Radiance files -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ck.SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_decode_is_the_model(emu, shape):
    ck.decode_matches_the_model(emu, *shape)


def test_the_model_encoder_splits_runs_and_mixes_forms():
    """The files hold what they are meant to hold: a run of 129 as 127 + 2, literals beside runs, flat scanlines in a mixed file."""
    assert sm.rle_plane([77] * 129) == bytes((128 + 127, 77, 128 + 2, 77))
    assert sm.rle_plane([1, 2, 3, 3, 3, 4]) == bytes((2, 1, 2, 128 + 3, 3, 1, 4))
    assert sm.rle_plane(list(range(130))) == bytes([128] + list(range(128)) + [2, 128, 129])
    data, _ = ck.file_case(130, 5, "rle")
    assert bytes((128 + 127, 77, 128 + 2, 77)) in data
    rle, flat, mixed = (len(ck.file_case(33, 5, m)[0]) for m in ck.MODES)
    assert mixed != rle and mixed != flat  # (a mixed file holds both forms)
    assert len(ck.file_case(7, 5, "rle")[0]) == len(ck.file_case(7, 5, "flat")[0])  # width 7 is flat whatever was asked


def test_hdr_info(pkg, emu_lib):
    for (w, h) in ck.SHAPES:
        for mode in ck.MODES:
            info = pkg.images.hdr_info(ck.file_case(w, h, mode)[0], emu_lib)
            assert (info["width"], info["height"], info["supported"], info["reason"]) == (w, h, True, ""), info
            assert info["rle"] == (w >= 8 and mode != "flat"), (w, h, mode, info)
            assert info["exposure"] == 1.0
    data = sm.encode(sm.sample_rgbe(8, 1), extra=b"EXPOSURE=2.5\nEXPOSURE=2\n")
    assert pkg.images.hdr_info(data, emu_lib)["exposure"] == 5.0
    for name, bad, code, words in ck.malformed():
        if code == ck.UNSUPPORTED:
            info = pkg.images.hdr_info(bad, emu_lib)
            assert not info["supported"] and all(w in info["reason"] for w in words), (name, info)
            assert info["width"] in (8, 33) and info["height"] in (2, 5), (name, info)
        else:
            with pytest.raises(RuntimeError, match="rfwhip_hdr_info"):
                pkg.images.hdr_info(bad, emu_lib)


def test_write_hdr_round_trips(emu, pkg, tmp_path):
    ck.write_hdr_round_trips(emu, pkg, tmp_path)


def test_rendering_under_the_file_is_rendering_under_its_texels(make_emu, pkg):
    ck.render_under_the_file(make_emu, pkg)


def test_malformed_files_are_refused(emu):
    cases = ck.malformed()
    assert len(cases) >= 20
    ck.refused_with_the_previous_sky_in_place(emu, cases)


def test_a_group_decodes_a_replica_per_member(pkg, emu_lib):
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0, 0], "peer")
    data, want = ck.file_case(33, 5, "mixed")
    g.set_sky_hdr(data, flip=True)
    for c in g.contexts:
        assert np.array_equal(ck.bits(c.read_sky()), ck.bits(want[::-1]))
    with pytest.raises(RuntimeError, match="truncated"):
        g.set_sky_hdr(data[:len(data) - 33 * 4 * 2 - 40])
    for c in g.contexts:
        assert np.array_equal(ck.bits(c.read_sky()), ck.bits(want[::-1]))
    g.destroy()


# ---- 2. the table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ck.TABLE_SIZES)
def test_the_table_over_given_weights(emu, n):
    ck.tables_of_size(emu, n)


def test_degenerate_weights(emu):
    """A single weight keeps itself; an infinite sum is no table; equal weights may all be heavy or all light, and keep themselves."""
    table, rec = emu.sky_alias_from_weights([3.0])
    assert rec["flags"] == sm.VALID | sm.DEVICE and rec["S"] == 3.0 and table["keep"][0] == 1.0 and table["alias"][0] == 0
    _, rec = emu.sky_alias_from_weights([1.0, np.inf, 2.0])
    assert not rec["flags"] & sm.VALID
    table, rec = emu.sky_alias_from_weights(np.full(777, 0.1))
    assert (table["keep"] == 1.0).all() and (table["alias"] == np.arange(777)).all()
    with pytest.raises(RuntimeError, match="null argument or no weights"):
        emu.sky_alias_from_weights([])


@pytest.mark.parametrize("size", ck.SKY_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_table_of_a_sky_and_the_host_control(make_emu, pkg, size):
    """The device's table and — the control — the host's Vose table of the same sky under the same rules and the same bound."""
    (dt, _), (ht, _) = ck.sky_tables(make_emu, pkg, *size)
    assert not np.array_equal(dt, ht)  # (the same distribution, other buckets)


def test_histogram_and_pdf_with_the_device_table(make_emu, pkg):
    ck.histogram_and_pdf(make_emu, pkg, ck.random_sky(24, 12))


def test_settings_and_rebuilds(make_emu, pkg):
    sky = ck.random_sky(24, 12)
    c, scene = ck.sky_context(make_emu, pkg, sky, None)
    assert c.get_setting("sky_table") == "host" and "sky_table" not in c.get_settings() and "sky_load_time" not in c.get_settings()
    with pytest.raises(RuntimeError, match="sky_table must be host or device"):
        c.set_setting("sky_table", "gpu")
    with pytest.raises(RuntimeError):
        c.set_setting("sky_load_time", "1")
    # the default is the host's table, and naming it changes nothing: the bytes and the image
    default_table, rec = c.read_sky_table()
    assert rec["flags"] == sm.VALID and len(default_table) == 24 * 12
    c.set_setting("spp", 2)
    c.render_frame(scene.camera, pkg.RESET)
    default_img = c.framebuffer()
    c.set_setting("sky_table", "host")
    t, _ = c.read_sky_table()
    c.render_frame(scene.camera, pkg.RESET)
    assert np.array_equal(t, default_table) and np.array_equal(c.framebuffer(), default_img)
    # switching rebuilds, there and back
    c.set_setting("stage_timing", 1)
    c.set_setting("sky_table", "device")
    dev_table, rec = c.read_sky_table()
    assert rec["flags"] == sm.VALID | sm.DEVICE and not np.array_equal(dev_table, default_table)
    c.render_frame(scene.camera, pkg.RESET)
    assert np.isfinite(c.framebuffer()).all() and not np.array_equal(c.framebuffer(), default_img)
    assert c.get_kernel_time("sky_load")[1] == 7 and c.get_setting("sky_load_time").split()[9:] == ["0", "0"] + ["1"] * 7
    c.read_sky_table()  # (nothing changed: no rebuild)
    c.wait()
    assert c.get_kernel_time("sky_load", reset=True)[1] == 7 and c.get_kernel_time("sky_load")[1] == 0
    # a new sky rebuilds on the device; an HDR decode of RLE scanlines is two launches, of flat ones one
    c.set_sky_hdr(ck.tame_file(pkg, 16, 8, "rle")[0])
    c.update()
    c.wait()
    assert c.get_setting("sky_load_time").split()[9:] == ["1"] * 9 and len(c.read_sky_table()[0]) == 16 * 8
    c.get_kernel_time("sky_load", reset=True)
    c.set_sky_hdr(ck.tame_file(pkg, 16, 8, "flat")[0])
    c.wait()
    assert c.get_setting("sky_load_time").split()[9:11] == ["0", "1"]
    c.set_setting("sky_table", "host")
    t, rec = c.read_sky_table()
    assert rec["flags"] == sm.VALID and len(t) == 16 * 8
    # a black sky is no table on either path
    for table in ("device", "host"):
        c.set_setting("sky_table", table)
        c.set_sky(np.zeros((8 * 4, 3), np.float32), 8, 4)
        c.update()
        t, rec = c.read_sky_table()
        assert len(t) == 0 and not rec["flags"] & sm.VALID and c.get_setting("sky") == "0"
    c.set_setting("sky_sampling", 0)
    with pytest.raises(RuntimeError, match="sky_sampling is off"):
        c.read_sky_table()
    c.destroy()


def test_unbiased_against_the_default_with_the_device_table(make_emu, pkg):
    """test_sky_sampling's rule for the host's table, for the device's: tile means of sky_sampling=1 with sky_table=device agree with
    those of sky_sampling=0 within z <= 4 on the sky-only terrain."""
    import test_sky_sampling as base
    scene = base._terrain(pkg, lights=False)
    frames = 24
    fa = base._frames(pkg, base._ctx(pkg, make_emu, scene, spp=8, max_depth=1), scene, frames)
    fb = base._frames(pkg, base._ctx(pkg, make_emu, scene, spp=8, max_depth=1, sky_sampling=1, sky_table="device"), scene, frames)
    z, ma, mb = base._tile_z(fa, fb)
    assert np.abs(z).max() <= 4.0, np.abs(z).max()
    assert ma.mean() > 0.1 and not np.array_equal(fa, fb)


def test_group_of_emulated_contexts_equals_the_single_context(pkg, make_emu, emu_lib):
    scene = pkg.scenes.terrain(n=24, width=70, height_px=51)
    settings = {"integrator": "pt", "spp": 4, "max_depth": 2, "sky_sampling": 1, "sky_table": "device"}

    def run(target):
        target.init(70, 51)
        scene.upload(target)
        for k, v in settings.items():
            target.set_setting(k, v)
        for f in range(2):
            target.render_async(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
        target.wait()
        return target.framebuffer()

    ref = run(make_emu())
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0, 0], "peer")
    img = run(g)
    for c in g.contexts:
        assert c.read_sky_table()[1]["flags"] == sm.VALID | sm.DEVICE
    g.destroy()
    assert np.array_equal(img, ref)
    settings["sky_table"] = "host"
    assert not np.array_equal(run(make_emu()), ref)  # ... and the device's table was in use: the host's gives another image


# ---- 3. the sanitizers ---------------------------------------------------------------------------------------------------------
def test_sanitized_stand_alone_program(tmp_path):
    """The header walk and the work items over exactly-sized heap arrays under AddressSanitizer and UBSan, in a child process."""
    gxx = shutil.which("g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if not gxx or subprocess.run([gxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ or its sanitizer runtime is not installed here")
    exe = tmp_path / "skyhdr_san"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g"] + flags + ["-I" + os.path.join(ROOT, "rendering-fw_amd", "csrc"),
                        os.path.join(ROOT, "tests", "skyhdr_san_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files, expect = [], []
    for k, (name, bad, code, _) in enumerate(ck.malformed()):
        files.append(tmp_path / ("bad%02d.hdr" % k))
        files[-1].write_bytes(bad)
        expect.append((name, code))
    for (w, h) in ck.SHAPES:
        for mode in ck.MODES:
            files.append(tmp_path / ("good_%d_%d_%s.hdr" % (w, h, mode)))
            files[-1].write_bytes(ck.file_case(w, h, mode)[0])
            expect.append(((w, h, mode), 0))
    r = subprocess.run([str(exe)] + [str(f) for f in files], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files) + 1 and lines[-1].startswith("tables ok")
    for line, (name, code) in zip(lines, expect):
        assert int(line.split()[1]) == code and int(line.split()[2]) == 0, (name, line)
