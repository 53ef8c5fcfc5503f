"""The sky's loaders on the HIP kernels (csrc/sky_load.h, kernel family 17): the checks of tests/test_sky_load.py through the same module
(tests/sky_load_checks.py), and the kernels against the emulation library byte for byte — the table's arithmetic is double add,
multiply and divide in a fixed shape, so the two must give the same tables and records."""
import numpy as np
import pytest

import sky_load_checks as ck
import sky_load_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip(make_hip):
    c = make_hip()
    yield c
    c.destroy()


@pytest.fixture
def emu(make_emu):
    c = make_emu()
    yield c
    c.destroy()


@pytest.mark.parametrize("shape", ck.SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_decode_is_the_model(hip, shape):
    ck.decode_matches_the_model(hip, *shape)


def test_write_hdr_round_trips(hip, pkg, tmp_path):
    ck.write_hdr_round_trips(hip, pkg, tmp_path)


def test_rendering_under_the_file_is_rendering_under_its_texels(make_hip, pkg):
    ck.render_under_the_file(make_hip, pkg)


def test_malformed_files_are_refused_before_any_launch(hip):
    """The host's walk refuses every malformed file (the same walk passed the sanitizers over the same files, test_sky_load.py): no
    kernel of family 17 runs for them, and the previous sky stays."""
    hip.set_setting("stage_timing", 1)
    ck.refused_with_the_previous_sky_in_place(hip, ck.malformed())
    hip.wait()
    assert hip.get_setting("sky_load_time").split()[9:11] == ["1", "1"]  # (the one good file the check begins with)


def test_a_group_decodes_a_replica_per_member(pkg):
    g = pkg.render_group([0, 0], transport="peer")
    data, want = ck.file_case(33, 5, "mixed")
    g.set_sky_hdr(data, flip=True)
    for c in g.contexts:
        assert np.array_equal(ck.bits(c.read_sky()), ck.bits(want[::-1]))
    with pytest.raises(RuntimeError, match="truncated"):
        g.set_sky_hdr(data[:len(data) - 33 * 4 * 2 - 40])
    for c in g.contexts:
        assert np.array_equal(ck.bits(c.read_sky()), ck.bits(want[::-1]))
    g.destroy()


@pytest.mark.parametrize("n", ck.TABLE_SIZES)
def test_the_table_over_given_weights_is_the_emulations(hip, emu, n):
    """Every weight vector at every size: the judging rules on the device's table, and its bytes and record against the emulation's."""
    got = ck.tables_of_size(hip, n)
    for kind, w in list(sm.weight_vectors(n).items()) + [("zero", np.zeros(n))]:
        table, rec = emu.sky_alias_from_weights(w)
        assert rec == got[kind][1], (kind, n, rec, got[kind][1])
        assert np.array_equal(table, got[kind][0]), (kind, n, "%d buckets differ" % int((table != got[kind][0]).sum()))


@pytest.mark.parametrize("size", ck.SKY_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_table_of_a_sky_is_the_emulations(make_hip, make_emu, pkg, size):
    (dt, drec), (ht, hrec) = ck.sky_tables(make_hip, pkg, *size)
    (et, erec), (eh, ehrec) = ck.sky_tables(make_emu, pkg, *size)
    assert drec == erec and np.array_equal(dt, et)
    assert hrec == ehrec and np.array_equal(ht, eh)  # (the host's table is host work on either library)


def test_histogram_and_pdf_with_the_device_table(make_hip, pkg):
    ck.histogram_and_pdf(make_hip, pkg, ck.random_sky(24, 12))


def test_an_hdr_sky_with_the_device_table_renders_the_hosts_image(make_hip, pkg):
    """One 256 x 128 HDR sky over a 96 x 64 sky-only terrain, sky_sampling=1: the image mean with sky_table=device against the mean with
    the host's table, z <= 4 (test_sky_sampling's bound) over 12 frames of 8 spp each; both tables are of the same decoded texels."""
    import test_sky_sampling as base
    data, want = ck.tame_file(pkg, 256, 128, "rle")
    scene = pkg.scenes.terrain(n=24, width=96, height_px=64, lights=False)
    scene.camera.clampValue = 1e9
    scene.wh = (96, 64)
    stacks = []
    for table in ("device", "host"):
        c = base._ctx(pkg, make_hip, scene, spp=8, max_depth=2)
        c.set_sky_hdr(data)
        c.update()
        c.set_setting("sky_sampling", 1)
        c.set_setting("sky_table", table)
        stacks.append(base._frames(pkg, c, scene, 12))
        t, rec = c.read_sky_table()
        assert len(t) == 256 * 128 and rec["flags"] == (sm.VALID | sm.DEVICE if table == "device" else sm.VALID)
        assert np.array_equal(ck.bits(c.read_sky()), ck.bits(want))
        c.destroy()
    z, ma, mb = ck.mean_z(stacks[0], stacks[1])
    assert abs(z) <= 4.0 and ma > 1e-3, (z, ma, mb)
    assert not np.array_equal(stacks[0], stacks[1])
