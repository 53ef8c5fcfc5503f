"""What tests/test_sky_load.py (host emulation) and tests/test_sky_load_gpu.py (the HIP kernels) both ask of a context: a decoded
Radiance file equals the numpy model (tests/sky_load_model.py) bit for bit, a malformed file is refused with the previous sky in place,
and an alias table — built by the kernels or by the host — describes the weights' distribution within bounds counted from the number
formats and the sums' shapes.  The model's files and texels are computed once per process and shared."""
import ctypes as C

import numpy as np
import pytest

import sky_load_model as sm
import sky_sampling_model as ssm

INVALID, UNSUPPORTED = 1, 5  # RFWHIP_ERR_INVALID_ARGUMENT, RFWHIP_ERR_UNSUPPORTED
# widths 7 (below 8: flat whatever the mode), 8, 33, 130 (a run of 129 splits at 127); heights 1 and 5
SHAPES = [(w, h) for w in (7, 8, 33, 130) for h in (1, 5)]
MODES = ("rle", "flat", "mixed")
B = sm.B
TABLE_SIZES = [1, 2, B - 1, B, B + 1, 2 * B + 1, B * B + 1]  # B * B + 1: the first size with two super-blocks (k_skytab_scan_top chains)
SKY_SIZES = [(8, 4), (24, 12), (64, 32)]
_FILES = {}


def file_case(w, h, mode):
    """(the file's bytes, the model's texels H x W x 4 float32)."""
    key = (w, h, mode)
    if key not in _FILES:
        rgbe = sm.sample_rgbe(w, h)
        data = sm.encode(rgbe, mode)
        want = sm.decode(data)
        assert np.array_equal(want.view(np.uint32), sm.rgbe_to_float(rgbe).view(np.uint32)), key  # the model reads what it wrote
        _FILES[key] = (data, want)
    return _FILES[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def decode_matches_the_model(c, w, h):
    """Every mode of one shape, with and without the flip, through rfwhip_read_sky: bit-equal to the model."""
    for mode in MODES:
        data, want = file_case(w, h, mode)
        for flip in (False, True):
            c.set_sky_hdr(data, flip=flip)
            got = c.read_sky()
            assert got.shape == (h, w, 4), (w, h, mode, flip, got.shape)
            ref = want[::-1] if flip else want
            assert np.array_equal(bits(got), bits(ref)), (w, h, mode, flip, "%d texels differ" % int((bits(got) != bits(ref)).any(-1).sum()))
            assert np.array_equal(bits(sm.decode(data, flip)), bits(ref))
    # the special texels came through: exponent 0 is black, exponent 1 is subnormal, exponent 255 is 255 * 2^119
    data, want = file_case(w, h, "rle")
    flat = want.reshape(-1, 4)
    if w < 130:
        assert (flat[0] == 0).all() and (flat[1][:3] == 0).all()
        assert flat[2, 0] == np.float32(255.0 * 2.0 ** -135) and flat[2, 1] == np.float32(2.0 ** -135) and flat[3, 0] == np.float32(255.0 * 2.0 ** 119)


def write_hdr_round_trips(c, pkg, tmp_path):
    """write_hdr -> set_sky_hdr -> read_sky is exact for texels RGBE can hold (mantissa 2^(e - 136), at least 1e-32), RLE and flat."""
    rng = np.random.default_rng(5)
    for (w, h) in ((33, 5), (130, 3), (7, 2)):
        rgbe = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        rgbe[..., 3] = rng.integers(60, 200, (h, w))
        rgbe[0, 0] = 0
        rgbe[:, w // 2:w // 2 + 6, :] = rgbe[:, w // 2:w // 2 + 1, :]  # a run
        rgb = sm.rgbe_to_float(rgbe)
        for rle in (True, False):
            path = str(tmp_path / ("rt_%d_%d_%d.hdr" % (w, h, rle)))
            enc = pkg.images.rgbe_from_float(rgb[..., :3])
            ok = ~((enc[..., 0] == 1) & (enc[..., 1] == 1) & (enc[..., 2] == 1))  # (1 1 1 e would read as an old-style run in a flat file)
            rgb_ok = rgb * ok[..., None]
            pkg.images.write_hdr(path, rgb_ok, rle=rle)
            info = pkg.images.load_hdr(path, c)
            assert (info["width"], info["height"], info["supported"]) == (w, h, True) and info["rle"] == (rle and w >= 8), info
            got = c.read_sky()
            assert np.array_equal(bits(got), bits(rgb_ok)), (w, h, rle)


def tame_file(pkg, w=64, h=32, mode="mixed"):
    """A sky worth rendering under (the scenes' test sky, through RGBE) as (file, the model's texels)."""
    s = pkg.scenes.Scene()
    s.set_test_sky(w, h)
    rgbe = pkg.images.rgbe_from_float(np.asarray(s.sky[0], np.float32).reshape(h, w, 3))
    data = sm.encode(rgbe, mode)
    return data, sm.decode(data)


def render_under_the_file(make, pkg):
    """A 48 x 32 terrain under the file is bit-equal to the same terrain under set_sky of the model's texels."""
    data, want = tame_file(pkg)
    scene = pkg.scenes.terrain(n=24, width=48, height_px=32, lights=False)
    imgs = []
    for from_file in (True, False):
        c = make()
        c.init(48, 32)
        if not from_file:
            scene.sky = (want[..., :3].reshape(-1, 3).copy(), want.shape[1], want.shape[0])
        scene.upload(c)
        if from_file:
            c.set_sky_hdr(data)
            c.update()
        for k, v in (("integrator", "pt"), ("spp", 4), ("max_depth", 2)):
            c.set_setting(k, v)
        c.render_frame(scene.camera, pkg.RESET)
        imgs.append(c.framebuffer())
        c.destroy()
    assert imgs[0][..., :3].mean() > 1e-3
    assert np.array_equal(bits(imgs[0]), bits(imgs[1]))


# ---- malformed input -------------------------------------------------------------------------------------------------------
def _scan(w, planes):
    return bytes((2, 2, w >> 8, w & 255)) + b"".join(bytes(p) for p in planes)


def malformed():
    """[(name, file, the code it must be refused with, words its message must hold)], built by editing good 8- and 33-wide files."""
    good, _ = file_case(33, 5, "rle")
    flat, _ = file_case(33, 5, "flat")
    rgbe = sm.sample_rgbe(33, 5)
    start = good.index(b"\n\n") + 2
    start = good.index(b"\n", start) + 1  # the first scanline
    line0 = len(sm.rle_scanline(rgbe[0]))
    ok8 = [[136, 7]] * 4  # a run of 8 per component
    head8 = sm.header(8, 2)
    flat_start = flat.index(b"\n\n") + 2
    flat_start = flat.index(b"\n", flat_start) + 1
    old = bytearray(flat)
    old[flat_start + 33 * 4 + 8:flat_start + 33 * 4 + 12] = bytes((1, 1, 1, 5))  # scanline 1, column 2
    cases = [
        ("truncated inside the first line", good[:8], INVALID, ("truncated",)),
        ("truncated inside the header", good[:good.index(b"FORMAT") + 9], INVALID, ("truncated",)),
        ("truncated inside the resolution line", good[:good.index(b"\n\n") + 6], INVALID, ("truncated",)),
        ("truncated in front of scanline 0", good[:start + 2], INVALID, ("scanline 0", "truncated")),
        ("truncated behind a scanline header", good[:start + 4], INVALID, ("scanline 0", "truncated")),
        ("truncated inside a component", good[:start + line0 // 2], INVALID, ("scanline 0", "truncated")),
        ("truncated in front of scanline 1", good[:start + line0], INVALID, ("scanline 1", "truncated")),
        ("truncated behind a run's count byte", head8 + _scan(8, ok8) + _scan(8, [[136, 7], [136]]), INVALID, ("scanline 1", "truncated")),
        ("truncated inside a literal", head8 + _scan(8, ok8) + _scan(8, [[136, 7], [8, 1, 2, 3]]), INVALID, ("scanline 1", "truncated")),
        ("a flat scanline cut short", flat[:flat_start + 33 * 4 * 3 + 17], INVALID, ("scanline 3", "truncated")),
        ("count byte 0", head8 + _scan(8, ok8) + _scan(8, [[131, 9, 0, 133, 9]] + ok8[:3]), INVALID, ("scanline 1", "count byte of 0")),
        ("a run across the plane's end", head8 + _scan(8, ok8) + _scan(8, [[133, 9, 133, 9]] + ok8[:3]), INVALID, ("scanline 1", "run", "overruns")),
        ("a literal across the plane's end", head8 + _scan(8, [[136, 7], [5, 1, 2, 3, 4, 5, 5, 1, 2, 3, 4, 5]] + ok8[:2]) + _scan(8, ok8), INVALID,
         ("scanline 0", "literal", "overruns")),
        ("a wrong width in 2 2 hi lo", head8 + _scan(8, ok8) + bytes((2, 2, 0, 9)) + bytes([136, 7] * 4), INVALID, ("scanline 1", "width 9")),
        ("no blank line", sm.header(8, 2, blank=False) + _scan(8, ok8) * 2, INVALID, ("no blank line",)),
        ("no FORMAT line", b"#?RADIANCE\n\n-Y 2 +X 8\n" + _scan(8, ok8) * 2, INVALID, ("FORMAT",)),
        ("another magic", b"#?PICTURE" + good[10:], INVALID, ("magic",)),
        ("+Y orientation", sm.header(8, 2, res=b"+Y 2 +X 8") + _scan(8, ok8) * 2, UNSUPPORTED, ("orientation", "+Y")),
        ("X-major orientation", sm.header(8, 2, res=b"+X 8 -Y 2") + _scan(8, ok8) * 2, UNSUPPORTED, ("orientation", "+X")),
        ("the XYZE format", sm.header(8, 2, fmt="32-bit_rle_xyze") + _scan(8, ok8) * 2, UNSUPPORTED, ("xyze",)),
        ("an old-style run pixel", bytes(old), UNSUPPORTED, ("scanline 1", "old-style")),
    ]
    return cases


def refused_with_the_previous_sky_in_place(c, cases):
    """Every case from a buffer with guard bytes around it: the code, the message, the guards, and the sky of before."""
    data, want = file_case(33, 5, "mixed")
    c.set_sky_hdr(data)
    fn = c._fn("set_sky_hdr")
    for name, bad, code, words in cases:
        buf = np.full(len(bad) + 128, 0xA5, np.uint8)
        buf[64:64 + len(bad)] = np.frombuffer(bad, np.uint8)
        got = fn(c._ctx, buf.ctypes.data + 64, len(bad), 0)
        msg = c._fn("last_error")().decode()
        assert got == code, (name, got, msg)
        assert msg.startswith("rfwhip_set_sky_hdr: ") and all(w in msg for w in words), (name, msg)
        assert (buf[:64] == 0xA5).all() and (buf[64 + len(bad):] == 0xA5).all(), name
        sky = c.read_sky()
        assert sky.shape == (5, 33, 4) and np.array_equal(bits(sky), bits(want)), (name, "the previous sky is gone")
    with pytest.raises(RuntimeError, match="unknown flags"):
        c._check(fn(c._ctx, np.frombuffer(data, np.uint8).ctypes.data, len(data), 2))


# ---- the table ---------------------------------------------------------------------------------------------------------------
def table_from_weights(c, w, label):
    """rfwhip_sky_alias_from_weights over w: the record, and the table's judging rules -> (table, record)."""
    table, rec = c.sky_alias_from_weights(w)
    ws = sm.sanitised(w)
    sm.check_record(rec, ws, label)
    if rec["flags"] & sm.VALID:
        sm.check_table(table, ws, rec["S"], label)
    return table, rec


def tables_of_size(c, n):
    out = {}
    for kind, w in sm.weight_vectors(n).items():
        out[kind] = table_from_weights(c, w, (kind, n))
    table, rec = c.sky_alias_from_weights(np.zeros(n))
    assert not rec["flags"] & sm.VALID and rec["S"] == 0.0 and rec["heavy"] == 0, ("all zero", n, rec)
    out["zero"] = (table, rec)
    return out


def random_sky(w, h, seed=3):
    """As test_sky_sampling's: asymmetric, a bright texel, a negative and a NaN texel (weight 0), a black row."""
    rng = np.random.default_rng(seed + w)
    px = (rng.random((h, w, 3)) ** 4 * 5).astype(np.float32)
    px[:, : w // 3] *= 0.05
    px[h // 4, w // 8] = (20, 30, 10)
    px[h // 2, w // 3] = (-1, -1, -1)
    px[h // 2, w // 2] = (np.nan, 1, 1)
    px[h - 1] = 0
    return px.reshape(-1, 3), w, h


def sky_context(make, pkg, sky, table, **settings):
    """A context with a small scene under `sky`, sky_sampling = 1 and sky_table = `table` (None: never set)."""
    import test_sky_sampling as base
    scene = base._open_scene(pkg)
    scene.sky = sky
    extra = dict(settings)
    if table is not None:
        extra["sky_table"] = table
    return base._ctx(pkg, make, scene, sky_sampling=1, **extra), scene


def sky_tables(make, pkg, w, h):
    """The device's and the host's table of one real sky under the same judging rules (the host's is the control: the same bound must
    hold for skysamp::build_alias) -> ((table, record) of the device, (table, record) of the host)."""
    sky = random_sky(w, h)
    weights = sm.weights(sky[0], w, h)
    out = []
    for table in ("device", "host"):
        c, _ = sky_context(make, pkg, sky, table)
        t, rec = c.read_sky_table()
        # (numpy's cosines may differ from the library's in the last place: an error of 2^-52 relative in a weight, far inside the scan's term)
        assert abs(rec["S"] - weights.sum()) <= 1e-12 * rec["S"], (table, rec, weights.sum())
        if table == "device":
            assert rec["flags"] == sm.VALID | sm.DEVICE and rec["heaviest"] == int(np.argmax(weights)), rec
            assert rec["heavy"] == int((weights > rec["S"] / (w * h)).sum()) and rec["light"] == w * h - rec["heavy"], rec
        else:
            assert rec["flags"] == sm.VALID, rec
        sm.check_table(t, weights, rec["S"], (table, w, h), device=table == "device")
        out.append((t, rec))
        c.destroy()
    return out


def histogram_and_pdf(make, pkg, sky, draws=400_000):
    """Through k_kat's sky cases with sky_table = device: the histogram of drawn texels against P_t (chi-square as test_sky_sampling's),
    no texel of weight 0 drawn, and the pdf integrating to one over the texels' solid angles."""
    px, w, h = sky
    c, _ = sky_context(make, pkg, sky, "device")
    assert c.get_setting("sky_table") == "device" and c.get_setting("sky") == "1"
    rng = np.random.default_rng(11)
    rec = np.zeros((draws, 24), np.float32)
    rec[:, :5] = rng.random((draws, 5), np.float32)
    out = c.kat("sky_sample", rec)
    texel = out[:, 7].view(np.uint32).astype(np.int64)
    assert c.read_sky_table()[1]["flags"] == sm.VALID | sm.DEVICE
    P, lum, S = ssm.distribution(px, w, h)
    P = P.reshape(-1)
    counts = np.bincount(texel, minlength=w * h)
    assert counts[P == 0].sum() == 0, "a texel of weight 0 was drawn"
    e = draws * P
    big = e >= 5
    chi2 = (((counts[big] - e[big]) ** 2) / e[big]).sum()
    rest_o, rest_e = counts[~big].sum(), e[~big].sum()
    dof = int(big.sum()) - 1
    if rest_e >= 5:
        chi2 += (rest_o - rest_e) ** 2 / rest_e
        dof += 1
    assert chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)
    D = ssm.texel_centre_directions(w, h)
    rq = np.zeros((len(D), 24), np.float32)
    rq[:, :3] = D
    pdf = c.kat("sky_pdf", rq)
    omega = np.broadcast_to(ssm.solid_angles(w, h), (h, w)).reshape(-1)
    assert abs((pdf[:, 3].astype(np.float64) * omega).sum() - 1.0) < 1e-5
    c.destroy()


def frame_stack(pkg, c, scene, frames):
    import test_sky_sampling as base
    return base._frames(pkg, c, scene, frames)


def mean_z(fa, fb):
    """z of the difference of the image means of two stacks of independent frames (variance from the frames)."""
    a, b = fa.mean((1, 2, 3)), fb.mean((1, 2, 3))
    return float((a.mean() - b.mean()) / np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b) + 1e-30)), float(a.mean()), float(b.mean())
