"""What tests/test_texture_decode.py (host emulation) and tests/test_texture_decode_gpu.py (the HIP kernels) both ask of a context:
a decoded image equals the numpy model (tests/texture_decode_model.py) byte for byte on both entropy paths, the coefficients and the
record match, a device-built mip chain equals the model's texel for texel, malformed streams are refused with nothing written.  The
model's results are computed once per process and shared."""
import ctypes as C
import os

import numpy as np

import jpeg_model as jm
import texture_decode_model as tm
from display_jpeg_checks import model as jpeg_case

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, UNSUPPORTED = 1, 5  # RFWHIP_ERR_INVALID_ARGUMENT, RFWHIP_ERR_UNSUPPORTED
PATH_HOST, PATH_DEVICE = 1, 2
MIP_SIZES = [(1, 1), (2, 2), (3, 5), (16, 16), (17, 9), (67, 35), (130, 70)]
_GOLDEN = {}


def golden():
    if not _GOLDEN:
        with np.load(os.path.join(HERE, "golden", "texture_streams.npz")) as f:
            _GOLDEN.update({k: f[k] for k in f.files})
    return _GOLDEN


def golden_streams():
    """[(name, the stream's bytes, Pillow's decode H x W x 3)]."""
    g = golden()
    return [(k[4:], g[k].tobytes(), g["dec_" + k[4:]]) for k in sorted(g) if k.startswith("jpg_")]


def matrix():
    """The cases of item 2: every size x subsampling x quality x Ri, the three plain inputs in rotation (as display_jpeg_checks.matrix)."""
    k = 0
    for (w, h) in jm.SIZES + [(33, 17), (5, 4), (4, 9), (2, 3)]:
        for sub in ("444", "420"):
            for quality in (1, 90, 100):
                for ri in (1, 8, 11, 65535):
                    yield ("constant", "smooth", "noise")[k % 3], w, h, quality, sub, ri
                    k += 1


def decode_matches_the_model(c, stream, label, coefficients=None):
    """decode_image on both entropy paths and on `auto`: the image, the coefficients and the record."""
    want, coef, info = tm.decode_cached(stream)
    if coefficients is not None:
        assert np.array_equal(coef, coefficients), (label, "the model's coefficients are not the encoder's")
    blocks, intervals = info["mw"] * info["mh"] * info["bpm"], len(info["intervals"])
    for mode in ("auto", "host", "device"):
        c.set_setting("texture_entropy", mode)
        got = c.decode_image(stream)
        assert got.shape == want.shape, (label, mode, got.shape)
        assert np.array_equal(got, want), (label, mode, "%d texels differ" % int((got != want).any(-1).sum()))
        assert np.array_equal(c.texture_coefficients(), coef), (label, mode)
        path = PATH_HOST if mode == "host" or (mode == "auto" and not info["ri"]) else PATH_DEVICE
        assert c.texture_record() == dict(width=info["w"], height=info["h"], blocks=blocks, intervals=intervals, errors=0, alpha_zero=0,
                                          path=path), (label, mode, c.texture_record())
    c.set_setting("texture_entropy", "auto")


def jm_case_matches(c, name, w, h, quality, sub, ri):
    _, stream, facts, coef = jpeg_case(name, w, h, quality, sub, ri)
    decode_matches_the_model(c, stream, (name, w, h, quality, sub, ri), coef)
    assert c.texture_record()["intervals"] == facts["intervals"] and c.texture_record()["blocks"] == facts["blocks"]


def noise_rgba(w, h, seed=5):
    rng = np.random.default_rng(seed + 131 * w + h)
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[..., 3][rng.random((h, w)) < 0.25] = 0
    return px


def mips_match(c, w, h, flags=0):
    """An RGBA8 source with random alpha (zeros among it): every level, the texel count and the alpha-zero count."""
    px = noise_rgba(w, h)
    c.set_textures([{"kind": "rgba8", "data": px, "flags": flags}])
    got, want = c.read_texture(0), tm.chain(tm.modify(px, flags))
    assert len(got) == tm.chain_texels(w, h) == len(want), (w, h, len(got))
    assert np.array_equal(got, want), (w, h, flags, "first difference at texel %d" % int(np.argmax(got != want)))
    rec = c.texture_record(0)
    assert rec == dict(width=w, height=h, blocks=0, intervals=0, errors=0, alpha_zero=int((px[..., 3] == 0).sum()), path=0), rec


def modifiers_match(c, stream):
    """Flip, c c >> 8 and the sRGB table against the model, through a JPEG and through RGBA8 pixels; linearisation before the mips."""
    for flags in (tm.FLIP_ROWS, tm.LINEARIZE_REFERENCE, tm.LINEARIZE_SRGB, tm.FLIP_ROWS | tm.LINEARIZE_SRGB):
        want = tm.decode_cached(stream, flags)[0]
        assert np.array_equal(c.decode_image(stream, flags), want), flags
        c.set_textures([{"kind": "jpeg", "data": stream, "flags": flags}])
        assert np.array_equal(c.read_texture(0), tm.chain(want)), flags  # (the chain of the LINEARISED level 0)
        mips_match(c, 19, 10, flags)
    t = tm.srgb_table()
    assert t[0] == 0 and t[255] == 255 and t[128] == 55 and (np.diff(t.astype(int)) >= 0).all()


def mixed_table(c, pkg, good, corrupt):
    """TEXELS + JPEG + RGBA8 in one call; then the same with a corrupt middle stream: refused, index 1 named, the table unchanged."""
    import pytest
    texels = pkg.scenes.make_texture_rgba8(noise_rgba(6, 4, 9))
    px = noise_rgba(9, 7, 3)
    c.set_textures([texels, {"kind": "jpeg", "data": good, "flags": 0}, {"kind": "rgba8", "data": px, "flags": tm.FLIP_ROWS}])
    want = [np.asarray(texels["data"], np.uint32), tm.chain(tm.decode_cached(good)[0]), tm.chain(tm.modify(px, tm.FLIP_ROWS))]

    def table_is_intact():
        for i, w in enumerate(want):
            assert np.array_equal(c.read_texture(i), w), i
        assert c.texture_record(0)["width"] == 0 and c.texture_record(1)["blocks"] > 0 and c.texture_record(2)["path"] == 0
    table_is_intact()
    for bad in corrupt:
        with pytest.raises(RuntimeError, match="texture 1"):
            c.set_textures([texels, {"kind": "jpeg", "data": bad, "flags": 0}, {"kind": "rgba8", "data": px, "flags": 0}])
        table_is_intact()


def sampler_walks_the_chain(c, pkg):
    """A device-built chain through the existing `tex_fetch` hook at level 0 and at level 2.  The image is made of 16 x 16 cells of
    one colour each and sampled at the cells' centres, where all four taps of the bilinear fetch are texels of that cell on either
    level (a level-2 texel covers 4 x 4 texels of one cell): the answer is the model's texel / 256 up to float32 rounding."""
    w, h, cell = 64, 48, 16
    rng = np.random.default_rng(17)
    cells = rng.integers(0, 256, (h // cell, w // cell, 4), dtype=np.uint8)
    px = np.kron(cells, np.ones((cell, cell, 1), np.uint8))
    s = pkg.scenes.Scene()
    s.add_texture({"kind": "rgba8", "data": px, "flags": 0, "type": pkg.abi.TEX_UINT, "width": w, "height": h})
    m = s.add_material(color=(0.5, 0.5, 0.5))
    s.add_instance(s.add_mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32), material=m))
    c.init(64, 48)
    s.upload(c)
    chain = tm.chain(px)
    assert np.array_equal(c.read_texture(0), chain)
    cy, cx = np.mgrid[0:h // cell, 0:w // cell]
    for level in (0, 2):
        lw, lh, off = w >> level, h >> level, sum((w >> i) * (h >> i) for i in range(level))
        rec = np.zeros((cx.size, 24), np.float32)
        ri = rec.view(np.uint32)
        ri[:, 0], ri[:, 5], ri[:, 6] = 0, w, h
        rec[:, 2], rec[:, 3], rec[:, 4] = level, (cx.reshape(-1) + 0.5) * cell / w, (cy.reshape(-1) + 0.5) * cell / h
        got = c.kat("tex_fetch", rec)[:, :4].astype(np.float64)
        tx, ty = (cx.reshape(-1) * cell + cell // 2) >> level, (cy.reshape(-1) * cell + cell // 2) >> level
        texel = chain[off + ty * lw + tx]
        want = np.stack([(texel >> sh) & 255 for sh in (0, 8, 16, 24)], -1) / 256.0
        assert np.abs(got - want).max() <= 4 * 2.0 ** -24, (level, np.abs(got - want).max())  # (four products and three sums of float32)


# ---- malformed input -------------------------------------------------------------------------------------------------------
def _scan(bits):
    """A bit string -> entropy bytes: padded with 1-bits, a 0x00 behind every 0xFF."""
    bits += "1" * (-len(bits) % 8)
    out = bytearray()
    for i in range(0, len(bits), 8):
        b = int(bits[i:i + 8], 2)
        out.append(b)
        if b == 255:
            out.append(0)
    return bytes(out)


def malformed():
    """[(name, stream, the code it must be refused with, scan level: the walk accepts it and the entropy decoder refuses it)], built by
    editing a good stream: 17 x 9, 4:4:4, Ri = 1 (six intervals)."""
    good = jpeg_case("smooth", 17, 9, 90, "444", 1)[1]
    one = jpeg_case("noise", 17, 9, 90, "444", 65535)[1]  # one interval
    dqt, sof, dht, sos = good.index(b"\xff\xdb"), good.index(b"\xff\xc0"), good.index(b"\xff\xc4"), good.index(b"\xff\xda")
    n_dqt = 2 + int.from_bytes(good[dqt + 2:dqt + 4], "big")
    rst0, s1 = good.index(b"\xff\xd0", sos), one.index(b"\xff\xda") + 14  # (s1: the first byte of `one`'s entropy data)

    def edit(at, value):
        b = bytearray(good)
        b[at:at + len(value)] = value
        return bytes(b)
    head = jm.header(8, 8, 90, "444", 1)
    dc0, ac = "".join(format(jm.codes(jm.DCL)[0][0], "0%db" % jm.codes(jm.DCL)[0][1])), jm.codes(jm.ACL)
    f1 = format(ac[0xF1][0], "0%db" % ac[0xF1][1]) + "1"  # run 15, size 1, the value +1
    return [
        ("truncated inside a segment header", good[:dqt + 3], INVALID, False),
        ("truncated inside the scan", good[:sos + 14 + (len(good) - sos - 14) // 2], INVALID, False),
        ("DHT whose counts overrun its length", edit(dht + 5 + 15, b"\xff"), INVALID, False),
        ("SOS naming an undefined table", edit(sos + 6, b"\x33"), INVALID, False),
        ("missing DQT", good[:dqt] + good[dqt + n_dqt:], INVALID, False),
        ("width 0", edit(sof + 7, b"\x00\x00"), INVALID, False),
        ("RST out of sequence", edit(rst0 + 1, b"\xd3"), INVALID, False),
        ("a run past coefficient 63", head + _scan(dc0 + f1 * 5) + b"\xff\xd9", INVALID, True),
        ("a code with no match", head + _scan(dc0 + "1" * 16) + b"\xff\xd9", INVALID, True),
        ("no EOI", good[:-2], INVALID, False),
        ("an interval cut short", one[:s1 + (len(one) - 2 - s1) // 2] + b"\xff\xd9", INVALID, True),
    ]


def refused_with_nothing_written(c, name, stream, code):
    """rfwhip_decode_image answers `code`, names the cause, and leaves the output and the bytes behind it as they were."""
    fn = c._fn("decode_image")
    src = np.frombuffer(stream, np.uint8)
    buf = np.full(4096 * 4 + 64, 0xA5, np.uint8)
    w, h = C.c_uint32(), C.c_uint32()
    got = fn(c._ctx, src.ctypes.data, src.size, 0, buf.ctypes.data, 4096, C.byref(w), C.byref(h))
    assert got == code, (name, got, c._fn("last_error")().decode())
    assert len(c._fn("last_error")().decode()) > len("rfwhip_decode_image: "), name
    assert (buf == 0xA5).all(), name
    return c._fn("last_error")().decode()


# ---- the front ends --------------------------------------------------------------------------------------------------------
def red_over_blue(w=16, h=16):
    px = np.zeros((h, w, 4), np.uint8)
    px[..., 3] = 255
    px[:h // 2, :, 0], px[h // 2:, :, 2] = 255, 255
    return px


def png_bytes(px):
    """A minimal RGBA PNG (filter None) of H x W x 4 pixels."""
    import struct
    import zlib
    h, w = px.shape[:2]

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    raw = b"".join(b"\x00" + px[y].tobytes() for y in range(h))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")


def write_quad_files(tmp_path):
    """A .gltf with a data-uri JPEG and an .obj + .mtl + .png: a two-triangle quad in the plane z = 0, upright (y up), whose texture
    is red above blue.  The uv of each follows its own convention: glTF's v = 0 is the image's top, OBJ's its bottom."""
    import base64
    import json
    stream = jm.encode(red_over_blue(), 100, "444", 2)[0]
    pos = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
    uv = np.array([[0, 1], [1, 1], [1, 0], [0, 0]], np.float32)  # top of the quad (y = 1) <-> v = 0 <-> the image's top row
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    blob = pos.tobytes() + uv.tobytes() + idx.tobytes()
    doc = {
        "asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}],
        "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "TEXCOORD_0": 1}, "indices": 2, "material": 0}]}],
        "materials": [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}}],
        "textures": [{"source": 0}], "images": [{"uri": "data:image/jpeg;base64," + base64.b64encode(stream).decode()}],
        "buffers": [{"uri": "data:application/octet-stream;base64," + base64.b64encode(blob).decode(), "byteLength": len(blob)}],
        "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 48}, {"buffer": 0, "byteOffset": 48, "byteLength": 32},
                        {"buffer": 0, "byteOffset": 80, "byteLength": 12}],
        "accessors": [{"bufferView": 0, "componentType": 5126, "count": 4, "type": "VEC3", "min": [-1, -1, 0], "max": [1, 1, 0]},
                      {"bufferView": 1, "componentType": 5126, "count": 4, "type": "VEC2"},
                      {"bufferView": 2, "componentType": 5123, "count": 6, "type": "SCALAR"}]}
    gltf = tmp_path / "quad.gltf"
    gltf.write_text(json.dumps(doc))
    (tmp_path / "quad.png").write_bytes(png_bytes(red_over_blue()))
    (tmp_path / "quad.mtl").write_text("newmtl card\nKd 1 1 1\nmap_Kd quad.png\n")
    obj = tmp_path / "quad.obj"
    obj.write_text("mtllib quad.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\n"
                   "usemtl card\nf 1/1/1 2/2/1 3/3/1\nf 1/1/1 3/3/1 4/4/1\n")
    return str(gltf), str(obj)


def renders_red_over_blue(c, pkg, scene):
    """A 48 x 32 render of the quad, lit from the camera's side: the upper half of the image is red, the lower half blue — the order
    of the two channels' means in each half, not a value (the BSDF scales both alike)."""
    scene.camera.look_at((0.0, 0.0, 3.2), (0.0, 0.0, 0.0))
    scene.camera.resize(48, 32)
    scene.add_point_light((0.0, 0.0, 3.0), (40.0, 40.0, 40.0))
    c.init(48, 32)
    scene.upload(c)
    c.set_setting("integrator", "pt")
    c.set_setting("spp", 8)
    c.render_frame(scene.camera, pkg.RESET)
    img = c.framebuffer()[..., :3].astype(np.float64)
    top, bottom = img[4:12, 16:32].mean((0, 1)), img[20:28, 16:32].mean((0, 1))
    assert top[0] > top[2] and top[0] > 0, ("the upper half is not red", top, bottom)
    assert bottom[2] > bottom[0] and bottom[2] > 0, ("the lower half is not blue", top, bottom)
