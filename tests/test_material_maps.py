"""The setting material_maps (include/rfwhip.h): the alpha mask of map slot 9 and the roughness / metallic
maps of slots 7 / 6 in the path tracer.  The rule is held three ways:

1. rfwhip_kat's `surface_maps` against the numpy model of tests/material_maps_model.py (its docstring derives the allowance): constant
   maps byte for byte, the shapes where a fetch can go wrong, and random 16 x 16 maps with mips;
2. images, all compared bit for bit: the setting without maps and maps without the setting change nothing, a constant map equals the
   scalar it works out to, a mask equals MF_ALPHA on the same texels (image, ray counts, denoiser guides), and a mapped material
   leaves the pixels whose paths never meet it alone;
3. the front ends: pack_materials, a .gltf with a metallicRoughnessTexture and alphaMode MASK, an .obj with map_d; and the plugin's
   RFWHIP_MATERIAL_MAPS.

CPU tier: the host emulation runs the work items of the HIP kernels.  The tests marked gpu are the same checks on the kernels, and
the strict (validation) build against its emulation bit for bit.  96 x 64 pixels, 4 spp, depth 2.
"""
import base64
import ctypes
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import material_maps_model as mm
from conftest import ROOT
from plugin_hosts import build_host, run_host

f32 = np.float32
STRICT_FLAGS = ("-DRT_STRICT_MATH", "-ffp-contract=off")
SET = (0, 1, 2, 3, 127, 128, 254, 255)


@pytest.fixture(scope="module")
def emu_strict_lib():
    import build_emu
    return ctypes.CDLL(build_emu.build(defines=STRICT_FLAGS, tag="_strict"))


def _strict_hip(pkg):
    so = os.path.join(ROOT, "tests", "_strict", "librfwhip_strict.so")
    assert os.path.exists(so), "build it with __graft_entry__.build() (build.py: build_strict)"
    return pkg._binding.CoreBinding(ctypes.CDLL(so), "rfwhip_", 0, 0, 1)


def _makers(request, pkg, which):
    """name -> a function that makes a fresh context of that implementation."""
    out = {}
    for w in which:
        if w == "emulation":
            out[w] = request.getfixturevalue("make_emu")
        elif w == "hip":
            out[w] = request.getfixturevalue("make_hip")
        elif w == "strict hip":
            out[w] = lambda: _strict_hip(pkg)
        elif w == "strict emulation":
            lib = request.getfixturevalue("emu_strict_lib")
            out[w] = lambda lib=lib: pkg._binding.CoreBinding(lib, "rfwhip_", 0, 0, 1)
    return out


SPREAD = f32(np.radians(40.0) / 64)


# ----------------------------------------------------------------------------------------------------------------------
# 1. known answers
# ----------------------------------------------------------------------------------------------------------------------
def _constant_pairs():
    """(parameter byte, texel byte) -> (the records under the 3 % condition, the set's exact ties).  The records: the pairs of the set
    and 200 random ones.  Eight of the set's 64 pairs are exact ties of the 1 / 256 scaling (P T = 128 mod 256: 128 with an odd
    byte) — 3.03 % of 264 records by themselves, before any random pair — so they are not among the records: they run beside them
    and are held to "either neighbouring byte"."""
    rng = np.random.default_rng(2510)
    grid = [(p, t) for p in SET for t in SET]
    ties = [q for q in grid if (q[0] * q[1]) % 256 == 128]
    pairs = [q for q in grid if q not in ties] + [tuple(int(v) for v in rng.integers(0, 256, 2)) for _ in range(200)]
    assert len(ties) == 8 and len(pairs) == 256
    return np.asarray(pairs, np.int64), np.asarray(ties, np.int64)


def _constant_model(pairs):
    """The exact product of chan = P / 255 and texel = T / 256 in byte units, P T / 256, its byte and the distance of
    P T / 256 + 0.5 to the nearest integer — the rounding boundary of byte()."""
    v = pairs[:, 0] * pairs[:, 1] / 256.0 + 0.5
    return np.floor(v).astype(np.int64), np.abs(v - np.rint(v))


def _check_constant_maps(pkg, makers):
    records, ties = _constant_pairs()
    _, dist = _constant_model(records)
    # a condition on the records, from the model alone, before any library is asked: at most 3 % are left out
    assert (dist < 1e-3).mean() <= 0.03, (dist < 1e-3).mean()
    pairs = np.concatenate([records, ties])
    want, dist = _constant_model(pairs)
    keep = dist >= 1e-3
    n = len(pairs)
    # material k: roughness map, material n + k: metallic map; texture k holds pair k's texel byte in green and blue
    materials = []
    s, v, uv, rng = mm.triangle_zoo(pkg, range(2 * n))
    for p, t in pairs:
        s.add_texture(mm.constant_rgba8(pkg, (9, int(t), int(t), 255)))
    for k, (p, t) in enumerate(pairs):
        materials.append(s.add_material(roughness=mm.param(p), metallic=mm.param(77), roughnessmap=k))
    for k, (p, t) in enumerate(pairs):
        materials.append(s.add_material(roughness=mm.param(66), metallic=mm.param(p), metallicmap=k))
    mm.finish_zoo(s, v, uv, rng, materials)
    rec = mm.hit_records(s, 4 * n, 11, SPREAD)
    tri = rec.view(np.uint32)[:, 1].astype(np.int64)
    rough = tri < n
    k = np.where(rough, tri, tri - n)
    for who, make in makers.items():
        c = make()
        c.init(64, 48)
        s.upload(c)
        got = c.kat("surface_maps", rec).view(np.uint32)
        flags = got[:, 3]
        assert np.array_equal(flags, np.where(rough, 4, 2)), who
        assert np.all(c.kat("surface_maps", rec)[:, 2] == 1.0), who
        sel = keep[k]
        assert np.array_equal(got[rough & sel, 0], want[k[rough & sel]]), who
        assert np.array_equal(got[~rough & sel, 1], want[k[~rough & sel]]), who
        assert np.all(got[rough, 1] == 77) and np.all(got[~rough, 0] == 66), who  # (the other parameter is the material's)
        # (records at a tie: either neighbour)
        tie = ~sel
        g = np.where(rough, got[:, 0], got[:, 1]).astype(np.int64)
        assert np.all(np.abs(g[tie] - (pairs[k[tie], 0] * pairs[k[tie], 1] / 256.0)) <= 0.5 + 1e-3), who
    left = int((~keep[:len(records)]).sum())
    print("constant maps: %d records, %d left out (%.2f %%); %d exact ties of the set beside them" % (len(records), left, 100.0 * left / len(records), len(ties)))


def test_constant_maps_give_the_models_byte(request, pkg):
    _check_constant_maps(pkg, _makers(request, pkg, ("emulation",)))


@pytest.mark.gpu
def test_constant_maps_give_the_models_byte_gpu(request, pkg):
    _check_constant_maps(pkg, _makers(request, pkg, ("hip", "strict hip")))


def _shapes_scene(pkg):
    """The materials where a fetch, a descriptor or a flag can go wrong, one triangle each -> (scene, packed materials, ids)."""
    sc = pkg.scenes
    rng = np.random.default_rng(97)
    names = ["64x1", "1x7", "5x3", "nan", "range", "width0", "absent", "absent_big", "halves", "shared", "split", "alpha_and_mask",
             "all_three", "other_descriptor", "none"]
    s, v, uv, zrng = mm.triangle_zoo(pkg, names)
    def rgba8(w, h):
        return s.add_texture(sc.make_texture_rgba8(rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)))
    t64x1, t1x7, t5x3, t16, t16b, t8 = rgba8(64, 1), rgba8(1, 7), rgba8(5, 3), rgba8(16, 16), rgba8(16, 16), rgba8(8, 8)
    nan = np.full((2, 2, 4), 0.5, f32)
    nan[1, 0] = np.nan
    tnan = s.add_texture(sc.make_texture_float4(nan))
    trange = s.add_texture(sc.make_texture_float4(rng.uniform(-0.5, 1.75, size=(3, 5, 4)).astype(f32)))  # above 1 and below 0
    tconst = s.add_texture(mm.constant_rgba8(pkg, (200, 100, 50, 255)))
    tdiff = s.add_texture(sc.make_texture_rgba8(rng.integers(0, 256, size=(8, 8, 4), dtype=np.uint8)))
    P = dict(roughness=mm.param(201), metallic=mm.param(155))
    ids = {}
    ids["64x1"] = s.add_material(roughnessmap=t64x1, alphamap=t64x1, **P)
    ids["1x7"] = s.add_material(metallicmap=t1x7, alphamap=t1x7, **P)
    ids["5x3"] = s.add_material(roughnessmap=t5x3, metallicmap=t5x3, alphamap=t5x3, uvscale=(1.5, -0.75), **P)
    ids["nan"] = s.add_material(roughnessmap=tnan, metallicmap=tnan, **P)
    ids["range"] = s.add_material(roughnessmap=trange, metallicmap=trange, **P)
    ids["width0"] = s.add_material(roughnessmap=tconst, metallicmap=tconst, **P)           # (descriptor patched below)
    ids["absent"] = s.add_material(roughnessmap=t16, metallicmap=t16, alphamap=t16, **P)   # (addresses patched below)
    ids["absent_big"] = s.add_material(roughnessmap=t16, alphamap=t16, **P)
    ids["halves"] = s.add_material(roughnessmap=t16, metallicmap=t16b, alphamap=t8, uvscale=(-2.5, 1.5), uvoffset=(0.25, -0.75), **P)
    ids["shared"] = s.add_material(roughnessmap=t16, metallicmap=t16, **P)                  # NO diffuse map
    ids["split"] = s.add_material(roughnessmap=t16, metallicmap=t16b, **P)
    ids["alpha_and_mask"] = s.add_material(texture=tdiff, alpha=True, alphamap=t16, roughnessmap=t8, **P)
    ids["all_three"] = s.add_material(texture=tdiff, roughnessmap=t16b, metallicmap=t8, alphamap=t16b, uvscale=(0.5, 0.5), **P)
    ids["other_descriptor"] = s.add_material(roughnessmap=t16, metallicmap=t16, **P)        # (slot 6's scale patched: two fetches)
    ids["none"] = s.add_material(**P)
    mm.finish_zoo(s, v, uv, zrng, [ids[k] for k in names])
    mats, tex_ids = sc.pack_materials(s.host_materials, s.textures)
    tex_ids = tex_ids.copy()
    raw = tex_ids.view(np.int32).reshape(-1, 11)
    m = mats[ids["width0"]]
    m["map"][7]["width"], m["map"][6]["height"] = 0, 0
    count = len(s.textures)
    m = mats[ids["absent"]]
    m["map"][6]["addr"], m["map"][7]["addr"], m["map"][9]["addr"] = count, count + 5, count
    raw[ids["absent"], [6, 7, 10]] = -1  # (no id: the descriptor's address is taken as it is)
    m = mats[ids["absent_big"]]
    m["map"][7]["addr"], m["map"][9]["addr"] = 0xFFFFFFFF, 0x80000000
    raw[ids["absent_big"], [7, 10]] = -1
    mats[ids["other_descriptor"]]["map"][6]["uscale"] = np.float16(3.0)
    return s, mats, tex_ids, ids


def _check_shapes(pkg, makers):
    s, mats, tex_ids, ids = _shapes_scene(pkg)
    rec = mm.hit_records(s, 30_000, 23, SPREAD)
    present, P, x, dt = mm.evaluate(pkg, s, mats, rec)
    tri = rec.view(np.uint32)[:, 1]
    names = {k: i for i, k in enumerate(["64x1", "1x7", "5x3", "nan", "range", "width0", "absent", "absent_big", "halves", "shared", "split",
                                         "alpha_and_mask", "all_three", "other_descriptor", "none"])}
    # the model itself sees the cases: absent slots, a NaN, values clamped at both ends, passes on both sides of the mask
    assert not present[tri == names["absent"]].any() and not present[tri == names["absent_big"]].any() and not present[tri == names["none"]].any()
    assert np.isnan(x[tri == names["nan"], 0]).all()
    r = x[tri == names["range"], 1]
    assert (r > 1.0).any() and (r < 0.0).any()
    a = x[tri == names["alpha_and_mask"], 2]
    assert (a < 0.45).any() and (a > 0.55).any()
    got = {}
    for who, make in makers.items():
        c = mm.upload_with(make(), s, mats, tex_ids)
        got[who] = c.kat("surface_maps", rec)
        n, free = mm.check_surface_maps(got[who], present, P, x, dt, who)
        # the NaN map gives 0 (one fetch against two: test_one_fetch_for_two_slots_equals_two_fetches)
        g = got[who].view(np.uint32)
        assert not g[tri == names["nan"], 0].any() and not g[tri == names["nan"], 1].any(), who
        print("%s: %d records, %d with a free mask decision" % (who, n, free))
    return got


def test_shapes_where_it_can_go_wrong(request, pkg):
    _check_shapes(pkg, _makers(request, pkg, ("emulation",)))


@pytest.mark.gpu
def test_shapes_where_it_can_go_wrong_gpu(request, pkg):
    got = _check_shapes(pkg, _makers(request, pkg, ("hip", "strict hip", "strict emulation")))
    assert np.array_equal(got["strict hip"].view(np.uint32), got["strict emulation"].view(np.uint32))


def _gradient_scene(pkg):
    sc = pkg.scenes
    rng = np.random.default_rng(1616)
    n = 12
    s, v, uv, zrng = mm.triangle_zoo(pkg, range(n), uv_seed=8)
    tex = [s.add_texture(sc.make_texture_rgba8(rng.integers(0, 256, size=(16, 16, 4), dtype=np.uint8))) for _ in range(6)]
    mats = []
    for k in range(n):
        mats.append(s.add_material(roughness=mm.param(rng.integers(1, 256)), metallic=mm.param(rng.integers(1, 256)),
                                   roughnessmap=tex[k % 6], metallicmap=tex[(k // 2) % 6], alphamap=tex[(k + 3) % 6] if k % 3 else -1,
                                   uvscale=(float(rng.choice([1.0, 2.0, -1.5, 0.5])), float(rng.choice([1.0, -2.0, 0.75]))),
                                   uvoffset=(float(rng.choice([0.0, 0.25])), float(rng.choice([0.0, -0.5])))))
    mm.finish_zoo(s, v, uv, zrng, mats)
    return s


def _check_gradients(pkg, makers):
    s = _gradient_scene(pkg)
    mats, tex_ids = pkg.scenes.pack_materials(s.host_materials, s.textures)
    rec = mm.hit_records(s, 40_000, 31, SPREAD)
    present, P, x, dt = mm.evaluate(pkg, s, mats, rec)
    lo, hi = mm.accepted_bytes(P[:, 0], x[:, 1], dt[:, 1])
    # (the intervals decide something: the coordinate's allowance — float32 at 1000 + x, times 16 texels — is a few thousandths of a
    # texel per axis, a byte or two of a random map's slope; records whose lambda window holds 0 accept every byte)
    assert np.median(hi - lo) <= 4 and (hi - lo <= 8).mean() > 0.95, (np.median(hi - lo), (hi - lo <= 8).mean())
    got = {}
    for who, make in makers.items():
        c = make()
        c.init(64, 48)
        s.upload(c)
        got[who] = c.kat("surface_maps", rec)
        n, free = mm.check_surface_maps(got[who], present, P, x, dt, who)
        print("%s: %d records, %d with a free mask decision; %.1f %% of the roughness intervals hold one byte, %.1f %% at most three" % (who, n, free, 100 * (hi == lo).mean(), 100 * (hi - lo <= 2).mean()))
    return got


def test_gradient_maps_against_the_model(request, pkg):
    _check_gradients(pkg, _makers(request, pkg, ("emulation",)))


@pytest.mark.gpu
def test_gradient_maps_against_the_model_gpu(request, pkg):
    got = _check_gradients(pkg, _makers(request, pkg, ("hip", "strict hip", "strict emulation")))
    assert np.array_equal(got["strict hip"].view(np.uint32), got["strict emulation"].view(np.uint32))


def _check_one_fetch_equals_two(pkg, makers):
    """Slots 6 and 7 with one descriptor are served by one fetch: the bytes must be the ones two fetches give.  Three triangles with the
    same vertices, uvs and LOD: material 0 carries the texture in both slots, material 1 in slot 7 alone, material 2 in slot 6 alone;
    the same hits on each.  Roughness byte of 0 == of 1, metallic byte of 0 == of 2, bit for bit, on every implementation."""
    sc = pkg.scenes
    rng = np.random.default_rng(67)
    s = sc.Scene()
    t = s.add_texture(sc.make_texture_rgba8(rng.integers(0, 256, size=(16, 16, 4), dtype=np.uint8)))
    P = dict(roughness=mm.param(233), metallic=mm.param(181), uvscale=(1.5, -2.0), uvoffset=(0.25, 0.5))
    mats = [s.add_material(roughnessmap=t, metallicmap=t, **P), s.add_material(roughnessmap=t, **P), s.add_material(metallicmap=t, **P)]
    v = np.tile(np.array([[0, 0, 0], [1, 0, 0.2], [0.1, 1, 0.1]], f32), (3, 1))
    uv = np.tile(np.array([[-1.3, 0.2], [2.1, -0.4], [0.3, 2.7]], f32), (3, 1))
    mesh = s.add_mesh(v, None, uvs=uv, material=0)
    s.meshes[mesh]["triangles"]["material"][:] = np.asarray(mats, np.uint32)
    s.meshes[mesh]["triangles"]["LOD"][:] = f32(0.75)
    s.add_instance(mesh)
    one = mm.hit_records(s, 20_000, 41, SPREAD)
    recs = []
    for tri in range(3):
        r = one.copy()
        r.view(np.uint32)[:, 1] = tri
        recs.append(r)
    out = {}
    for who, make in makers.items():
        c = make()
        c.init(64, 48)
        s.upload(c)
        both, rough, metal = (c.kat("surface_maps", r).view(np.uint32) for r in recs)
        assert np.all(both[:, 3] == 6) and np.all(rough[:, 3] == 4) and np.all(metal[:, 3] == 2), who
        assert np.array_equal(both[:, 0], rough[:, 0]) and np.array_equal(both[:, 1], metal[:, 1]), who
        assert len(np.unique(both[:, 0])) > 50 and len(np.unique(both[:, 1])) > 50, who  # (a gradient: the fetch matters)
        out[who] = both
    return out


def test_one_fetch_for_two_slots_equals_two_fetches(request, pkg):
    _check_one_fetch_equals_two(pkg, _makers(request, pkg, ("emulation",)))


@pytest.mark.gpu
def test_one_fetch_for_two_slots_equals_two_fetches_gpu(request, pkg):
    got = _check_one_fetch_equals_two(pkg, _makers(request, pkg, ("hip", "strict hip", "strict emulation")))
    assert np.array_equal(got["strict hip"], got["strict emulation"])


def _check_setting_is_not_read_by_the_hook(pkg, make):
    """surface_maps works whatever the setting is, and the read-only key follows setting and materials."""
    s = _gradient_scene(pkg)
    rec = mm.hit_records(s, 500, 5, SPREAD)
    c = make()
    c.init(64, 48)
    assert c.get_setting("material_maps") == "0" and c.get_setting("material_maps_on") == "0"
    assert "material_maps" not in c.get_settings()
    s.upload(c)
    a = c.kat("surface_maps", rec)
    assert c.get_setting("material_maps_on") == "0"
    c.set_setting("material_maps", 1)
    assert c.get_setting("material_maps_on") == "1"
    assert np.array_equal(a.view(np.uint32), c.kat("surface_maps", rec).view(np.uint32))
    c.set_textures([])  # (no texture behind any address: no slot is present)
    assert c.get_setting("material_maps_on") == "0"
    with pytest.raises(RuntimeError):
        c.set_setting("material_maps", 2)
    with pytest.raises(RuntimeError):
        c.set_setting("material_maps_on", 1)


def test_the_hook_works_whatever_the_setting_is(pkg, make_emu):
    _check_setting_is_not_read_by_the_hook(pkg, make_emu)


@pytest.mark.gpu
def test_the_hook_works_whatever_the_setting_is_gpu(pkg, make_hip):
    _check_setting_is_not_read_by_the_hook(pkg, make_hip)


# ----------------------------------------------------------------------------------------------------------------------
# 2. images
# ----------------------------------------------------------------------------------------------------------------------
W, H = 96, 64
BOX = 3  # scenes.cornell: the boxes' material


def _mapped_boxes(pkg, f, t, fm=255, tm=64):
    """Scene A of (c): the boxes' material with a constant roughness map (factor byte f, texel byte t in green) and a constant
    metallic map (fm, tm in blue)."""
    s = mm.room(pkg, W, H)
    tr = s.add_texture(mm.constant_rgba8(pkg, (255, t, 255, 255)))
    tm_ = s.add_texture(mm.constant_rgba8(pkg, (255, 255, tm, 255)))
    s.host_materials[BOX].update(roughness=mm.param(f), metallic=mm.param(fm), roughnessmap=tr, metallicmap=tm_)
    return s


def _scalar_boxes(pkg, f, t, fm=255, tm=64):
    """Scene B of (c): the expected bytes in parameters[0], and a mapped material no triangle uses."""
    s = mm.room(pkg, W, H)
    tr = s.add_texture(mm.constant_rgba8(pkg, (255, t, 255, 255)))
    s.add_texture(mm.constant_rgba8(pkg, (255, 255, tm, 255)))
    want_r, dr = _constant_model(np.array([[f, t]]))
    want_m, dm = _constant_model(np.array([[fm, tm]]))
    assert dr[0] > 0.1 and dm[0] > 0.1  # (well away from a rounding boundary: the device's byte is the model's)
    s.host_materials[BOX].update(roughness=mm.param(want_r[0]), metallic=mm.param(want_m[0]))
    s.add_material(roughnessmap=tr)
    return s, int(want_r[0])


def _mask_scenes(pkg):
    """(d): A = a card whose diffuse texture is white with the mask in its alpha channel, with MF_ALPHA; B = the white texture with
    alpha 255 and the mask in the RGB of an alpha map."""
    mask = mm.mask_image()
    white = np.full((16, 16, 4), 255, np.uint8)
    a = mm.room(pkg, W, H)
    wa = white.copy()
    wa[..., 3] = mask
    mm.add_card(a, a.add_material(color=(0.8, 0.7, 0.6), texture=a.add_texture(pkg.scenes.make_texture_rgba8(wa)), alpha=True))
    b = mm.room(pkg, W, H)
    mk = white.copy()
    mk[..., :3] = mask[..., None]
    mm.add_card(b, b.add_material(color=(0.8, 0.7, 0.6), texture=b.add_texture(pkg.scenes.make_texture_rgba8(white)),
                                  alphamap=b.add_texture(pkg.scenes.make_texture_rgba8(mk))))
    return a, b


def _side_card_scene(pkg, card=True):
    """(e): the room, and beside it — outside the left wall, facing the camera — a card with all three maps.  No ray that leaves
    the room or the sky reaches it: only the pixels that see it have paths on it."""
    s = mm.room(pkg, W, H)
    rng = np.random.default_rng(4)
    t = s.add_texture(pkg.scenes.make_texture_rgba8(rng.integers(0, 256, size=(16, 16, 4), dtype=np.uint8)))
    m = s.add_material(color=(0.7, 0.7, 0.7), roughness=0.9, metallic=0.8, roughnessmap=t, metallicmap=t,
                       alphamap=s.add_texture(pkg.scenes.make_texture_rgba8(np.repeat(mm.mask_image()[..., None], 4, -1))))
    if card:
        mm.add_card(s, m, centre=(-6.6, 5.0, -3.0), size=2.6)
    return s


def _cleared(pkg, scene):
    """The same scene with bits 4, 5 and 13 cleared: its packed materials without those flags."""
    def upload(c):
        scene.upload(c)
        mats, ids = pkg.scenes.pack_materials(scene.host_materials, scene.textures)
        mats["flags"] &= ~np.uint32((1 << 4) | (1 << 5) | (1 << 13))
        c.set_materials(mats, ids)
        c.update()
    return upload


def _guides(c):
    g = c.read_denoise_guides()
    return np.concatenate([g["albedo"].reshape(-1), g["normal"].reshape(-1), g["z"].reshape(-1), g["valid"].reshape(-1).astype(f32)]).view(np.uint32)


def _check_setting_on_without_maps(pkg, make):
    """(a)"""
    s = pkg.scenes.cards(W, H)
    off, n_off = mm.render(make(), s, {"material_maps": 0})
    c = make()
    on, n_on = mm.render(c, s, {"material_maps": 1})
    assert c.get_setting("material_maps_on") == "0" and c.get_setting("textured") == "1"
    assert np.array_equal(off.view(np.uint32), on.view(np.uint32)) and n_off == n_on


def _check_setting_off_with_maps(pkg, make):
    """(b)"""
    for s in (_mapped_boxes(pkg, 200, 128), _mask_scenes(pkg)[1]):
        c = make()
        a, na = mm.render(c, s, {"material_maps": 0})
        assert c.get_setting("material_maps_on") == "0"
        b, nb = mm.render(make(), s, {"material_maps": 0}, upload=_cleared(pkg, s))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and na == nb


def _check_constant_map_equals_scalar(pkg, make, extra, equal_to=None):
    """(c)  -> the images of scene A, by case"""
    out = {}
    for name, (f, t) in (("rough", (200, 128)), ("specular", (4, 128))):
        sa = _mapped_boxes(pkg, f, t)
        sb, byte_r = _scalar_boxes(pkg, f, t)
        assert (byte_r == 2) == (name == "specular") and (byte_r / 255.0 < 0.01) == (name == "specular")
        ca, cb = make(), make()
        a, na = mm.render(ca, sa, dict({"material_maps": 1}, **extra))
        b, nb = mm.render(cb, sb, dict({"material_maps": 1}, **extra))
        assert ca.get_setting("material_maps_on") == "1" and cb.get_setting("material_maps_on") == "1"
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and na == nb, (name, extra)
        # ... and the map is read: without the setting scene A is another image
        plain, _ = mm.render(make(), sa, dict({"material_maps": 0}, **extra))
        assert not np.array_equal(a, plain), (name, extra)
        out[name] = a
    assert not np.array_equal(out["rough"], out["specular"])
    return out


VARIANTS = [{}, {"sky_sampling": 1}, {"light_sampling": "tree"}, {"sky_sampling": 1, "light_sampling": "tree"}]
VARIANT_IDS = ["default", "sky", "tree", "sky+tree"]


def _check_mask_equals_alpha(pkg, make):
    """(d)  -> (image, counts, guides) of scene B"""
    sa, sb = _mask_scenes(pkg)
    ca, cb = make(), make()
    a, na = mm.render(ca, sa, {"material_maps": 1})
    b, nb = mm.render(cb, sb, {"material_maps": 1})
    assert ca.get_setting("material_maps_on") == "0" and cb.get_setting("material_maps_on") == "1"
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert na == nb
    ga, gb = _guides(ca), _guides(cb)
    assert np.array_equal(ga, gb)
    # the mask is seen through: without the setting scene B shows an opaque card, in the image and in the guides — and turning the
    # setting off makes the guides of the same frame stale
    cb.set_setting("material_maps", 0)
    assert not np.array_equal(_guides(cb), gb)
    opaque, _ = mm.render(make(), sb, {"material_maps": 0})
    assert not np.array_equal(opaque, b)
    return b, nb, gb


def _check_mixed_materials(pkg, make):
    """(e)"""
    s = _side_card_scene(pkg)
    con, coff = make(), make()
    on, _ = mm.render(con, s, {"material_maps": 1})
    off, _ = mm.render(coff, s, {"material_maps": 0})
    assert con.get_setting("material_maps_on") == "1"
    bare, _ = mm.render(make(), _side_card_scene(pkg, card=False), {"material_maps": 0})
    # the pixels the card does not reach: those the scene without the card renders the same, setting off
    untouched = (off.view(np.uint32) == bare.view(np.uint32)).all(-1)
    touched = ~untouched
    assert untouched.sum() > 0.5 * W * H and touched.sum() > 20, (untouched.sum(), touched.sum())
    assert touched[:, :2 * W // 3].sum() == 0  # (the card shows at one edge of the image: -x of the world is its right)
    assert np.array_equal(on.view(np.uint32)[untouched], off.view(np.uint32)[untouched])
    assert not np.array_equal(on[touched], off[touched])  # (and the maps are read where the card is)


def _source_scene(pkg):
    """The room with the boxes' roughness / metallic map and a card's mask handed over as image SOURCES (PNG files the device turns
    into textures: rfwhip_set_texture_sources), as the front ends hand them over with load_images."""
    rng = np.random.default_rng(58)
    s = mm.room(pkg, W, H)
    mr = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    t = s.add_texture(pkg.images.texture_from_bytes(_png(mr)))
    s.host_materials[BOX].update(roughness=mm.param(250), metallic=mm.param(200), roughnessmap=t, metallicmap=t)
    mask = np.repeat(mm.mask_image()[..., None], 4, -1)
    mm.add_card(s, s.add_material(color=(0.8, 0.7, 0.6), alphamap=s.add_texture(pkg.images.texture_from_bytes(_png(mask)))))
    assert all(tx.get("kind") == "rgba8" for tx in s.textures)
    return s


def _materials_first(pkg, scene):
    """Scene.upload's calls with the materials in front of the textures."""
    def upload(c):
        pix, w, h = scene.sky
        c.set_sky(pix, w, h)
        mats, ids = pkg.scenes.pack_materials(scene.host_materials, scene.textures)
        c.set_materials(mats, ids)
        c.set_textures(scene.textures)
        for i, m in enumerate(scene.meshes):
            c.set_mesh(i, m["vertices"], m["triangles"], m["indices"])
        for i, inst in enumerate(scene.instances):
            c.set_instance(i, inst["mesh"], inst["transform"])
        c.set_lights(*scene.light_arrays())
        c.update()
    return upload


def _check_call_order_of_sources(pkg, make):
    """Presence depends on the texture count, whichever call sets it: materials first and the textures as sources afterwards runs the
    map kernels and renders the image of the other call order; replacing the textures follows."""
    s = _source_scene(pkg)
    ca, cb = make(), make()
    a, na = mm.render(ca, s, {"material_maps": 1})
    b, nb = mm.render(cb, s, {"material_maps": 1}, upload=_materials_first(pkg, s))
    assert ca.get_setting("material_maps_on") == "1" and cb.get_setting("material_maps_on") == "1"
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and na == nb
    off, _ = mm.render(make(), s, {"material_maps": 0}, upload=_materials_first(pkg, s))
    assert not np.array_equal(off, b)  # (the maps are read)
    cb.set_textures([])
    assert cb.get_setting("material_maps_on") == "0"
    cb.set_textures(s.textures)
    assert cb.get_setting("material_maps_on") == "1"
    cb.update()
    cb.render_frame(s.camera, 0)
    assert np.array_equal(cb.framebuffer().view(np.uint32), a.view(np.uint32))


def test_sources_after_the_materials(pkg, make_emu):
    _check_call_order_of_sources(pkg, make_emu)


@pytest.mark.gpu
def test_sources_after_the_materials_gpu(pkg, make_hip):
    _check_call_order_of_sources(pkg, make_hip)


def test_setting_on_without_maps_changes_nothing(pkg, make_emu):
    _check_setting_on_without_maps(pkg, make_emu)


def test_setting_off_ignores_the_maps(pkg, make_emu):
    _check_setting_off_with_maps(pkg, make_emu)


@pytest.mark.parametrize("extra", VARIANTS, ids=VARIANT_IDS)
def test_constant_map_equals_the_scalar(pkg, make_emu, extra):
    _check_constant_map_equals_scalar(pkg, make_emu, extra)


def test_mask_equals_the_alpha_flag(pkg, make_emu):
    _check_mask_equals_alpha(pkg, make_emu)


def test_mixed_materials_leave_the_other_pixels_alone(pkg, make_emu):
    _check_mixed_materials(pkg, make_emu)


@pytest.mark.gpu
def test_images_gpu(request, pkg, make_hip):
    """(a), (b), (d), (e) on the shipped kernels — the device against itself — and (d) on the strict build against its emulation."""
    _check_setting_on_without_maps(pkg, make_hip)
    _check_setting_off_with_maps(pkg, make_hip)
    _check_mask_equals_alpha(pkg, make_hip)
    _check_mixed_materials(pkg, make_hip)
    mk = _makers(request, pkg, ("strict hip", "strict emulation"))
    dev, emu = _check_mask_equals_alpha(pkg, mk["strict hip"]), _check_mask_equals_alpha(pkg, mk["strict emulation"])
    assert np.array_equal(dev[0].view(np.uint32), emu[0].view(np.uint32)) and dev[1] == emu[1] and np.array_equal(dev[2], emu[2])


@pytest.mark.gpu
@pytest.mark.parametrize("extra", VARIANTS, ids=VARIANT_IDS)
def test_constant_map_equals_the_scalar_gpu(request, pkg, make_hip, extra):
    """(c) on the shipped kernels, and the strict build bit-equal to its emulation."""
    _check_constant_map_equals_scalar(pkg, make_hip, extra)
    mk = _makers(request, pkg, ("strict hip", "strict emulation"))
    dev, emu = _check_constant_map_equals_scalar(pkg, mk["strict hip"], extra), _check_constant_map_equals_scalar(pkg, mk["strict emulation"], extra)
    for k in dev:
        assert np.array_equal(dev[k].view(np.uint32), emu[k].view(np.uint32)), (k, extra)


# ----------------------------------------------------------------------------------------------------------------------
# 3. front ends
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("faithful", [False, True])
def test_pack_materials_packs_the_three_slots(pkg, faithful):
    sc, abi = pkg.scenes, pkg.abi
    tex = [mm.constant_rgba8(pkg, (1, 2, 3, 4), w, h) for w, h in ((4, 4), (8, 2), (2, 16), (5, 3))]
    hm = [sc.host_material(texture=0, roughnessmap=1, metallicmap=2, alphamap=3, uvscale=(2.0, 0.5), uvoffset=(0.25, -1.0)),
          sc.host_material(roughnessmap=2), sc.host_material(alphamap=0), sc.host_material()]
    mats, ids = sc.pack_materials(hm, tex, faithful=faithful)
    ids = ids.view(np.int32).reshape(-1, 11)
    bits = lambda m: int(m["flags"]) & ((1 << 4) | (1 << 5) | (1 << 13))  # noqa: E731
    assert bits(mats[0]) == (1 << 4) | (1 << 5) | (1 << 13) and bits(mats[1]) == 1 << 5 and bits(mats[2]) == 1 << 13 and bits(mats[3]) == 0
    assert (1 << abi.MAT_HAS_ROUGHNESS_MAP, 1 << abi.MAT_HAS_SPECULARITY_MAP, 1 << abi.MAT_HAS_ALPHA_MAP) == (1 << 5, 1 << 4, 1 << 13)
    assert list(ids[0]) == [0, -1, -1, -1, -1, -1, 2, 1, -1, -1, 3] and list(ids[1][6:]) == [-1, 2, -1, -1, -1] and ids[2][10] == 0
    assert (ids[3] == -1).all() and ids[2][9] == -1
    for slot, t in ((7, 1), (6, 2), (9, 3)):
        d = mats[0]["map"][slot]
        assert (int(d["width"]), int(d["height"])) == (tex[t]["width"], tex[t]["height"])
        assert (float(d["uscale"]), float(d["vscale"]), float(d["uoffs"]), float(d["voffs"])) == (2.0, 0.5, 0.25, -1.0)
        assert int(d["addr"]) == (0 if faithful else t)
    assert mats[0]["map"][8]["width"] == 0 and mats[3]["map"][7]["width"] == 0
    if faithful:
        # the reference's packer: roughness, then specularity write texaddr0 (material_list.cpp:441-460); the alpha mask writes none
        assert int(mats[0]["map"][0]["addr"]) == 2 and int(mats[1]["map"][0]["addr"]) == 2 and int(mats[2]["map"][0]["addr"]) == 0
    else:
        assert int(mats[0]["map"][0]["addr"]) == 0


def _png(rgba):
    """An 8-bit RGBA PNG of the array (h, w, 4), filter 0 on every row."""
    h, w, _ = rgba.shape
    def chunk(kind, data):
        body = kind + data
        return len(data).to_bytes(4, "big") + body + (zlib.crc32(body) & 0xFFFFFFFF).to_bytes(4, "big")
    raw = b"".join(b"\x00" + rgba[y].tobytes() for y in range(h))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([8, 6, 0, 0, 0])) +
            chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def test_gltf_metallic_roughness_texture_and_alpha_mask(pkg, tmp_path):
    rng = np.random.default_rng(12)
    (tmp_path / "mr.png").write_bytes(_png(rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)))
    (tmp_path / "base.png").write_bytes(_png(rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)))
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
    uv = np.array([[0, 0], [1, 0], [0, 1]], f32)
    blob = pos.tobytes() + uv.tobytes()
    doc = {
        "asset": {"version": "2.0"}, "scenes": [{"nodes": [0, 1]}], "nodes": [{"mesh": 0}, {"mesh": 1}],
        "buffers": [{"uri": "data:application/octet-stream;base64," + base64.b64encode(blob).decode(), "byteLength": len(blob)}],
        "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 36}, {"buffer": 0, "byteOffset": 36, "byteLength": 24}],
        "accessors": [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3"},
                      {"bufferView": 1, "componentType": 5126, "count": 3, "type": "VEC2"}],
        "images": [{"uri": "base.png"}, {"uri": "mr.png"}], "textures": [{"source": 0}, {"source": 1}],
        "materials": [{"alphaMode": "MASK", "pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicRoughnessTexture": {"index": 1},
                                                                     "metallicFactor": 0.5, "roughnessFactor": 0.75}},
                      {"alphaMode": "BLEND", "pbrMetallicRoughness": {"baseColorFactor": [0.2, 0.3, 0.4, 1.0]}}],
        "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "TEXCOORD_0": 1}, "material": 0}]},
                   {"primitives": [{"attributes": {"POSITION": 0, "TEXCOORD_0": 1}, "material": 1}]}],
    }
    (tmp_path / "m.gltf").write_text(json.dumps(doc))
    s, g, _ = pkg.gltf.load_scene(str(tmp_path / "m.gltf"), load_images=True)
    m, plain = s.host_materials
    assert m["alpha"] is True and plain["alpha"] is False
    assert m["roughnessmap"] == m["metallicmap"] and m["roughnessmap"] >= 0 and m["roughnessmap"] != m["texture"] and m["texture"] >= 0
    assert plain["roughnessmap"] == plain["metallicmap"] == plain["alphamap"] == -1 and m["alphamap"] == -1
    assert (m["roughness"], m["metallic"]) == (0.75, 0.5)
    src = s.textures[m["roughnessmap"]]
    lin = pkg.abi.TEXSRC_LINEARIZE_REFERENCE | pkg.abi.TEXSRC_LINEARIZE_SRGB
    assert src["flags"] & lin == 0 and s.textures[m["texture"]]["flags"] & lin == pkg.abi.TEXSRC_LINEARIZE_SRGB  # a data texture
    mats, ids = pkg.scenes.pack_materials(s.host_materials, s.textures)
    fl = int(mats[0]["flags"])
    assert (fl >> 4) & 1 and (fl >> 5) & 1 and (fl >> 12) & 1 and not (fl >> 13) & 1
    assert int(mats[0]["map"][6]["addr"]) == int(mats[0]["map"][7]["addr"]) == m["roughnessmap"]
    # without load_images the file's textures are not read, the alpha mode still is
    s2, _, _ = pkg.gltf.load_scene(str(tmp_path / "m.gltf"))
    assert s2.host_materials[0]["roughnessmap"] == -1 and s2.host_materials[0]["alpha"] is True and not s2.textures


def test_obj_map_d_becomes_the_alpha_mask(pkg, tmp_path):
    rng = np.random.default_rng(13)
    (tmp_path / "mask.png").write_bytes(_png(rng.integers(0, 256, (4, 4, 4), dtype=np.uint8)))
    (tmp_path / "kd.png").write_bytes(_png(rng.integers(0, 256, (4, 4, 4), dtype=np.uint8)))
    (tmp_path / "q.mtl").write_text("newmtl leaf\nKd 1 1 1\nmap_Kd kd.png\nmap_d mask.png\n\nnewmtl bark\nKd 0.4 0.3 0.2\n")
    (tmp_path / "q.obj").write_text("mtllib q.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvt 1 1\n"
                                    "usemtl leaf\nf 1/1 2/2 3/3\nusemtl bark\nf 2/2 4/4 3/3\n")
    s, materials, _ = pkg.obj.load_scene(str(tmp_path / "q.obj"), load_images=True)
    assert materials[0][1]["map_d"] == "mask.png" and materials[1][1]["map_d"] is None
    leaf, bark = s.host_materials
    assert leaf["alphamap"] >= 0 and leaf["texture"] >= 0 and leaf["alphamap"] != leaf["texture"] and bark["alphamap"] == -1
    lin = pkg.abi.TEXSRC_LINEARIZE_REFERENCE | pkg.abi.TEXSRC_LINEARIZE_SRGB
    assert s.textures[leaf["alphamap"]]["flags"] & lin == 0 and s.textures[leaf["alphamap"]]["flags"] & pkg.abi.TEXSRC_FLIP_ROWS
    mats, ids = pkg.scenes.pack_materials(s.host_materials, s.textures)
    assert (int(mats[0]["flags"]) >> 13) & 1 and int(mats[0]["map"][9]["addr"]) == leaf["alphamap"]
    assert ids.view(np.int32).reshape(-1, 11)[0, 10] == leaf["alphamap"]
    s2, _, _ = pkg.obj.load_scene(str(tmp_path / "q.obj"))
    assert s2.host_materials[0]["alphamap"] == -1


# ----------------------------------------------------------------------------------------------------------------------
# 4. plugin
# ----------------------------------------------------------------------------------------------------------------------
PLUGIN_VARS = ("RFWHIP_MATERIAL_MAPS", "RFWHIP_DISPLAY", "RFWHIP_INTEGRATOR", "RFWHIP_DEVICES", "RFWHIP_DEVICE", "RFWHIP_TRANSPORT",
               "RFWHIP_FRAMES_IN_FLIGHT", "RFWHIP_NOISE", "RFWHIP_BLOOM", "RFWHIP_GRADE", "RFWHIP_EXPOSURE", "RFWHIP_SKY_HDR", "RFWHIP_SKY_TABLE")


def _check_plugin(host, tmp_path):
    out = {}
    for name, env in (("on", {"RFWHIP_MATERIAL_MAPS": "1"}), ("off", {}), ("zero", {"RFWHIP_MATERIAL_MAPS": "0"})):
        d = tmp_path / name
        d.mkdir()
        r = run_host(host, d, drop=PLUGIN_VARS, **env)
        assert r.returncode == 0, (name, r.returncode, r.stdout, r.stderr)
        on = 1 if name == "on" else 0
        assert r.stdout == "material_maps %d\nmaterial_maps_on %d\nequal 1\n" % (on, on), (name, r.stdout, r.stderr)
        out[name] = (d / "plugin.rgba32f").read_bytes()
        assert len(out[name]) == 96 * 64 * 16
    assert out["off"] == out["zero"] and out["on"] != out["off"]  # (the mask is seen through)
    r = run_host(host, tmp_path, drop=PLUGIN_VARS, RFWHIP_MATERIAL_MAPS="yes")
    assert r.returncode == 5 and r.stderr == 'exception: HipRT: RFWHIP_MATERIAL_MAPS must be "0" or "1"\n', (r.returncode, r.stderr)


def test_plugin_environment_variable(pkg, tmp_path, tmp_path_factory):
    """tests/plugin/maps_host.cpp behind HipRT.cpp built against the host-emulation library (as tests/test_plugin_env.py builds it)."""
    import build_emu
    emu = build_emu.build()
    plugin_dir = tmp_path_factory.mktemp("emu_plugin_maps")
    lib = str(plugin_dir / "librfwhip_emu.so")
    os.symlink(emu, lib)
    csrc = os.path.join(ROOT, "rendering-fw_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(csrc, "plugin"), os.path.join(csrc, "plugin", "HipRT.cpp"), "-o", str(plugin_dir / "HipRT.so"),
                        lib, "-Wl,-rpath," + os.path.dirname(emu)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    _check_plugin(build_host(pkg, tmp_path_factory, "maps_host", lib=lib), tmp_path)


@pytest.mark.gpu
def test_plugin_environment_variable_gpu(pkg, tmp_path, tmp_path_factory):
    _check_plugin(build_host(pkg, tmp_path_factory, "maps_host"), tmp_path)
