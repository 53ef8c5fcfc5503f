"""The rule of the setting material_maps (include/rfwhip.h) in numpy, for tests/test_material_maps*.py, and
the scenes those tests render.  Nothing here reads rt_core.h's arithmetic: the fetches are the numpy restatement of
getShadingData.h in tests/golden/make_golden_pt.py (fetch_trilinear, texels64), as tests/test_texture_fetch.py uses it, and the
allowance of a fetch is the one that file derives for `surface_layers` (its docstring, "SURFACE LAYERS"), restated per slot:

    dt_K = 18 u M_K + R_K (d_tcx + d_tcy + d_lambda [+ 1 where lambda's window holds 0])

is the deviation of ONE legal evaluation of RT_LAYER(K) from exact arithmetic (u = 2^-24, M_K the largest |channel| of the texture,
R_K its largest channel range); the model's own float32 fetch is one legal evaluation, so an implementation's texel lies within
2 dt_K of it.  Carried through the product: with c = chan(p0, shift) = P / 255 and the model's texel channel x,

    v in [c (x - 2 dt) - e, c (x + 2 dt) + e],   e = 8 u max(1, |x|)

(e: the rounding of 1 / 255, of the product, of the multiplication by 255 and of the addition of 0.5, each below 2 u max(1, |x|)),
and byte() is monotone, so the accepted bytes are byte(lo) .. byte(hi).  a = min(x, w) moves by at most 2 dt as well.
"""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_pt as model  # noqa: E402

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
C_TRILINEAR = 18
BIT_METALLIC, BIT_ROUGHNESS, BIT_MASK = 4, 5, 13


def byte(v):
    """byte(v) = (uint32)(fmin(fmax(v, 0), 1) * 255 + 0.5); a NaN gives 0."""
    v = np.asarray(v, f64)
    return np.floor(np.clip(np.where(np.isnan(v), 0.0, v), 0.0, 1.0) * 255.0 + 0.5).astype(np.int64)


def _ulp(x):
    x = np.abs(np.asarray(x, f64)).astype(f32)
    return (np.nextafter(x, f32(np.inf)) - x).astype(f64)


def model_texture(pkg, t):
    f4t = int(t["type"]) == pkg.abi.TEX_FLOAT4
    return dict(float4=f4t, data=np.asarray(t["data"], f32).reshape(-1, 4) if f4t else np.asarray(t["data"], np.uint32))


def hit_records(scene, n, seed, spread, min_cos=0.05):
    """n random hits over the scene's instances and triangles: barycentrics, a direction with |D.N| >= min_cos against the
    triangle's normal (the instances of these scenes carry the identity), t over four decades."""
    rng = np.random.default_rng(seed)
    inst = rng.integers(0, len(scene.instances), n)
    ntri = np.array([len(scene.meshes[i["mesh"]]["triangles"]) for i in scene.instances])
    prim = (rng.random(n) * ntri[inst]).astype(np.int64)
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    bu, bv = (r1 * (1 - r2)).astype(f32), (r1 * r2).astype(f32)
    over = (f32(1) - bu - bv) < 0
    bu[over] *= f32(0.5)
    bv[over] *= f32(0.5)
    N = np.zeros((n, 3))
    for ii, i in enumerate(scene.instances):
        assert np.array_equal(i["transform"], np.eye(4))
        tr = scene.meshes[i["mesh"]]["triangles"]
        sel = inst == ii
        N[sel] = np.stack([tr["Nx"], tr["Ny"], tr["Nz"]], -1)[prim[sel]]
    D = rng.normal(size=(n, 3))
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    low = np.abs((D * N).sum(-1)) < min_cos
    D[low] = (D[low] + N[low] * np.sign((D[low] * N[low]).sum(-1) + 1e-30)[:, None] * 0.5)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    t = (10.0 ** rng.uniform(-2, 2, n)).astype(f32)
    rec = np.zeros((n, 24), f32)
    ri = rec.view(np.uint32)
    ri[:, 0], ri[:, 1] = inst, prim
    rec[:, 2], rec[:, 3], rec[:, 4:7], rec[:, 7], rec[:, 8] = bu, bv, D.astype(f32), t, spread
    return rec


def evaluate(pkg, scene, mats, rec):
    """The rule on the records of `hit_records`, for the packed materials `mats` as they are uploaded (addresses resolved).
    Returns per record: present (n, 3 bool: slots 6, 7, 9), P (n, 2: the material's roughness and metallic bytes), x (n, 3: the
    texel channel each slot reads — green of 7, blue of 6, min(red, alpha) of 9 — NaN-free or NaN), dt (n, 3: its allowance 2 dt)."""
    n = len(rec)
    ri = rec.view(np.uint32)
    inst, prim = ri[:, 0].astype(np.int64), ri[:, 1].astype(np.int64)
    bw1, bw2 = rec[:, 2], rec[:, 3]
    bw0 = (f32(1) - bw1 - bw2).astype(f32)
    D, t, spread = rec[:, 4:7], rec[:, 7], rec[:, 8]
    texu, texv, lod = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n, f32)
    N, matid = np.zeros((n, 3), f32), np.zeros(n, np.int64)
    for ii, i in enumerate(scene.instances):
        tr = scene.meshes[i["mesh"]]["triangles"]
        sel = inst == ii
        q = tr[prim[sel]]
        texu[sel], texv[sel], lod[sel], matid[sel] = q["u"], q["v"], q["LOD"], q["material"]
        N[sel] = model.normalize(np.stack([q["Nx"], q["Ny"], q["Nz"]], -1).astype(f32))
    tu = ((bw0 * texu[:, 0] + bw1 * texu[:, 1]) + bw2 * texu[:, 2]).astype(f32)
    tv = ((bw0 * texv[:, 0] + bw1 * texv[:, 1]) + bw2 * texv[:, 2]).astype(f32)
    d = np.abs(model.dot(-D, N))
    lam = (lod + np.log2((spread * t).astype(f32) * (f32(1) / d)).astype(f32)).astype(f32)
    # the allowance of lambda and of the texel coordinates (tests/test_texture_fetch.py, _layer_bounds; identity instances:
    # kappa = sum |n_j| / |n| <= sqrt(3), doubled there for smooth normals — kept)
    eps_n = (3 * 2 * np.sqrt(3.0) + 6) * U
    dd = 3 * U + np.sqrt(3) * eps_n
    L = lam.astype(f64) - lod
    dlam = (dd / d.astype(f64) + 3 * U) / np.log(2) + 4 * U * np.maximum(np.abs(L), 1) + 2 * U * np.abs(lam.astype(f64))
    at_zero = np.abs(lam) <= 2 * dlam
    uvmax, vvmax = np.abs(texu).max(-1).astype(f64), np.abs(texv).max(-1).astype(f64)
    textures = [model_texture(pkg, tx) for tx in scene.textures]
    present = np.zeros((n, 3), bool)
    x, dt = np.ones((n, 3)), np.zeros((n, 3))
    P = np.zeros((n, 2), np.int64)
    for mi in np.unique(matid):
        sel = np.nonzero(matid == mi)[0]
        m = mats[mi]
        fl, p0 = int(m["flags"]), int(m["parameters"][0])
        P[sel, 0], P[sel, 1] = p0 >> 24, p0 & 255
        for col, (slot, bit, chan) in enumerate(((6, BIT_METALLIC, 2), (7, BIT_ROUGHNESS, 1), (9, BIT_MASK, None))):
            desc = m["map"][slot]
            if not (fl >> bit) & 1 or int(desc["addr"]) >= len(textures):
                continue
            present[sel, col] = True
            tex = textures[int(desc["addr"])]
            t64 = model.texels64(tex, np.arange(len(tex["data"])))
            us, vs, uo, vo = (f32(desc[k]) for k in ("uscale", "vscale", "uoffs", "voffs"))
            w, h = int(desc["width"]), int(desc["height"])
            if np.isnan(t64).any():
                # (a FLOAT4 map of at most 2 x 2 texels, one of them NaN in every channel: every footprint holds it)
                assert tex["float4"] and len(t64) <= 4 and w <= 2 and h <= 2 and np.isnan(t64).all(-1).any()
                x[sel, col] = np.nan
                continue
            Mk, Rk = np.abs(t64).max(), (t64.max(0) - t64.min(0)).max()
            if Rk == 0.0:  # a constant map: every fetch is the constant, whatever the descriptor says (width 0 included)
                texel = np.tile(t64[:1], (len(sel), 1))
                dt[sel, col] = 2 * C_TRILINEAR * U * Mk
            else:
                xs, ys = (us * (uo + tu[sel])).astype(f32), (vs * (vo + tv[sel])).astype(f32)
                texel = model.fetch_trilinear(tex, lam[sel], xs, ys, w, h).astype(f64)
                ax, ay = np.abs(xs.astype(f64)), np.abs(ys.astype(f64))
                aus, avs, auo, avo = abs(float(us)), abs(float(vs)), abs(float(uo)), abs(float(vo))
                dx = aus * (5 * U * uvmax[sel] + U * (auo + np.abs(tu[sel].astype(f64)))) + U * ax
                dy = avs * (5 * U * vvmax[sel] + U * (avo + np.abs(tv[sel].astype(f64)))) + U * ay
                dtc = (_ulp(ax + 1000) + dx) * w + _ulp((ax + 1000) * w) + (_ulp(ay + 1000) + dy) * h + _ulp((ay + 1000) * h)
                dt[sel, col] = 2 * (C_TRILINEAR * U * Mk + Rk * (dtc + dlam[sel] + at_zero[sel]))
            x[sel, col] = np.minimum(texel[:, 0], texel[:, 3]) if chan is None else texel[:, chan]
    return present, P, x, dt


def accepted_bytes(P, x, dt):
    """(lo, hi) of the bytes the rule allows for parameter bytes P, texel channels x and allowances dt (arrays of one shape)."""
    c = P.astype(f64) / 255.0
    e = 8 * U * np.maximum(1.0, np.abs(np.where(np.isnan(x), 0.0, x)))
    return byte(c * (x - dt) - e), byte(c * (x + dt) + e)


def check_surface_maps(got, present, P, x, dt, who):
    """Holds the output records of `surface_maps` against evaluate()'s.  Returns (records, records whose mask decision was free)."""
    gi = got.view(np.uint32)
    flags = gi[:, 3]
    assert not got[:, 4:].any(), who
    for col, bit in enumerate((1, 2, 3)):
        assert np.array_equal(((flags >> bit) & 1).astype(bool), present[:, col]), (who, "presence bit", bit)
    assert not (flags >> 4).any(), who
    # the mask
    a = got[:, 2].astype(f64)
    assert np.all(a[~present[:, 2]] == 1.0), who
    assert np.all(np.abs(a - x[:, 2])[present[:, 2]] <= dt[:, 2][present[:, 2]]), (who, "a", np.abs(a - x[:, 2])[present[:, 2]].max())
    skip = (flags & 1).astype(bool)
    want_skip = present[:, 2] & (x[:, 2] < 0.5)
    free = present[:, 2] & (np.abs(x[:, 2] - 0.5) <= dt[:, 2])
    assert np.array_equal(skip[~free], want_skip[~free]), (who, "pass-through bit")
    assert np.array_equal(skip, present[:, 2] & (got[:, 2] < f32(0.5))), who  # (the bit is the record's own a < 0.5)
    # the two bytes: a hit the mask passes through keeps the material's
    for col, out in ((1, 0), (0, 1)):  # (roughness: slot 7 -> out[0]; metallic: slot 6 -> out[1])
        mapped = present[:, col] & ~skip
        lo, hi = accepted_bytes(P[:, out], x[:, col], dt[:, col])
        g = gi[:, out].astype(np.int64)
        assert np.array_equal(g[~mapped], P[~mapped, out]), (who, "unmapped byte", out)
        bad = mapped & ((g < lo) | (g > hi))
        assert not bad.any(), (who, "byte", out, int(bad.sum()), g[bad][:5], lo[bad][:5], hi[bad][:5])
    return len(got), int(free.sum())


# ----------------------------------------------------------------------------------------------------------------------
# scenes
# ----------------------------------------------------------------------------------------------------------------------
def constant_rgba8(pkg, rgba, w=4, h=4):
    return pkg.scenes.make_texture_rgba8(np.tile(np.asarray(rgba, np.uint8), (h, w, 1)))


def param(b):
    """A host parameter that packs to byte b (TOCHAR truncates)."""
    return (int(b) + 0.5) / 255.0


def triangle_zoo(pkg, materials, uv_seed=5):
    """One mesh of len(materials) triangles, triangle k with material k, random uvs in [-2, 3], LODs from -1 to 3; identity instance."""
    rng = np.random.default_rng(uv_seed)
    s = pkg.scenes.Scene()
    n = len(materials)
    v = np.zeros((3 * n, 3), f32)
    for k in range(n):
        v[3 * k:3 * k + 3] = np.array([[0, 0, 0], [1, 0, 0.2], [0.1, 1, 0.1]], f32) + rng.uniform(-0.2, 0.2, (3, 3)).astype(f32) + (2.0 * k, 0, 0)
    uv = rng.uniform(-2.0, 3.0, (3 * n, 2)).astype(f32)
    return s, v, uv, rng


def finish_zoo(s, v, uv, rng, material_ids):
    mesh = s.add_mesh(v, None, uvs=uv, material=0)
    tr = s.meshes[mesh]["triangles"]
    tr["material"][:] = np.asarray(material_ids, np.uint32)
    tr["LOD"][:] = rng.uniform(-1.0, 3.0, len(tr)).astype(f32)
    s.add_instance(mesh)
    return s


def upload_with(c, scene, mats, ids):
    """scene.upload with the given packed materials in place of the scene's own packing."""
    c.init(64, 48)
    scene.upload(c)
    c.set_materials(mats, ids)
    c.update()
    return c


def room(pkg, W=96, H=64):
    """A small lit room for the image tests: the Cornell box's walls and boxes (scenes.cornell) with its point light."""
    return pkg.scenes.cornell(W, H, geometric_emitter=True)


def add_card(scene, material, centre=(0.0, 5.0, -3.0), size=5.0):
    """A card of the given size facing the camera of scenes.cornell (normal -z), uv 0..2 across it."""
    x0, y0, z = centre[0] - size / 2, centre[1] - size / 2, centre[2]
    v = np.array([[x0, y0, z], [x0 + size, y0, z], [x0 + size, y0 + size, z], [x0, y0 + size, z]], f32)
    uv = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], f32)
    mesh = scene.add_mesh(v, np.array([[0, 2, 1], [0, 3, 2]], np.uint32), uvs=uv, material=material)
    scene.add_instance(mesh)
    return mesh


def mask_image(seed=3, n=16):
    """An n x n mask: 4 x 4 cells of 0 / 255 with a grey ramp across two of them (values on both sides of 128)."""
    rng = np.random.default_rng(seed)
    m = np.kron(rng.integers(0, 2, (n // 4, n // 4)), np.ones((4, 4))).astype(np.int64) * 255
    m[0:4, :] = np.linspace(20, 235, n).astype(np.int64)[None, :]
    return m.astype(np.uint8)


def render(c, scene, settings, W=96, H=64, upload=None):
    c.init(W, H)
    (upload or scene.upload)(c)
    for k, v in dict({"integrator": "pt", "spp": 4, "max_depth": 2}, **settings).items():
        c.set_setting(k, v)
    c.render_frame(scene.camera, 0)
    st = c.get_stats()
    return c.framebuffer(), (st.primaryCount, st.secondaryCount, st.deepCount, st.shadowCount)
