"""Known answers for the texture sampler of the path tracer (rt_core.h: load_texel, tex_wrap, fetch_texel, fetch_trilinear,
pt_surface, pt_textures), through rfwhip_kat's `tex_fetch` and `surface_layers` on the C oracle, the host emulation and the HIP
kernels, against the numpy restatement of getShadingData.h in tests/golden/make_golden_pt.py and a float64 evaluation of the same
sums (texel_coordinate, fetch_texel64, trilinear_levels there).

THE MIP CHAIN.  test_integer_level_is_the_uploaded_level_image states what the chain walk owes the front end: for a texture laid out
as scenes.make_texture_rgba8 lays it out — five levels of sides max(1, side // 2) — fetch_trilinear at an integer level L returns
the bilinear fetch of the L-th level image that was uploaded.  It is held on the texture set below (every level's texels
independent) and on textures the helper itself builds from random images.  With the walk `w >>= 1, h >>= 1` of the commits before
this file it fails for every map one of whose sides reaches 0 before the last level — 1 x 1, 2 x 2, 3 x 5, 5 x 3, 16 x 2, 2 x 16,
64 x 1, 1 x 64, 8192 x 2, at the levels behind that one: from there on the offsets stop advancing (64 x 1: 0, 64, 64, 64, 64 against the helper's 0, 64, 96, 112, 120).  (The
helper of those commits did not filter a level along a side of 1 but cropped it, so each of its thin levels was a prefix of the one
before and the wrong offset happened to read equal texels: test_helper_levels_are_box_filtered.)

THE FETCH BOUND.  u = 2^-24 is the unit roundoff of float32, M the largest |channel| of the texture's texels.  Given the texel
coordinates tcx, tcy (below), fetch_texel computes, per channel, 0 + p0 w0 + p1 w1 + p2 w2 + p3 w3 with
    fu = tcx - floor(tcx), fv likewise            exact for tcx >= 1; for tcx in (-0.5, 1) one rounding, |d fu| <= u
    1 - fu, 1 - fv                                exact, or one rounding each
    w0 = (1-fu)(1-fv), w1 = fu(1-fv), w2 = (1-fu)fv   a product of two factors of at most one rounding each: |d w_i| <= 3 u w_i
    w3 = 1 - ((w0 + w1) + w2)                     inherits 3u (w0+w1+w2) <= 3u, two sums and one difference of values <= 1: |d w3| <= 6u
so sum_i |p_i| |d w_i| <= M (3u + 6u) = 9uM; the four products round once each (or are fused), sum_i u |p_i w_i| <= uM; the three
sums of partial results that are at most M round once each, 3uM; adding to 0, the decode of an RGBA8 texel (an integer below 256
times 2^-8) and the load of a FLOAT4 texel are exact.  c_bilinear = 9 + 1 + 3 = 13.  fetch_trilinear blends two such fetches,
(1-f) p0 + f p1 with f = lambda - floor(lambda) (at most one rounding, as is 1-f: |d f| <= u, |d(1-f)| <= 2u): the fetches bring
((1-f) + f) 13uM, the weights 3uM, the two products uM between them, the sum uM.  c_trilinear = 13 + 3 + 1 + 1 = 18.  The bounds
are c u M; they were written down before any implementation was run against them.

THE COORDINATE.  tc = (max(t + 1000, 0) * side) - 0.5 is where a legal rounding changes a DISCRETE decision (which texels, and at
texture sizes of a few hundred texels and beyond, weights quantised to 1/32 and coarser: 1000 * 512 has an ulp of 2^-5).  A compiler
may contract the product and the difference into one fused multiply-add or not, per axis and — the function is inlined — per
call: four candidate coordinate pairs per level, sixteen blends per trilinear fetch.  An implementation's record passes when it
lies within the bound of ONE candidate (all four channels of the same one).  lambda is an input here, so the level pair and f are
exact; note that the reference takes level0 = (int)lambda and f = lambda - floor(lambda), so lambda in (-1, 0) blends levels 0
and 1 with f = lambda + 1, and the fetch is NOT continuous at lambda = 0 — the grid holds -1e-6, 0 and 1e-6.

THE INPUTS reach up to the largest coordinates with (t + 1000) * side < 2^31.  Beyond that `(int)tc` is undefined in the
reference and on the host (the device saturates); such coordinates are not part of the test.

SURFACE LAYERS.  Between two legal evaluations of pt_surface / pt_textures the following differ (each figure is the deviation of ONE
evaluation from exact arithmetic; two evaluations differ by at most twice that, which is what the test allows — B2 = 2B):
  * tu = bw0 u0 + bw1 u1 + bw2 u2 (weights in [0, 1], three products, two sums, contractable): <= 5u max|u_i|; the layer's
    x = uscale (uoffs + tu): <= |uscale| (5u max|u_i| + u |uoffs + tu|) + u |x| =: dx.  a = x + 1000 is rounded to float32, so two
    evaluations' a differ by at most one ulp(a) + dx, and tc by at most d_tc = (ulp(a) + dx) side + ulp(a side) texels.  The bilinear
    interpolant is continuous and piecewise bilinear in tc with slope at most R per texel and axis (R = the largest channel range
    of the texture's texels), so the fetch moves by at most R (d_tcx + d_tcy).
  * N = normalize(M n): |d N| <= eps_N = (3 kappa + 6) u per component, kappa = max_i sum_j |M_ij n_j| / |M n| of the instance
    (three roundings per term of the matrix product; the dot product, the reciprocal root — v_rsq_f32 / 1 / sqrt: 1 ulp — and the
    scaling of the normalisation, 6u).  d = D.N: <= 3u + sqrt(3) eps_N =: dd.  lambda = LOD + log2(spread t * rcp|d|): the
    reciprocal (v_rcp_f32: 1 ulp; the host's division: half an ulp) and the product 3u relative, the logarithm (v_log_f32: 1 ulp;
    log2f: 1 ulp) 2u max(|L|, 1) each side, the sum u |lambda|:  d_lambda <= (dd / |d| + 3u) / ln 2 + 4u max(|L|, 1) + 2u |lambda|.
    The trilinear blend is continuous and piecewise linear in lambda with slope |p1 - p0| <= R — across the integers too, so the
    level pair may fall either way there at no extra allowance — EXCEPT at lambda = 0 (above): a record whose
    [lambda - 2 d_lambda, lambda + 2 d_lambda] holds 0 is allowed R more.
  * a colour layer k: dt_k = 18 u M_k + R_k (d_tcx + d_tcy + d_lambda); a normal-map layer: dn_k = 13 u M_k + R_k (d_tcx + d_tcy).
  * colour = ((c t0 + t1 + t2) t0), six roundings:
        B_colour = (|c| dt0 + dt1 + dt2)(M0 + dt0) + (|c| M0 + M1 + M2) dt0 + 6u (|c| M0 + M1 + M2) M0.
  * normal: sn = sum_k 2 (p_k - 0.5): d sn <= 2 sum dn_k + 18u; the zoo's and the cards' normal maps keep every layer's z at or above
    ZMIN, so |sn| >= 2 (ZMIN - 0.5) layers =: smin and the unit vector moves by <= 2 d sn / smin + 6u =: ds.  The tangent frame
    (tools.h:204-211, -1 / (sign + N.z): conditioned by |sign + N.z| >= 1; the zoo keeps |N.z| away from 0, where the frame
    flips) moves by eps_F = 8 eps_N.  iN' = normalize(T sx + B sy + iN sz):  B_normal = 2 (sqrt(3) (eps_F + ds) + 5u) + 6u; without a
    normal map B_normal = eps_N.
  * the alpha flag is a comparison of t0.w with 0.5: it may differ where |t0.w - 0.5| <= 2 dt0, and the record is then held against
    the branch the implementation took.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_pt as model  # noqa: E402  (the numpy restatement; importing it generates nothing)

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
C_BILINEAR, C_TRILINEAR = 13, 18
ZMIN = 0.8125  # smallest z channel of a normal-map texel in this file's scenes (208 / 256)
STRICT_FLAGS = ("-DRT_STRICT_MATH", "-ffp-contract=off")

CHAINED = [(1, 1), (2, 2), (3, 5), (5, 3), (8, 8), (16, 2), (2, 16), (64, 1), (1, 64), (48, 20), (64, 64), (100, 36), (512, 256)]
PLAIN = [(4, 4), (64, 64), (7, 9)]
FLOAT4 = [(1, 1), (16, 16), (13, 6)]
WIDE = (8192, 2)  # 1000 * 8192 > 2^22: the plain-remainder side of the device's tex_wrap
LAMBDAS = np.array([-3, -1, -0.999, -0.5, -1e-6, 0, 1e-6, 0.5] + [k + d for k in range(1, 7) for d in (-2.0 ** -20, 0.0, 2.0 ** -20)] +
                   [3.999, 100], f32)


# ----------------------------------------------------------------------------------------------------------------------
# the texture set
# ----------------------------------------------------------------------------------------------------------------------
def helper_level_shapes(w, h):
    """What scenes.make_texture_rgba8 appends: five levels of sides max(1, side // 2)."""
    out = []
    for _ in range(5):
        out.append((w, h))
        w, h = max(1, w // 2), max(1, h // 2)
    return out


def _rgba8(pkg, rng, w, h, chain):
    n = sum(a * b for a, b in helper_level_shapes(w, h)) if chain else w * h
    b = rng.integers(8, 248, size=(n, 4), dtype=np.uint32)  # (the sentinels hold the bytes 0 and 255)
    return {"type": pkg.abi.TEX_UINT, "width": w, "height": h, "data": (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)).astype(np.uint32)}


def _float4(pkg, rng, w, h):
    return {"type": pkg.abi.TEX_FLOAT4, "width": w, "height": h, "data": rng.uniform(-3.0, 5.0, size=(w * h * 4)).astype(f32)}


def _sentinel(pkg, like):
    if like["type"] == pkg.abi.TEX_UINT:
        return {"type": pkg.abi.TEX_UINT, "width": 8, "height": 8, "data": np.tile(np.array([0xFF00FF00, 0x00FF00FF], np.uint32), 32)}
    return {"type": pkg.abi.TEX_FLOAT4, "width": 8, "height": 8, "data": np.tile(np.array([1e6, -1e6], f32), 128)}


def _model_texture(pkg, t):
    f4t = int(t["type"]) == pkg.abi.TEX_FLOAT4
    return dict(float4=f4t, data=np.asarray(t["data"], f32).reshape(-1, 4) if f4t else np.asarray(t["data"], np.uint32))


def _texels(mt):
    return model.texels64(mt, np.arange(len(mt["data"])))


def _card_scene(pkg, textures):
    """The textures and one untextured card (the functions run on the scene of an update)."""
    s = pkg.scenes.Scene()
    for t in textures:
        s.add_texture(t)
    m = s.add_material(color=(0.5, 0.5, 0.5))
    mesh = s.add_mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32), np.array([[0, 1, 2]], np.uint32), material=m)
    s.add_instance(mesh)
    return s


def _texture_set(pkg):
    """[(name, texture index in the scene, model texture, [(descriptor width, height), ...])] and the scene: every texture is
    followed in its pool by a sentinel texture whose values no texel of the set has."""
    rng = np.random.default_rng(20261017)
    entries = []
    for w, h in CHAINED:
        entries.append(("rgba8 %dx%d chain" % (w, h), _rgba8(pkg, rng, w, h, True), [(w, h)]))
    for w, h in PLAIN:
        entries.append(("rgba8 %dx%d plain" % (w, h), _rgba8(pkg, rng, w, h, False), [(w, h)]))
    for w, h in FLOAT4:
        entries.append(("float4 %dx%d" % (w, h), _float4(pkg, rng, w, h), [(w, h)]))
    entries.append(("rgba8 %dx%d chain" % WIDE, _rgba8(pkg, rng, WIDE[0], WIDE[1], True), [WIDE]))
    # descriptors that disagree with the texture: larger ones drive indices into load_texel's clamp (the chain of a larger descriptor
    # always needs more texels than the texture has, so those are read at level 0), a smaller one walks its own, shorter chain
    entries.append(("rgba8 64x64 chain, other descriptors", _rgba8(pkg, rng, 64, 64, True), [(100, 80), (80, 50), (32, 32), (64, 128)]))
    entries.append(("rgba8 7x9 plain, other descriptors", _rgba8(pkg, rng, 7, 9, False), [(9, 7), (16, 16)]))
    entries.append(("float4 13x6, other descriptors", _float4(pkg, rng, 13, 6), [(6, 13), (20, 10)]))
    textures, out = [], []
    for name, t, descs in entries:
        out.append((name, len(textures), _model_texture(pkg, t), descs))
        textures += [t, _sentinel(pkg, t)]
    return out, _card_scene(pkg, textures)


# ----------------------------------------------------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------------------------------------------------
def _neighbours(x):
    x = np.asarray(x, f32)
    return np.concatenate([np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))])


def _largest(side):
    """The largest float32 t with (t + 1000) * side <= 2^31 - 256 (so that tc, rounded either way, stays below 2^31 - 128)."""
    x = f32((2.0 ** 31 - 256) / side - 1000.0)
    while f64(f32(x + f32(1000))) * side > 2.0 ** 31 - 256:
        x = np.nextafter(x, f32(-np.inf))
    return x


def _axis_values(side, rng):
    v = [rng.uniform(-4.0, 4.0, 48).astype(f32),
         np.array([-1000.0, -1001.0, -1e6, 0.0, 1.0], f32), _neighbours([-1000.0]), np.nextafter(f32(1), f32(0)).reshape(1)]
    if side <= 64:  # every texel border and centre, and their float32 neighbours
        k = np.arange(side + 1, dtype=f64)
        v += [_neighbours((k / side).astype(f32)), _neighbours(((k + 0.5) / side).astype(f32))]
    for edge in (2.0 ** 22, 2.0 ** 23):  # (t + 1000) * side within +-2 of the edge
        v.append(((edge + np.array([-2, -1, -0.5, 0, 0.5, 1, 2])) / side - 1000.0).astype(f32))
    big = _largest(side)
    v.append(np.array([big, np.nextafter(big, f32(-np.inf)), f32(0.5) * big], f32))
    return np.concatenate(v).astype(f32)


def _coordinates(w, h, seed):
    """Pairs (tu, tv): every value of either axis' list appears, paired with a value of the other's in a fixed shuffle."""
    rng = np.random.default_rng(seed)
    a, b = _axis_values(w, rng), _axis_values(h, rng)
    n = max(len(a), len(b))
    a, b = np.resize(a, n), np.resize(b, n)
    return a, b[rng.permutation(n)]


def _records(ti, w, h, seed):
    tu, tv = _coordinates(w, h, seed)
    lam, form, k = np.meshgrid(LAMBDAS, np.array([0, 1], np.uint32), np.arange(len(tu)), indexing="ij")
    lam, form, k = lam.reshape(-1), form.reshape(-1), k.reshape(-1)
    rec = np.zeros((len(k), 24), f32)
    ri = rec.view(np.uint32)
    ri[:, 0], ri[:, 1], ri[:, 5], ri[:, 6] = ti, form, w, h
    rec[:, 2], rec[:, 3], rec[:, 4] = lam, tu[k], tv[k]
    return rec


def _all_records(tset):
    """One array of records for the whole set, with the slices of its (texture, descriptor) blocks."""
    blocks, recs, at = [], [], 0
    for name, ti, mt, descs in tset:
        for w, h in descs:
            r = _records(ti, w, h, 1000 * ti + w)
            blocks.append((name, mt, w, h, slice(at, at + len(r))))
            recs.append(r)
            at += len(r)
    return np.concatenate(recs), blocks


# ----------------------------------------------------------------------------------------------------------------------
# the float64 candidates
# ----------------------------------------------------------------------------------------------------------------------
def _level_candidates(mt, tu, tv, o, w, h):
    """(4, n, 4): the fetch at one level for the four ways the two texel coordinates may be rounded."""
    out = []
    for fx in (False, True):
        for fy in (False, True):
            out.append(model.fetch_texel64(mt, model.texel_coordinate(tu, w, fx), model.texel_coordinate(tv, h, fy), o, w, h))
    return np.stack(out)


def _candidates(mt, rec, w, h):
    """Per record the candidate values (K, n, 4) — K = 16; a bilinear record repeats its four — and the bound's constant c."""
    n = len(rec)
    form = rec.view(np.uint32)[:, 1]
    lam, tu, tv = rec[:, 2], rec[:, 3], rec[:, 4]
    z = np.zeros(n, np.int64)
    base = _level_candidates(mt, tu, tv, z, z + w, z + h)
    (o0, w0, h0), (o1, w1, h1), f = model.trilinear_levels(mt, lam, w, h)
    p0, p1 = _level_candidates(mt, tu, tv, o0, w0, h0), _level_candidates(mt, tu, tv, o1, w1, h1)
    tri = ((1 - f)[None, None, :, None] * p0[:, None] + f[None, None, :, None] * p1[None, :]).reshape(16, n, 4)
    cand = np.where((form == 1)[None, :, None], np.tile(base, (4, 1, 1)), tri)
    return cand, np.where(form == 1, C_BILINEAR, C_TRILINEAR).astype(f64)


def _fetch_errors(got, rec, blocks):
    """Per record: error against the nearest candidate over the bound, and the distance outside the texture's own hull over it."""
    ratio, outside = np.full(len(rec), np.inf), np.full(len(rec), np.inf)
    for name, mt, w, h, sl in blocks:
        r, g = rec[sl], got[sl, :4].astype(f64)
        assert (model.texel_coordinate(r[:, 3], w, False).max() < 2.0 ** 31 - 64) and (model.texel_coordinate(r[:, 4], h, True).max() < 2.0 ** 31 - 64)
        cand, c = _candidates(mt, r, w, h)
        tex = _texels(mt)
        bound = c * U * np.abs(tex).max()
        ratio[sl] = np.abs(cand - g[None]).max(-1).min(0) / bound
        lo, hi = tex.min(0), tex.max(0)
        outside[sl] = np.maximum(np.maximum(lo[None] - g, g - hi[None]).max(-1), 0.0) / bound
        assert not got[sl, 4:].any(), name
    return ratio, outside


def _worst(name, ratio, rec, blocks):
    i = int(np.argmax(ratio))
    where = [b for b in blocks if b[4].start <= i < b[4].stop][0]
    return "%s: worst error / bound %.3f (%s, descriptor %dx%d, form %d, lambda %r, tu %r, tv %r)" % (
        name, ratio[i], where[0], where[2], where[3], rec.view(np.uint32)[i, 1], float(rec[i, 2]), float(rec[i, 3]), float(rec[i, 4]))


def _upload(c, scene):
    c.init(64, 48)
    scene.upload(c)
    return c


def _strict_hip(pkg):
    so = os.path.join(ROOT, "tests", "_strict", "librfwhip_strict.so")
    assert os.path.exists(so), "build it with __graft_entry__.build() (build.py: build_strict)"
    return pkg._binding.CoreBinding(ctypes.CDLL(so), "rfwhip_", 0, 0, 1)


@pytest.fixture(scope="module")
def emu_strict_lib():
    import build_emu
    return ctypes.CDLL(build_emu.build(defines=STRICT_FLAGS, tag="_strict"))


def _contexts(request, pkg, which):
    """name -> a fresh context of that implementation."""
    out = {}
    for w in which:
        if w == "oracle":
            out[w] = request.getfixturevalue("make_oracle")()
        elif w == "emulation":
            out[w] = request.getfixturevalue("make_emu")()
        elif w == "hip":
            out[w] = request.getfixturevalue("make_hip")()
        elif w == "strict hip":
            out[w] = _strict_hip(pkg)
        elif w == "strict emulation":
            out[w] = pkg._binding.CoreBinding(request.getfixturevalue("emu_strict_lib"), "rfwhip_", 0, 0, 1)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the mip chain of the front ends' textures
# ----------------------------------------------------------------------------------------------------------------------
def _check_integer_levels(pkg, ctxs):
    rng = np.random.default_rng(7)
    sizes = CHAINED + [WIDE]
    # the set's textures (every level independent) and what the helper builds from random images
    textures = [_rgba8(pkg, rng, w, h, True) for w, h in sizes]
    textures += [pkg.scenes.make_texture_rgba8(rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)) for w, h in sizes]
    sizes = sizes + sizes
    scene = _card_scene(pkg, textures)
    recs, want = [], []
    for ti, (w, h) in enumerate(sizes):
        data, at = np.asarray(textures[ti]["data"], np.uint32), 0
        for level, (lw, lh) in enumerate(helper_level_shapes(w, h)):
            image = dict(float4=False, data=data[at:at + lw * lh])  # the level image as it was uploaded
            at += lw * lh
            k = np.arange(max(lw, lh) * 2 + 1, dtype=f64)
            tu = np.concatenate([rng.uniform(-2, 2, 64), (k + 0.3) / (2 * lw), (k + 0.7) / (2 * lw)]).astype(f32)
            tv = np.concatenate([rng.uniform(-2, 2, 64), (k + 0.6) / (2 * lh), (k + 0.2) / (2 * lh)]).astype(f32)
            r = np.zeros((len(tu), 24), f32)
            ri = r.view(np.uint32)
            ri[:, 0], ri[:, 5], ri[:, 6] = ti, w, h
            r[:, 2], r[:, 3], r[:, 4] = level, tu, tv
            z = np.zeros(len(tu), np.int64)
            recs.append(r)
            want.append((w, h, level, _level_candidates(image, tu, tv, z, z + lw, z + lh), C_TRILINEAR * U * _texels(image).max()))
        assert at == len(data)
    failed = {}
    for name, c in ctxs.items():
        _upload(c, scene)
        got = c.kat("tex_fetch", np.concatenate(recs))[:, :4].astype(f64)
        at, worst = 0, 0.0
        for w, h, level, cand, bound in want:
            g = got[at:at + cand.shape[1]]
            at += cand.shape[1]
            ratio = (np.abs(cand - g[None]).max(-1).min(0) / bound).max()
            worst = max(worst, min(ratio, 1e9))
            if not ratio <= 1.0:
                failed.setdefault(name, []).append("%dx%d L%d" % (w, h, level))
        print("%s: integer levels of the helper's chains: worst error / bound %.3f" % (name, worst))
    assert not failed, "\n".join("%s: %s" % (k, ", ".join(v)) for k, v in failed.items())


def test_integer_level_is_the_uploaded_level_image(request, pkg):
    """fetch_trilinear at lambda = L is the bilinear fetch of the L-th level image that was uploaded, for every size of the set, in the
    layout of scenes.make_texture_rgba8 (oracle and emulation; the model's own walk is held to the same in test_model_*)."""
    _check_integer_levels(pkg, _contexts(request, pkg, ("oracle", "emulation")))


@pytest.mark.gpu
def test_integer_level_is_the_uploaded_level_image_gpu(request, pkg):
    _check_integer_levels(pkg, _contexts(request, pkg, ("hip", "strict hip")))


def test_helper_levels_are_box_filtered(pkg):
    """Every texel of every appended level is the mean of the texels of the level before under it — 2 x 2, or 2 x 1 / 1 x 2 along a
    side of 1 — within the two roundings to bytes (the stored level before it and its own: 0.5 each)."""
    rng = np.random.default_rng(3)
    for w, h in CHAINED + [WIDE, (7, 9), (1000, 3)]:
        img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        data = np.asarray(pkg.scenes.make_texture_rgba8(img)["data"], np.uint32)
        shapes = helper_level_shapes(w, h)
        assert len(data) == sum(a * b for a, b in shapes)
        at, prev = 0, None
        for lw, lh in shapes:
            lvl = model.uchar4_to_float4(data[at:at + lw * lh]).astype(f64).reshape(lh, lw, 4) * 256.0
            at += lw * lh
            if prev is None:
                assert np.array_equal(lvl, img)
            else:
                fy, fx = min(2, prev.shape[0]), min(2, prev.shape[1])
                want = prev[:lh * fy, :lw * fx].reshape(lh, fy, lw, fx, 4).mean(axis=(1, 3))
                assert np.abs(lvl - want).max() <= 1.0, (w, h, lw, lh)
            prev = lvl


def test_model_walks_the_helper_chain(pkg):
    """The numpy model's level table is the helper's layout, and its float32 fetches lie within the bound of the unfused candidate."""
    for w, h in CHAINED + PLAIN + [WIDE, (7, 3), (1000, 3)]:
        levels, chain = model.mip_levels(w, h)
        at = 0
        for (o, lw, lh), (hw, hh) in zip(levels, helper_level_shapes(w, h)):
            assert (o, lw, lh) == (at, hw, hh), (w, h)
            at += hw * hh
        assert chain == at == len(pkg.scenes.make_texture_rgba8(np.zeros((h, w, 4), np.uint8))["data"])
    tset, _ = _texture_set(pkg)
    rec, blocks = _all_records(tset)
    worst = 0.0
    for name, mt, w, h, sl in blocks:
        r = rec[sl]
        n = len(r)
        z = np.zeros(n, np.int64)
        tri = model.fetch_trilinear(mt, r[:, 2], r[:, 3], r[:, 4], w, h)
        bil = model.fetch_texel(mt, r[:, 3], r[:, 4], z, z + w, z + h)
        got = np.where((r.view(np.uint32)[:, 1] == 1)[:, None], bil, tri).astype(f64)
        cand, c = _candidates(mt, r, w, h)
        worst = max(worst, (np.abs(cand[0] - got).max(-1) / (c * U * np.abs(_texels(mt)).max())).max())
    print("numpy float32 model against its float64 evaluation: worst error / bound %.3f" % worst)
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# tex_fetch
# ----------------------------------------------------------------------------------------------------------------------
def _check_fetches(pkg, ctxs):
    tset, scene = _texture_set(pkg)
    rec, blocks = _all_records(tset)
    got, lines, bad = {}, [], []
    for name, c in ctxs.items():
        got[name] = _upload(c, scene).kat("tex_fetch", rec)
        ratio, outside = _fetch_errors(got[name], rec, blocks)
        lines.append(_worst(name, ratio, rec, blocks) + "; outside the texture's hull: %.3f x the bound" % outside.max())
        if not (ratio.max() <= 1.0 and outside.max() <= 1.0):
            bad.append(lines[-1] + "; %d of %d records beyond the bound" % (int((ratio > 1.0).sum()), len(rec)))
    print("tex_fetch, %d records:\n  " % len(rec) + "\n  ".join(lines))
    assert not bad, bad
    return got


def test_fetches_against_the_model(request, pkg):
    """Every record of the grid on the oracle and the emulation: within the derived bound of a candidate of the float64 model, and
    inside the hull of the texture's own texels (no sentinel of the neighbouring texture contributes)."""
    _check_fetches(pkg, _contexts(request, pkg, ("oracle", "emulation")))


@pytest.mark.gpu
def test_fetches_against_the_model_gpu(request, pkg):
    """The same on the HIP kernels; the strict build equals the strict emulation bit for bit."""
    got = _check_fetches(pkg, _contexts(request, pkg, ("hip", "strict hip", "strict emulation")))
    assert np.array_equal(got["strict hip"].view(np.uint32), got["strict emulation"].view(np.uint32))


def _check_loud_failures(pkg, c):
    tset, scene = _texture_set(pkg)
    rec = _records(0, 1, 1, 1)[:4]
    with pytest.raises(RuntimeError):  # no scene yet: no texture table
        c.kat("tex_fetch", rec)
    _upload(c, scene)
    assert c.kat("tex_fetch", rec).shape == (4, 8)
    for index in (len(scene.textures), 2 ** 31, 2 ** 32 - 1):
        r = rec.copy()
        r.view(np.uint32)[2, 0] = index
        with pytest.raises(RuntimeError):
            c.kat("tex_fetch", r)
    layer = np.zeros((2, 24), f32)
    layer[:, 2:9] = (0.25, 0.25, 0, 0, -1, 1.0, 1e-3)
    assert c.kat("surface_layers", layer).shape == (2, 8)
    for col, index in ((0, len(scene.instances)), (0, 2 ** 32 - 1), (1, 1), (1, 2 ** 31)):
        r = layer.copy()
        r.view(np.uint32)[1, col] = index
        with pytest.raises(RuntimeError):
            c.kat("surface_layers", r)


def test_indices_outside_the_scene_fail_loudly(request, pkg):
    for c in _contexts(request, pkg, ("oracle", "emulation")).values():
        _check_loud_failures(pkg, c)


@pytest.mark.gpu
def test_indices_outside_the_scene_fail_loudly_gpu(request, pkg):
    _check_loud_failures(pkg, _contexts(request, pkg, ("hip",))["hip"])


# ----------------------------------------------------------------------------------------------------------------------
# surface_layers
# ----------------------------------------------------------------------------------------------------------------------
def _normal_map_rgba8(pkg, rng, w, h):
    b = rng.integers(8, 248, size=(h, w, 4), dtype=np.uint8)
    b[..., 2] = rng.integers(int(ZMIN * 256), 248, size=(h, w))
    return pkg.scenes.make_texture_rgba8(b, mips=False)


def _normal_map_float4(pkg, rng, w, h):
    v = rng.uniform(-1.0, 2.0, size=(h, w, 4)).astype(f32)
    v[..., 2] = rng.uniform(0.85, 1.5, size=(h, w))
    return pkg.scenes.make_texture_float4(v)


def _rot(axis, deg):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(deg)
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * (K @ K)
    return m


def zoo(pkg):
    """Cards that carry the thin, odd-sized and FLOAT4 maps as first, second and third colour layers and as normal maps, an alpha
    material, negative uv scales and offsets, smooth normals, an untextured card, and a non-uniformly scaled, rotated instance."""
    sc = pkg.scenes
    rng = np.random.default_rng(424242)
    s = sc.Scene()
    s.name = "zoo"
    def rgba8(w, h):
        return s.add_texture(sc.make_texture_rgba8(rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)))
    def flt4(w, h):
        return s.add_texture(sc.make_texture_float4(rng.uniform(-0.5, 1.75, size=(h, w, 4)).astype(f32)))
    t16x2, t64x1, t1x64, t2x16, t5x3, t3x5 = rgba8(16, 2), rgba8(64, 1), rgba8(1, 64), rgba8(2, 16), rgba8(5, 3), rgba8(3, 5)
    t48x20, t100x36, t8x8 = rgba8(48, 20), rgba8(100, 36), rgba8(8, 8)
    f16, f13x6, f1 = flt4(16, 16), flt4(13, 6), flt4(1, 1)
    n7x9, n5x3, n2x16 = (s.add_texture(_normal_map_rgba8(pkg, rng, w, h)) for w, h in ((7, 9), (5, 3), (2, 16)))
    nf13x6 = s.add_texture(_normal_map_float4(pkg, rng, 13, 6))
    mats = [
        s.add_material(color=(0.9, 0.8, 0.7), texture=t16x2, texture1=t64x1, texture2=f13x6, normalmap=n7x9, normalmap1=n5x3,
                       normalmap2=n2x16, uvscale=(-2.5, 1.5), uvoffset=(0.25, -0.75), smooth=False),
        s.add_material(color=(1.0, 1.0, 1.0), texture=t48x20, alpha=True, uvscale=(3.0, -2.0), uvoffset=(-0.5, 0.125), smooth=False),
        s.add_material(color=(0.6, 0.7, 0.8), texture=f16, texture1=t5x3, normalmap=n2x16, uvscale=(1.0, 1.0), smooth=False),
        s.add_material(color=(0.8, 0.8, 0.8), texture=t1x64, texture1=t100x36, texture2=t3x5, normalmap=nf13x6, normalmap1=n7x9,
                       uvscale=(0.75, -4.0), uvoffset=(-3.0, 2.5), smooth=False),
        s.add_material(color=(0.4, 0.5, 0.6), smooth=False),
        s.add_material(color=(0.7, 0.7, 0.7), texture=t2x16, texture1=f1, texture2=t8x8, normalmap=n5x3, alpha=True, smooth=True,
                       uvscale=(-1.0, -1.0), uvoffset=(0.5, 0.5)),
    ]
    v = np.array([[0, 0, 0], [2, 0, 0.3], [2.2, 1.5, 0.1], [-0.1, 1.4, -0.2]], f32)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    uv = np.array([[-0.3, 0.1], [1.7, -0.2], [2.1, 1.4], [0.2, 1.9]], f32)
    vn = np.array([[0.1, -0.2, 1.0], [-0.15, 0.1, 1.0], [0.2, 0.2, 0.9], [-0.1, 0.25, 1.0]], f64)
    vn = (vn / np.linalg.norm(vn, axis=1, keepdims=True)).astype(f32)
    lods = (0.0, 1.5, -0.75, 2.25, 0.0, 0.5)
    meshes = []
    for m, lod in zip(mats, lods):
        meshes.append(s.add_mesh(v, idx, normals=vn, uvs=uv, material=m))
        s.meshes[-1]["triangles"]["LOD"][:] = lod
    # (generic rotations: every world normal keeps |z| well away from 0, where the tangent frame of tools.h:204-211 flips)
    for k, mesh in enumerate(meshes):
        T = np.eye(4)
        T[:3, 3] = (3.0 * k, 0.5 * k, -k)
        s.add_instance(mesh, T @ _rot((1, 2 + k, 0.5), 20 + 7 * k))
    S = np.diag([3.0, 0.4, 1.7, 1.0])
    T = np.eye(4)
    T[:3, 3] = (-4, 2, 1)
    s.add_instance(meshes[0], T @ _rot((0.3, 1, 0.2), 33) @ S)
    s.add_instance(meshes[3], T @ _rot((1, 0.2, -0.4), -25) @ np.diag([0.5, 2.5, 1.0, 1.0]))
    return s


def _layer_records(pt, scene, n, seed):
    """Random hits: (instance, triangle, barycentrics, D, t) with t over six decades and a quarter of the directions grazing the surface
    (|D.N| down to 1e-4)."""
    rng = np.random.default_rng(seed)
    inst = rng.integers(0, len(scene.instances), n)
    ntri = np.array([len(scene.meshes[i["mesh"]]["triangles"]) for i in scene.instances])
    prim = (rng.random(n) * ntri[inst]).astype(np.int64)
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    bu, bv = (r1 * (1 - r2)).astype(f32), (r1 * r2).astype(f32)
    over = (f32(1) - bu - bv) < 0  # (a rounding error outside the triangle: pull it in)
    bu[over] *= f32(0.5)
    bv[over] *= f32(0.5)
    D = rng.normal(size=(n, 3))
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    _, N, _, _, _, _, _, _ = pt.shading_data(D.astype(f32), bu, bv, inst, prim, np.ones(n, f32))
    graze = rng.random(n) < 0.25
    tang = np.cross(N.astype(f64), D)
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    g = tang + N.astype(f64) * (10.0 ** rng.uniform(-4, 0, n) * rng.choice([-1.0, 1.0], n))[:, None]
    D[graze] = (g / np.linalg.norm(g, axis=1, keepdims=True))[graze]
    t = (10.0 ** rng.uniform(-3, 3, n)).astype(f32)
    rec = np.zeros((n, 24), f32)
    ri = rec.view(np.uint32)
    ri[:, 0], ri[:, 1] = inst, prim
    rec[:, 2], rec[:, 3], rec[:, 4:7], rec[:, 7], rec[:, 8] = bu, bv, D.astype(f32), t, pt.spread_angle
    return rec


def _ulp(x):
    x = np.abs(np.asarray(x, f64)).astype(f32)
    return (np.nextafter(x, f32(np.inf)) - x).astype(f64)


def _layer_bounds(pkg, pt, scene, rec, probe, N):
    """B_colour, B_normal, 2 dt0 (the alpha window) per record: the module docstring's derivation."""
    n = len(rec)
    inst, prim = rec.view(np.uint32)[:, 0].astype(np.int64), rec.view(np.uint32)[:, 1].astype(np.int64)
    D, lam = rec[:, 4:7].astype(f64), probe["lam"].astype(f64)
    kappa, uvmax, vvmax, lod = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for ii, g in enumerate(pt.geo.inst):
        sel = inst == ii
        tr = g["tris"][prim[sel]]
        ng = np.stack([tr["Nx"], tr["Ny"], tr["Nz"]], -1).astype(f64)
        M = g["nrm"].astype(f64)
        kappa[sel] = ((np.abs(M)[None] * np.abs(ng)[:, None, :]).sum(-1) / np.linalg.norm(ng @ M.T, axis=1, keepdims=True)).max(-1)
        uvmax[sel], vvmax[sel], lod[sel] = np.abs(tr["u"]).max(-1), np.abs(tr["v"]).max(-1), tr["LOD"]
    # (smooth normals: the interpolated normal is within the hull of the vertex normals; the same kappa with a factor 2 covers it)
    eps_n = (3 * 2 * kappa + 6) * U
    d = np.abs((D * N.astype(f64)).sum(-1))
    dd = 3 * U + np.sqrt(3) * eps_n
    L = lam - lod
    dlam = (dd / d + 3 * U) / np.log(2) + 4 * U * np.maximum(np.abs(L), 1) + 2 * U * np.abs(lam)
    at_zero = np.abs(lam) <= 2 * dlam
    tu, tv = probe["tu"].astype(f64), probe["tv"].astype(f64)
    dt = np.zeros((6, n))     # per map slot: the fetch's allowance
    mag = np.zeros((6, n))    # M_k
    layers = np.zeros(n)      # normal-map layers
    for mi in np.unique(probe["matid"]):
        sel = probe["matid"] == mi
        fl, maps = int(pt.mat_flags[mi]), pt.mat_maps[mi]
        present = [(fl >> 2) & 1, (fl >> 9) & 1, (fl >> 10) & 1, (fl >> 3) & 1, (fl >> 3) & (fl >> 7) & 1, (fl >> 3) & (fl >> 8) & 1]
        if not present[0]:
            continue
        for k in range(6):
            if not present[k]:
                continue
            m = maps[4 if k == 5 else k]  # (the third normal layer reads the second one's descriptor)
            tex = _texels(pt.textures[int(m["addr"])])
            Mk, Rk = np.abs(tex).max(), (tex.max(0) - tex.min(0)).max()
            us, vs, uo, vo = (abs(float(m[x])) for x in ("uscale", "vscale", "uoffs", "voffs"))
            x, y = us * (uo + np.abs(tu[sel])), vs * (vo + np.abs(tv[sel]))
            dx = us * (5 * U * uvmax[sel] + U * (uo + np.abs(tu[sel]))) + U * x
            dy = vs * (5 * U * vvmax[sel] + U * (vo + np.abs(tv[sel]))) + U * y
            w, h = int(m["width"]), int(m["height"])
            dtc = (_ulp(x + 1000) + dx) * w + _ulp((x + 1000) * w) + (_ulp(y + 1000) + dy) * h + _ulp((y + 1000) * h)
            mag[k, sel] = Mk
            if k < 3:
                dt[k, sel] = C_TRILINEAR * U * Mk + Rk * (dtc + dlam[sel] + at_zero[sel])
            else:
                dt[k, sel] = C_BILINEAR * U * Mk + Rk * dtc
                layers[sel] += 1
    c = np.abs(pt.mat_color[probe["matid"]].astype(f64)).max(-1)
    s = c * mag[0] + mag[1] + mag[2]
    b_colour = (c * dt[0] + dt[1] + dt[2]) * (mag[0] + dt[0]) + s * dt[0] + 6 * U * s * mag[0]
    smin = 2 * (ZMIN - 0.5) * np.maximum(layers, 1)
    ds = 2 * (2 * dt[3:].sum(0) + 18 * U) / smin + 6 * U
    b_normal = np.where(layers > 0, 2 * (np.sqrt(3) * (8 * eps_n + ds) + 5 * U) + 6 * U, eps_n)
    return b_colour, b_normal, 2 * dt[0]


def _absdiff(a, b):
    """|a - b| per record (the largest component); a NaN agrees with a NaN only.  (The reference's createTangentSpace takes sign(N.z),
    which is 0 for N.z = 0: the frame of the cards scene's floor — normal (0, 1, 0) — is NaN in the reference, the model and every
    implementation alike.)"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    d = np.abs(a - b)
    d[np.isnan(a) & np.isnan(b)] = 0.0
    d[np.isnan(a) != np.isnan(b)] = np.inf
    return d.max(-1)


def _check_layers(pkg, scene, ctxs, n, seed, name):
    pt = model.PathTracer(pkg, scene, 96, 64)
    rec = _layer_records(pt, scene, n, seed)
    ri = rec.view(np.uint32)
    probe = {}
    sd, N, iN, _, _, _, _, alpha = pt.shading_data(rec[:, 4:7], f32(1) - rec[:, 2] - rec[:, 3], rec[:, 2], ri[:, 0].astype(np.int64),
                                                   ri[:, 1].astype(np.int64), rec[:, 7], w=rec[:, 3], probe=probe)
    b_colour, b_normal, window = _layer_bounds(pkg, pt, scene, rec, probe, N)
    lam = probe["lam"][((pt.mat_flags[probe["matid"]] >> 2) & 1).astype(bool)]
    assert lam.min() < -1 and lam.max() > 5 and (np.abs((rec[:, 4:7] * N).sum(-1)) < 1e-3).mean() > 0.02
    near = np.abs(probe["texel0"][:, 3].astype(f64) - 0.5) <= window
    base_colour, base_normal = pt.mat_color[probe["matid"]], probe["iN0"]
    got, lines, bad = {}, [], []
    def held(a_flags, a, want_alpha, want_colour, want_normal, who):
        skip = (a_flags & 1).astype(bool)
        wrong = (skip != want_alpha) & ~near
        # the record is held against the branch the implementation took (they differ only inside the alpha window)
        colour = np.where(skip[:, None], base_colour, want_colour).astype(f64)
        normal = np.where(skip[:, None], base_normal, want_normal).astype(f64)
        rc = _absdiff(a[:, 0:3], colour) / (2 * b_colour + 1e-300)  # (an untextured record's colour has to be the material's, exactly)
        rn = _absdiff(a[:, 3:6], normal) / (2 * b_normal)
        lines.append("%s %s: alpha flags that differ outside the window %d (inside it %d of %d near 0.5); colour error / bound %.3f, "
                     "normal error / bound %.3f" % (name, who, int(wrong.sum()), int((skip != want_alpha).sum()) - int(wrong.sum()), int(near.sum()),
                                                    rc.max(), rn.max()))
        if wrong.any() or not (rc.max() <= 1.0 and rn.max() <= 1.0):
            bad.append(lines[-1])
    textured = ((pt.mat_flags[probe["matid"]] >> 2) & 1).astype(np.uint32)
    for who, c in ctxs.items():
        got[who] = _upload(c, scene).kat("surface_layers", rec)
        fl = got[who].view(np.uint32)[:, 6]
        assert np.array_equal((fl >> 1) & 1, textured) and not (fl >> 2).any() and not got[who][:, 7].any(), who
        held(fl, got[who], alpha, probe["color"], probe["iN"], who + " against the model")
    if "oracle" in got:
        o = got["oracle"]
        oskip = (o.view(np.uint32)[:, 6] & 1).astype(bool)
        for who in got:
            if who == "oracle":
                continue
            a = got[who]
            skip = (a.view(np.uint32)[:, 6] & 1).astype(bool)
            same = skip == oskip
            assert not (~same & ~near).any(), who
            rc = (_absdiff(a[:, 0:3], o[:, 0:3]) / (2 * b_colour + 1e-300))[same]
            rn = (_absdiff(a[:, 3:6], o[:, 3:6]) / (2 * b_normal))[same]
            lines.append("%s %s against the oracle: colour error / bound %.3f, normal error / bound %.3f" % (name, who, rc.max(), rn.max()))
            if not (rc.max() <= 1.0 and rn.max() <= 1.0):
                bad.append(lines[-1])
    print("surface_layers, %d records:\n  " % n + "\n  ".join(lines))
    assert not bad, bad
    return got


def _layer_scenes(pkg):
    return [("cards", pkg.scenes.cards(96, 64), 11), ("zoo", zoo(pkg), 12)]


def test_surface_layers_against_the_model(request, pkg):
    """200 000 random hits per scene on the oracle and the emulation, against PathTracer.shading_data and each other."""
    for name, scene, seed in _layer_scenes(pkg):
        _check_layers(pkg, scene, _contexts(request, pkg, ("oracle", "emulation")), 200_000, seed, name)


@pytest.mark.gpu
def test_surface_layers_against_the_model_gpu(request, pkg):
    """The same on the HIP kernels; the strict build equals the strict emulation bit for bit."""
    for name, scene, seed in _layer_scenes(pkg):
        got = _check_layers(pkg, scene, _contexts(request, pkg, ("oracle", "hip", "strict hip", "strict emulation")), 200_000, seed, name)
        assert np.array_equal(got["strict hip"].view(np.uint32), got["strict emulation"].view(np.uint32)), name
