"""The light tree on the MI355X (k_shade_pt_lt, the light-tree cases of k_kat_lt): the device against the host emulation of the
same sources (bit for bit under the strict build), scheduling independence, the estimator of `tree` against `linear`, and the
O(log n) against O(n) sanity condition."""
import ctypes
import os
import time

import numpy as np
import pytest

from conftest import ROOT
from test_light_tree import _lamp, _n_lights, _points, _with_light

pytestmark = pytest.mark.gpu

STRICT_FLAGS = ("-DRT_STRICT_MATH", "-ffp-contract=off")

# Default build against the emulation on the 100 000 records of test_device_kat_equals_the_emulation, measured on the MI355X on
# the first run: the drawn light (or whether the sample point gets a density at all) differs on 1.0e-5 of the records — a
# selection number within rounding of an interval's edge: v_rcp / v_sqrt / v_rsq against IEEE division and square root at every
# level; the emulation against the float64 model's walk: 0 of 2000 — and on the others the largest relative difference is
# 6.09e-4 for q and lightPdf (lightPdf = dist^2 / (area LNdotL) near a light's horizon, where LNdotL is a difference of rounded
# products) and 1.88e-5 for LT_PICK_PROB.  Allowed: 1e-3 of the records and four times the larger relative difference.
KAT_REL_MEASURED = 6.09e-4
KAT_REL_TOL = 4.0 * KAT_REL_MEASURED


@pytest.fixture(scope="module")
def emu_strict_lib():
    import build_emu
    return ctypes.CDLL(build_emu.build(defines=STRICT_FLAGS, tag="_strict"))


def _strict_hip():
    so = os.path.join(ROOT, "tests", "_strict", "librfwhip_strict.so")
    assert os.path.exists(so), "build it with __graft_entry__.build() (build.py: build_strict)"
    return ctypes.CDLL(so)


def _upload(pkg, c, scene, w, h, settings):
    c.init(w, h)
    scene.upload(c)
    for k, v in settings.items():
        c.set_setting(k, v)
    return c


def _render(pkg, c, scene, frames=1):
    for f in range(frames):
        c.render_frame(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
    st = c.get_stats()
    return c.framebuffer(), (st.primaryCount, st.secondaryCount, st.deepCount, st.shadowCount)


@pytest.mark.parametrize("strict", [False, True])
def test_device_kat_equals_the_emulation(pkg, make_hip, make_emu, emu_strict_lib, strict):
    """RFWHIP_KAT_LT_SAMPLE / _LT_PICK_PROB on 100 000 records over the 1000-light scene: bit-equal to the emulation under the
    strict build.  Default build: the drawn light differs on at most 1e-3 of the records (the emulation against the float64
    model stays inside that too: checked here first), q and lightPdf on the others within KAT_REL_TOL."""
    import light_tree_model as model
    scene = _lamp(pkg, 1000, 64, 48)
    settings = {"integrator": "pt", "light_sampling": "tree"}
    if strict:
        dev = _upload(pkg, pkg._binding.CoreBinding(_strict_hip(), "rfwhip_", 0, 0, 1), scene, 64, 48, settings)
        emu = _upload(pkg, pkg._binding.CoreBinding(emu_strict_lib, "rfwhip_", 0, 0, 1), scene, 64, 48, settings)
    else:
        dev = _upload(pkg, make_hip(), scene, 64, 48, settings)
        emu = _upload(pkg, make_emu(), scene, 64, 48, settings)
    n = _n_lights(scene)
    na, nb = dev.get_light_tree(n), emu.get_light_tree(n)
    assert np.array_equal(na[0], nb[0]) and np.array_equal(na[1], nb[1])  # (the host builds it: the same tree)
    rec = _points(100_000, seed=31, lo=(-8, 0, -8), hi=(8, 8, 8))
    a, b = dev.kat("lt_sample", rec), emu.kat("lt_sample", rec)
    la, lb = a[:, 5].view(np.int32), b[:, 5].view(np.int32)
    rq = _with_light(rec, np.where(lb >= 0, lb, 0).astype(np.uint32))
    pa, pb = dev.kat("lt_pick_prob", rq), emu.kat("lt_pick_prob", rq)
    if strict:
        # (bit patterns: "no light" is index -1, a NaN when read as a float)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
        return
    # the emulation against the model first: the light the model's walk draws for the same r1 (2000 records: the model walks in Python)
    k = 2000
    dirs = scene.light_arrays()[3]
    lm = np.array([model.sample(nb[0], n - len(dirs), dirs, rec[i, 0:3], rec[i, 3:6], float(rec[i, 7]))[0] for i in range(k)])
    off_model = float((lm != lb[:k]).mean())
    # (a lightPdf that is 0 on one side only — the sample point within rounding of the light's horizon or the surface's — counts
    # as a differing record)
    differ = float(((la != lb) | ((a[:, 4] > 0) != (b[:, 4] > 0))).mean())
    same = (la == lb) & (lb >= 0)
    lit = same & (a[:, 4] > 0) & (b[:, 4] > 0)
    rel = max(float(np.abs(a[same, 3] / b[same, 3] - 1.0).max()), float(np.abs(a[lit, 4] / b[lit, 4] - 1.0).max()))
    relp = float(np.abs(pa[same, 0] / pb[same, 0] - 1.0).max())
    print("default build against the emulation: drawn light differs on %.2e of %d records (the emulation against the float64 model: "
          "%.2e of 2000); largest relative difference of q, lightPdf %.2e, of LT_PICK_PROB %.2e (allowed %.2e)"
          % (differ, len(rec), off_model, rel, relp, KAT_REL_TOL))
    assert off_model <= 1e-3
    assert differ <= 1e-3
    assert rel <= KAT_REL_TOL and relp <= KAT_REL_TOL
    np.testing.assert_allclose(a[same, 0:3], b[same, 0:3], atol=2e-5)


@pytest.mark.parametrize("mode", ["tree", "linear"])
def test_strict_hip_equals_strict_emulation_bit_for_bit(pkg, emu_strict_lib, mode):
    w, h = 96, 64
    scene = _lamp(pkg, 300, w, h)
    settings = {"integrator": "pt", "spp": 8, "max_depth": 2, "light_sampling": mode}
    hip = _upload(pkg, pkg._binding.CoreBinding(_strict_hip(), "rfwhip_", 0, 0, 1), scene, w, h, settings)
    emu = _upload(pkg, pkg._binding.CoreBinding(emu_strict_lib, "rfwhip_", 0, 0, 1), scene, w, h, settings)
    a, b = _render(pkg, hip, scene), _render(pkg, emu, scene)
    differing = int((np.abs(a[0] - b[0]).max(-1) > 0).sum())
    print("%s: strict HIP vs strict emulation: %d of %d pixels differ; counts %s / %s" % (mode, differing, w * h, a[1], b[1]))
    assert a[1] == b[1] and differing == 0
    assert a[0][..., :3].mean() > 0.05


def test_scheduling_does_not_change_the_image(pkg, make_hip):
    """spp 16 at 480 x 270 on the lamp scene (the packet form of the depth-0 connection wave is active): fuse, shadow_packets,
    shadow_side, streams and ring (pipelined calls) give the same image and ray counts in `tree`."""
    w, h = 480, 270
    scene = _lamp(pkg, 300, w, h)
    base = {"integrator": "pt", "spp": 16, "max_depth": 2, "light_sampling": "tree"}
    ref = None
    variants = [{}, {"fuse": 0}, {"fuse": 1}, {"shadow_packets": 0}, {"shadow_packets": 1}, {"shadow_side": 0},
                {"shadow_side": 1}, {"streams": 1}, {"streams": 4}]
    c = _upload(pkg, make_hip(), scene, w, h, base)
    assert int(c.get_setting("light_tree")) == 2 * (_n_lights(scene) - 1)
    for v in variants:
        for k, x in base.items():
            c.set_setting(k, x)
        for k, x in v.items():
            c.set_setting(k, x)
        img = _render(pkg, c, scene)
        if ref is None:
            ref = img
        assert img[1] == ref[1] and np.array_equal(img[0], ref[0]), v
    for ring in (1, 2, 4):  # pipelined: frames in flight on the ring of buffer sets
        c.set_setting("ring", ring)
        for f in range(3):
            c.render_async(scene.camera, pkg.RESET)
        c.wait()
        st = c.get_stats()
        assert np.array_equal(c.framebuffer(), ref[0]), ring
        assert (st.primaryCount, st.secondaryCount, st.deepCount, st.shadowCount) == ref[1], ring
    # and the other modes give other images
    for mode in ("linear", "reference"):
        c.set_setting("light_sampling", mode)
        assert not np.array_equal(_render(pkg, c, scene)[0], ref[0])


def test_tree_unbiased_against_linear(pkg, make_hip):
    """`tree` against `linear` at 480 x 270, 16 frames of 8 spp, on the lamp scene: tile means (30 x 30 pixels) show no systematic
    difference — mean z over tiles, share of |z| > 4 and image mean as test_bench_terrain_unbiased_and_less_noisy states them."""
    w, h = 480, 270
    scene = _lamp(pkg, 300, w, h)
    t, n = 30, 16
    tiles = []
    for mode in ("linear", "tree"):
        c = _upload(pkg, make_hip(), scene, w, h, {"integrator": "pt", "spp": 8, "max_depth": 2, "light_sampling": mode})
        tl, prev = [], None
        for k in range(1, n + 1):
            c.render_frame(scene.camera, pkg.RESET if k == 1 else pkg.CONVERGE)
            m = c.framebuffer()[..., :3].astype(np.float64)
            f = m if prev is None else k * m - (k - 1) * prev  # (this frame's own samples)
            prev = m
            tl.append(f.reshape(h // t, t, w // t, t, 3).mean((1, 3)))
        tiles.append(np.stack(tl))
    ta, tb = tiles
    z = (ta.mean(0) - tb.mean(0)) / np.sqrt(ta.var(0, ddof=1) / n + tb.var(0, ddof=1) / n + 1e-30)
    rel = abs(tb.mean() / ta.mean() - 1.0)
    tail = float((np.abs(z) > 4.0).mean())
    print("lamp scene, linear against tree: z over %d tile channels: mean %.3f, max |z| %.2f, share beyond 4: %.4f; image means "
          "%.5f / %.5f (%.2e relative)" % (z.size, z.mean(), np.abs(z).max(), tail, ta.mean(), tb.mean(), rel))
    assert ta.mean() > 0.05
    assert abs(z.mean()) <= 0.15 and tail <= 5e-3 and rel <= 5e-3


def test_tree_frame_takes_less_than_half_a_reference_frame_at_4096_lights(pkg, make_hip):
    """O(log n) against O(n), a sanity condition: 4096 light triangles, 480 x 270, spp 4."""
    w, h = 480, 270
    scene = _lamp(pkg, 4096, w, h, extras=False)
    times = {}
    for mode in ("reference", "tree"):
        c = _upload(pkg, make_hip(), scene, w, h, {"integrator": "pt", "spp": 4, "max_depth": 2, "light_sampling": mode})
        c.render_frame(scene.camera, pkg.RESET)  # (warm-up: allocations, the tree)
        best = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            c.render_frame(scene.camera, pkg.RESET)
            best = min(best, time.perf_counter() - t0)
        times[mode] = best
    print("4096 lights, 480 x 270, spp 4: reference %.2f ms, tree %.2f ms per frame" % (1e3 * times["reference"], 1e3 * times["tree"]))
    assert times["tree"] < 0.5 * times["reference"]
