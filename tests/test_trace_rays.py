"""Closest-hit traversal on arbitrary rays (rfwhip_trace_rays) against the oracle: random rays, axis-parallel rays
whose direction has exact zero components, rays starting on / inside boxes, empty intervals.  CPU tier through the
host-emulation build; the GPU tier repeats it on the kernels."""
import numpy as np
import pytest


def _rays(rng, n, extent):
    o = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    o[:, 1] = rng.uniform(2.0, 30.0, n)
    d = rng.normal(size=(n, 3))
    d[:, 1] = -np.abs(d[:, 1]) - 0.05
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def _degenerate_rays(n_side, extent):
    """Rays with exactly-zero direction components, origins on the grid lines x = 0 / z = 0 of the terrain."""
    xs = np.linspace(-extent * 0.4, extent * 0.4, n_side, dtype=np.float32)
    o, d = [], []
    for x in xs:
        o.append((x, 20.0, 0.0)); d.append((0.0, -1.0, 0.0))            # straight down: d.x = d.z = 0
        o.append((0.0, 18.0, x)); d.append((0.0, -0.6, 0.8))            # d.x = 0, origin in the plane x = 0
        o.append((x, 6.0, -extent)); d.append((0.0, -0.05, 1.0))        # grazing, d.x = 0
        o.append((-extent, 5.0, x)); d.append((1.0, -0.04, 0.0))        # grazing, d.z = 0
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float64)
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _compare(a, b, ties=False):
    if ties:
        # rays running exactly along shared edges / through shared vertices: which of the tied neighbours wins is
        # traversal-order dependent (both restate "t > t_min && t < current"), distance and hit status are not
        assert np.array_equal(a["prim"] >= 0, b["prim"] >= 0)
        hit = a["prim"] >= 0
        assert np.abs(a["t"][hit] - b["t"][hit]).max() <= 2e-3
        return
    assert (a["prim"] != b["prim"]).mean() <= 2e-3
    assert (a["inst"] != b["inst"]).mean() <= 2e-3
    same = (a["prim"] == b["prim"]) & (a["prim"] >= 0)
    assert same.sum() > 0.5 * len(same)
    assert np.abs(a["t"][same] - b["t"][same]).max() <= 2e-3
    assert np.abs(a["u"][same] - b["u"][same]).max() <= 1e-3 and np.abs(a["v"][same] - b["v"][same]).max() <= 1e-3


def check_traversal(pkg, core, oracle, n_random=20000):
    scene = pkg.scenes.terrain(n=64, width=64, height_px=64)
    for c in (core, oracle):
        c.init(64, 64)
        scene.upload(c)
    rng = np.random.default_rng(17)
    o, d = _rays(rng, n_random, 45.0)
    _compare(core.trace_rays(o, d), oracle.trace_rays(o, d))
    # exact-zero direction components must neither change the answer nor blow up the traversal
    o, d = _degenerate_rays(64, 50.0)
    core.set_setting("count_traversal", 1)
    core.get_counters(reset=True)
    a = core.trace_rays(o, d)
    cnt = core.get_counters(reset=True)
    core.set_setting("count_traversal", 0)
    _compare(a, oracle.trace_rays(o, d), ties=True)
    assert cnt["rays_extend"] == len(o)
    assert cnt["inner_extend"] / len(o) < 120, cnt    # was ~5800 per ray before slab_rcp's clamp (inf * 0 = NaN in the slab test)
    # intervals: nothing before t_min, nothing beyond t_max
    full = core.trace_rays(o[:64], d[:64])
    hit = full["prim"] >= 0
    far = core.trace_rays(o[:64], d[:64], t_min=1e-5, t_max=float(full["t"][hit].min()) * 0.5)
    assert (far["prim"] < 0).all()
    beyond = core.trace_rays(o[:64], d[:64], t_min=float(full["t"][hit].max()) + 1.0, t_max=1e34)
    assert (beyond["t"][beyond["prim"] >= 0] > full["t"][hit].max()).all()


def test_traversal_emulated_core(pkg, make_emu, make_oracle):
    check_traversal(pkg, make_emu(), make_oracle())


def test_instanced_traversal_emulated_core(pkg, make_emu, make_oracle):
    scene = pkg.scenes.cornell(32, 32)
    e, o = make_emu(), make_oracle()
    for c in (e, o):
        c.init(32, 32)
        scene.upload(c)
    rng = np.random.default_rng(23)
    org = rng.uniform(-4.5, 4.5, (5000, 3)).astype(np.float32)
    org[:, 1] = rng.uniform(0.2, 9.5, 5000)
    d = rng.normal(size=(5000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    _compare(e.trace_rays(org, d), o.trace_rays(org, d))


@pytest.mark.gpu
def test_traversal_gpu(pkg, make_hip, make_oracle):
    check_traversal(pkg, make_hip(), make_oracle(), n_random=200000)
