"""Scenes and ray families of tests/test_traversal_forms.py: the smallest geometry and the smallest ray sets at which the traversal
kernels can go wrong.  Everything is built here from fixed seeds; nothing is read from a file."""
import numpy as np

RANDOM_FAMILIES = ("random", "zero_components", "inside_boxes", "miss", "between")  # the model alone must decide 99 % of these
# undecided by construction (a hit at the edge of a rule): no such cap
ADVERSARIAL_FAMILIES = ("along_faces", "on_planes", "edges", "vertices", "diagonals", "det_rule", "strip")
FAMILIES = RANDOM_FAMILIES + ADVERSARIAL_FAMILIES
SPILL_MESH_NAME = "graded strip"


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
def grid(nx, nz, size, bump, seed, origin=(0.0, 0.0, 0.0)):
    """nx x nz cells in the xz plane around `origin`, displaced in y: indexed, every inner edge and vertex shared."""
    rng = np.random.default_rng(seed)
    gx, gz = np.meshgrid(np.arange(nx + 1), np.arange(nz + 1), indexing="xy")
    v = np.stack([(gx / nx - 0.5) * size, rng.uniform(-bump, bump, gx.shape), (gz / nz - 0.5) * size], -1).reshape(-1, 3)
    v = (v + np.asarray(origin)).astype(np.float32)
    i00 = (gz[:-1, :-1] * (nx + 1) + gx[:-1, :-1]).ravel()
    idx = np.empty((2 * nx * nz, 3), np.uint32)
    idx[0::2] = np.stack([i00, i00 + nx + 1, i00 + 1], 1)
    idx[1::2] = np.stack([i00 + 1, i00 + nx + 1, i00 + nx + 2], 1)
    return v, idx


def fan(k, seed, size=1.0):
    """k triangles around one shared vertex (k = 1 .. 9)."""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 1.6 * np.pi, k + 1))
    rim = np.stack([np.cos(ang), rng.uniform(-0.2, 0.2, k + 1), np.sin(ang)], -1) * size * rng.uniform(0.6, 1.0, (k + 1, 1))
    v = np.concatenate([[[0.0, 0.1, 0.0]], rim]).astype(np.float32)
    idx = np.array([(0, j + 1, j + 2) for j in range(k)], np.uint32)
    return v, idx


def flat_quad(axis, coord, size=1.5):
    """An axis-aligned quad in the plane x_axis = coord (two triangles sharing the diagonal): a box of zero extent."""
    a, b = [k for k in range(3) if k != axis]
    v = np.zeros((4, 3), np.float32)
    v[:, axis] = coord
    v[:, a] = (-size, size, size, -size)
    v[:, b] = (-size, -size, size, size)
    return v, np.array([(0, 1, 2), (0, 2, 3)], np.uint32)


def open_box(h):
    lo, hi = -h, h
    c = np.array([[lo, lo, lo], [hi, lo, lo], [hi, hi, lo], [lo, hi, lo], [lo, lo, hi], [hi, lo, hi], [hi, hi, hi], [lo, hi, hi]], np.float32)
    faces = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 4, 7, 3), (1, 2, 6, 5), (3, 7, 6, 2), (0, 1, 5, 4)]
    return c, np.array([t for a, b, c_, d in faces for t in ((a, b, c_), (a, c_, d))], np.uint32)


def graded_strip(n=160, ratio=1.06, first=1e-3):
    """A strip of quads along x whose lengths grow geometrically: every split of a builder peels a little off one end, the tree is as
    deep as trees over sane geometry get."""
    x = np.concatenate([[0.0], np.cumsum(first * ratio ** np.arange(n))])
    w = 0.05
    v = np.zeros((2 * (n + 1), 3), np.float32)
    v[0::2, 0], v[1::2, 0] = x, x
    v[0::2, 2], v[1::2, 2] = -w, w
    idx = np.empty((2 * n, 3), np.uint32)
    k = np.arange(n)
    idx[0::2] = np.stack([2 * k, 2 * k + 1, 2 * k + 2], 1)
    idx[1::2] = np.stack([2 * k + 2, 2 * k + 1, 2 * k + 3], 1)
    return v, idx


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    return m


def scale(x, y=None, z=None):
    return np.diag([x, x if y is None else y, x if z is None else z, 1.0])


def torture(pkg):
    """One scene of many meshes (module docstring of tests/test_traversal_forms.py lists what each is for).  Returns the scene; its
    attribute `parts` names the instances: {name: instance index}."""
    s = pkg.scenes.Scene()
    s.name = "torture"
    s.add_material(color=(0.7, 0.7, 0.7), roughness=1.0)
    parts = {}

    def put(name, v, idx, transform=None):
        m = s.add_mesh(v, idx)
        parts[name] = s.add_instance(m, transform)
        return m

    # meshes of 1, 2, 3, 4, 5 and 9 triangles: roots that are leaves, "slot 1", the edges of the 4-wide collapse
    for j, k in enumerate((1, 2, 3, 4, 5, 9)):
        v, idx = fan(k, 100 + k)
        put("fan%d" % k, v + np.float32([-10 + 4 * j, 0, -10]), idx)
    # one flat quad per axis: boxes of zero extent
    for axis in range(3):
        v, idx = flat_quad(axis, 0.0)
        put("flat%d" % axis, v + np.float32([-10 + 5 * axis, 0.5, -4]), idx)
    # two coplanar duplicate triangles inside one mesh (primitives 1 and 2), between two others
    v, idx = grid(2, 1, 2.0, 0.1, 7)
    idx = np.concatenate([idx[:2], idx[1:2], idx[2:]])
    put("dup_prims", v + np.float32([6, 0, -4]), idx)
    # one mesh instanced twice in the same place: ties on the instance
    v, idx = grid(2, 2, 2.0, 0.1, 8)
    m = put("twin_a", v, idx, translate(10, 0, -4))
    parts["twin_b"] = s.add_instance(m, translate(10, 0, -4))
    # slivers, aspect 1 : 10^4
    v = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 2e-4], [0, 0.5, 0], [0, 0.5, 2], [2e-4, 0.5, 1], [0, 1, 0], [2, 1, 2], [2 - 1.4e-4, 1, 2 + 1.4e-4]], np.float32)
    put("slivers", v + np.float32([-10, 0, 2]), np.arange(9, dtype=np.uint32).reshape(3, 3))
    # right triangles whose doubled area (|a| for a unit ray along the normal) is 0.5, 0.9995, 1.0005 and 2 times the 1e-6 of the rule
    tv = []
    for j, k in enumerate((0.5, 0.9995, 1.0005, 2.0)):
        L = np.sqrt(1e-6 * k)
        tv += [[0.01 * j, 0, 0], [0.01 * j, 0, L], [0.01 * j + L, 0, 0]]
    put("det_rule", np.float32(tv) + np.float32([-5, 0.25, 2]), np.arange(12, dtype=np.uint32).reshape(4, 3))
    # a mesh 1e3 units from the origin with 0.1-unit triangles (its vertices ARE there: the transform is the identity)
    v, idx = grid(6, 6, 0.6, 0.02, 9, origin=(1000.0, 0.0, 1000.0))
    put("far", v, idx)
    # instances: rotation, non-uniform scale, scale 0.002 and 50, a mirror
    v, idx = grid(5, 5, 2.0, 0.15, 10)
    base = put("rotated", v, idx, translate(0, 0, 2) @ rotation((1, 2, 3), 37.0))
    parts["stretched"] = s.add_instance(base, translate(4, 0, 2) @ scale(1.0, 3.0, 0.25))
    parts["mirrored"] = s.add_instance(base, translate(8, 0, 2) @ rotation((0, 1, 0), 20.0) @ scale(-1.0, 1.0, 1.0))
    v, idx = grid(5, 5, 1000.0, 60.0, 11)
    put("scaled_down", v, idx, translate(12, 0, 2) @ scale(0.002))
    v, idx = grid(5, 5, 0.04, 0.003, 12)
    put("scaled_up", v, idx, translate(16, 0, 2) @ rotation((0, 0, 1), 10.0) @ scale(50.0))
    # an instance whose box lies inside another's
    v, idx = open_box(1.0)
    box = put("outer_box", v, idx, translate(-10, 1.0, 8) @ rotation((1, 2, 3), 30.0))
    parts["inner_box"] = s.add_instance(box, translate(-10, 1.0, 8) @ rotation((3, 1, 2), 50.0) @ scale(0.3))
    # an axis-aligned box as uploaded (identity): rays with zero direction components run exactly along its faces
    put("aligned_box", v * np.float32(0.75) + np.float32([-5, 1.0, 12]), idx)
    # the spill scene: a tree deeper than both LDS stacks
    v, idx = graded_strip()
    put(SPILL_MESH_NAME, v, idx, translate(-4, 0.0, 20))
    s.parts = parts
    return s


def upload(ctx, scene, flat):
    """flat: static instances linked flat into the world tree, or every instance kept as an instance."""
    ctx.init(32, 32)
    ctx.set_setting("flat_instances", 1 if flat else 0)
    scene.upload(ctx)


# ---- rays -----------------------------------------------------------------------------------------------------------------------
def _world_triangles(scene):
    """float64 world-space corners of every triangle: (inst, prim, 3 x 3), and the indexed corners for shared edges / vertices"""
    out = []
    for ii, it in enumerate(scene.instances):
        mesh = scene.meshes[it["mesh"]]
        v = np.asarray(mesh["vertices"], np.float32)[:, :3].astype(np.float64)
        idx = mesh["indices"]
        idx = np.arange(len(v)).reshape(-1, 3) if idx is None else np.asarray(idx, np.int64).reshape(-1, 3)
        M = np.asarray(it["transform"], np.float64).astype(np.float32).astype(np.float64)
        w = v @ M[:3, :3].T + M[:3, 3]
        out.append(dict(inst=ii, corners=w[idx], idx=idx, world=w))
    return out


def _aim(rng, target, dist_lo=0.5, dist_hi=6.0, jitter=0.0):
    """float32 rays from random origins towards float64 targets"""
    n = len(target)
    away = rng.normal(size=(n, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    org = (target + away * rng.uniform(dist_lo, dist_hi, (n, 1))).astype(np.float32)
    d = target - org.astype(np.float64) + rng.normal(size=(n, 3)) * jitter
    return org, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _points_on(rng, tris, n, weights=None):
    """n random interior points on randomly chosen triangles (every instance alike, whatever its size)"""
    which = rng.integers(0, len(tris), n) if weights is None else rng.choice(len(tris), n, p=weights)
    pts, scale_ = np.empty((n, 3)), np.empty(n)
    for k, w in enumerate(which):
        T = tris[w]["corners"]
        c = T[rng.integers(0, len(T))]
        b = rng.dirichlet((1.5, 1.5, 1.5))
        pts[k] = b @ c
        scale_[k] = np.sqrt(np.linalg.norm(np.cross(c[1] - c[0], c[2] - c[0])))
    return pts, scale_


def families(scene, n=512, seed=20261017):
    """{family: (org, dir)} float32, n rays each (fewer where the scene has nothing to aim at)."""
    rng = np.random.default_rng(seed)
    tris = _world_triangles(scene)
    fam = {}
    # random origins and directions, aimed near the geometry so that most of them meet something
    pts, sc = _points_on(rng, tris, n)
    o, d = _aim(rng, pts, jitter=0.05)
    o[: n // 4] = (pts[: n // 4] + rng.normal(size=(n // 4, 3)) * sc[: n // 4, None] * 3.0).astype(np.float32)  # close-up: a few extents away
    dd = pts[: n // 4] - o[: n // 4].astype(np.float64)
    d[: n // 4] = (dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(np.float32)
    fam["random"] = (o, d)
    # one and two exactly-zero direction components, +0.0 and -0.0
    def zero_rays(targets, m, off_plane):
        pts, sc = _points_on(rng, targets, m)
        pts = pts + rng.normal(size=(m, 3)) * off_plane * sc[:, None]  # (aimed beside the point: the ray lies in no face's plane)
        d = rng.normal(size=(m, 3))
        zero = rng.integers(0, 3, m)
        d[np.arange(m), zero] = 0.0
        two = rng.random(m) < 0.4
        d[np.arange(m)[two], (zero[two] + 1) % 3] = 0.0
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d = d.astype(np.float32)
        neg = rng.random((m, 3)) < 0.5
        d[(d == 0) & neg] = -0.0
        return (pts - d.astype(np.float64) * rng.uniform(0.5, 5.0, (m, 1)) * np.maximum(sc, 0.05)[:, None]).astype(np.float32), d

    parts = getattr(scene, "parts", {})
    aligned = parts.get("aligned_box", -1)
    fam["zero_components"] = zero_rays([t for t in tris if t["inst"] != aligned], n, 0.05)
    if aligned >= 0:
        # ... and aimed at the axis-aligned box: they start in the plane of a face and run exactly along it, into the edges of others
        fam["along_faces"] = zero_rays([tris[aligned]], n // 2, 0.0)
    # origins inside the meshes' world boxes (the nested boxes among them)
    o = np.empty((n, 3), np.float32)
    for k in range(n):
        T = tris[rng.integers(0, len(tris))]
        lo, hi = T["world"].min(0), T["world"].max(0)
        o[k] = rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo))
    d = rng.normal(size=(n, 3))
    fam["inside_boxes"] = (o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    # origins exactly on a triangle's plane (a corner, a point of the triangle: t = 0 against the 1e-5 of the rule) and exactly on a
    # face of a mesh's world box (which for flat geometry is the triangles' plane again)
    o = np.empty((n, 3), np.float32)
    for k in range(n):
        T = tris[rng.integers(0, len(tris))]
        c = T["corners"][rng.integers(0, len(T["corners"]))]
        if k % 3 == 0:
            o[k] = c[rng.integers(0, 3)]
        elif k % 3 == 1:
            o[k] = c[0] + (c[1] - c[0]) * np.float32(0.25) + (c[2] - c[0]) * np.float32(0.25)
        else:
            lo, hi = T["world"].min(0), T["world"].max(0)
            p = rng.uniform(lo, hi)
            ax = rng.integers(0, 3)
            p[ax] = (lo, hi)[rng.integers(0, 2)][ax]
            o[k] = p
    d = rng.normal(size=(n, 3))
    fam["on_planes"] = (o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    # rays that miss everything: they start outside the scene's bounding sphere and point away from it
    allw = np.concatenate([t["world"] for t in tris])
    centre, radius = 0.5 * (allw.min(0) + allw.max(0)), 0.5 * np.linalg.norm(allw.max(0) - allw.min(0))
    out = rng.normal(size=(n, 3))
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    o = (centre + out * radius * rng.uniform(1.01, 1.5, (n, 1))).astype(np.float32)
    d = out + rng.normal(size=(n, 3)) * 0.3
    fam["miss"] = (o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    # rays through the gaps: aimed at points a little off the geometry (they end in empty space as occlusion rays)
    pts, sc = _points_on(rng, tris, n)
    off = rng.normal(size=(n, 3))
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    fam["between"] = _aim(rng, pts + off * np.maximum(sc, 0.05)[:, None] * rng.uniform(0.2, 1.5, (n, 1)))
    # aimed in float64 at interior points of shared edges, at shared vertices, at the diagonals of the flat quads
    edges, verts = [], []
    for T in tris:
        idx, w = T["idx"], T["world"]
        e = np.sort(np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]]), axis=1)
        ue, cnt = np.unique(e, axis=0, return_counts=True)
        edges += [(w[a], w[b]) for a, b in ue[cnt >= 2]]
        uv, cnt = np.unique(idx, return_counts=True)
        verts += [w[a] for a in uv[cnt >= 2]]
    if edges:
        pick = rng.integers(0, len(edges), n)
        lam = rng.uniform(0.05, 0.95, n)
        fam["edges"] = _aim(rng, np.array([edges[p][0] * (1 - l) + edges[p][1] * l for p, l in zip(pick, lam)]))
        fam["vertices"] = _aim(rng, np.array([verts[p] for p in rng.integers(0, len(verts), n)]))
    diag = []
    for axis in range(3):
        if "flat%d" % axis in parts:
            w = tris[parts["flat%d" % axis]]["world"]
            diag.append((w[0], w[2]))
    if diag:
        pick, lam = rng.integers(0, len(diag), n), rng.uniform(0.02, 0.98, n)
        fam["diagonals"] = _aim(rng, np.array([diag[p][0] * (1 - l) + diag[p][1] * l for p, l in zip(pick, lam)]))
    if "det_rule" in parts:
        # at the tiny triangles on either side of |a| = 1e-6, nearly along their normal (|a| = |d . n| x doubled area for a unit d)
        C = tris[parts["det_rule"]]["corners"]
        pts = np.array([rng.dirichlet((2, 2, 2)) @ C[k % len(C)] for k in range(n)])
        o = (pts + np.array([0, 1, 0]) * rng.uniform(0.5, 2.0, (n, 1)) * np.where(rng.random((n, 1)) < 0.5, 1, -1) + rng.normal(size=(n, 3)) * 0.05).astype(np.float32)
        dd = pts - o.astype(np.float64)
        fam["det_rule"] = (o, (dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(np.float32))
    if SPILL_MESH_NAME in parts:
        # along the graded strip, grazing it from the wide end towards the narrow one and back: every box of the deep tree is entered
        w = tris[parts[SPILL_MESH_NAME]]["world"]
        lo, hi = w.min(0), w.max(0)
        m = min(n, 256)
        a = np.stack([np.full(m, hi[0] + 0.5), lo[1] + rng.uniform(1e-4, 0.05, m), rng.uniform(lo[2], hi[2], m)], -1)
        b = np.stack([np.full(m, lo[0]) + rng.uniform(0, 0.02, m), np.full(m, lo[1]) - rng.uniform(-1e-4, 1e-3, m), rng.uniform(lo[2], hi[2], m)], -1)
        flip = rng.random(m) < 0.3
        a[flip], b[flip] = b[flip] + [-0.5, 0.01, 0], a[flip] + [0, -0.06, 0]
        o = a.astype(np.float32)
        dd = b - o.astype(np.float64)
        fam["strip"] = (o, (dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(np.float32))
    return fam


T_MAX_KINDS = ("before", "just_before", "at", "just_behind", "behind", "half", "tiny", "eps", "negative", "far")
T_MAX_DECIDED = ("before", "behind", "half", "tiny", "eps", "negative", "far")  # (the kinds a ulp or two from the hit are adversarial)


def t_max_for(first_hit, kind):
    """Per-ray t_max (float32) placed around the float64 first hit (rays without one: around 1)."""
    t = np.where(np.isfinite(first_hit), first_hit, 1.0)
    t32 = t.astype(np.float32)
    one = np.float32(np.inf)
    if kind == "before":
        return (t * (1 - 1e-3)).astype(np.float32)
    if kind == "just_before":
        return np.nextafter(np.nextafter(t32, -one), -one)
    if kind == "at":
        return t32
    if kind == "just_behind":
        return np.nextafter(np.nextafter(t32, one), one)
    if kind == "behind":
        return (t * (1 + 1e-3)).astype(np.float32)
    if kind == "half":
        return (t * 0.5).astype(np.float32)
    if kind == "tiny":
        return np.full(len(t), 1e-5, np.float32)
    if kind == "eps":
        return np.full(len(t), 4e-6, np.float32)
    if kind == "negative":
        return np.full(len(t), -1.0, np.float32)
    return np.full(len(t), 1e34, np.float32)


def mixed_t_max(first_hit, seed):
    """One kind per ray, in a fixed random order: (t_max, kind index per ray)."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, len(T_MAX_KINDS), len(first_hit))
    t = np.empty(len(first_hit), np.float32)
    for k, name in enumerate(T_MAX_KINDS):
        t[kind == k] = t_max_for(first_hit, name)[kind == k]
    return t, kind


def terrain_rays(n, seed=17, extent=45.0):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    o[:, 1] = rng.uniform(2.0, 30.0, n)
    d = rng.normal(size=(n, 3))
    d[:, 1] = -np.abs(d[:, 1]) - 0.05
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
