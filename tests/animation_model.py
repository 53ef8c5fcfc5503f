"""A float64 restatement of the animation rule of csrc/animation.h (include/rfwhip.h, rfwhip_animate) over the packed tables of a rig,
with a BOUND beside every value, and the rigs and checks that tests/test_animation.py (emulation) and tests/test_animation_gpu.py
(HIP kernels) share.  Nothing here reads gltf.py's classes: the model works on the tables a host hands to rfwhip_set_rig.

THE BOUND is a running error count over the shapes the header states.  A quantity is a pair (v, e): v the exact-arithmetic value in
float64, e a bound on |float32 result - v|.  u = 2^-24.  Every float32 operation of the header is one of
    R(a b)          v = a b,            e = |a| e_b + |b| e_a + e_a e_b, then one rounding
    fmaf(a, b, c)   v = a b + c,        e = (the product's) + e_c,       then one rounding
    a + b, a - b    v = a +- b,         e = e_a + e_b,                   then one rounding
    a / b           v = a / b,          e = (e_a + |v| e_b) / (|b| - e_b), then one rounding
    sqrt(a)         v = sqrt(a),        e = e_a / sqrt(a - e_a),          then one rounding
and one rounding adds u (|v| + e) (the computed value is at most |v| + e; an exact zero stays exact).  This is gamma(n) sum|terms|
carried term by term: through the samplers, the quaternion's matrix, every 4 x 4 product of the chain (matmul: an entrywise and
a normwise count, the smaller kept), the cofactors, the determinant and the divisions of the inverse.  The count treats the
errors of its operands as independent, so it is generous where they cancel (the Hermite weights near f = 1: some hundred u on a
CUBICSPLINE rotation), never too small.  float64's own error (2^-53 per operation against 2^-24) is covered by a factor
1 + 2^-20 on every bound.  Discrete steps are exact in both arithmetics: fmodf is exact, the segment search compares float32 key
times, and f <= 0 exactly when time <= t_k because t_k+1 - t_k rounds to a positive number and a difference keeps its sign.  The
two fallbacks are decided on a computed norm or determinant.  The model decides on the exact value and refuses (AssertionError)
a rig whose non-zero norm or determinant lies within four times its bound; a rig that means to fall back is built so that
float32 computes an exact zero as well (zero keys; a zero scale under an identity rotation on a root).

No measured tolerance enters: a device value passes when |value - v| <= e.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
TINY = 2.0 ** -149
CAP = 2.0 ** -12  # every bound of a test rig stays below CAP x the largest entry of its matrix (test_bounds_are_not_vacuous)
TRANSLATION, ROTATION, SCALE, WEIGHTS = 0, 1, 2, 3
STEP, LINEAR, CUBICSPLINE = 0, 1, 2
BASE_POSE = 0xFFFFFFFF
LDS_NODES, THREADS = 320, 256  # csrc/animation.h: RIG_LDS_NODES, RIG_THREADS


# ----------------------------------------------------------------------------------------------------------------------
# values with bounds
# ----------------------------------------------------------------------------------------------------------------------
class E:
    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, f64)
        self.e = np.broadcast_to(np.asarray(e, f64), self.v.shape).copy()

    f = None  # matrices out of matmul(): a bound on the Frobenius norm of each matrix's error

    def __getitem__(self, i):
        r = E(self.v[i], self.e[i])
        if self.f is not None and not isinstance(i, tuple):  # (a selection of whole matrices keeps their norm bounds)
            r.f = self.f[i]
        return r

    def __neg__(self):
        return E(-self.v, self.e)

    def twice(self):
        return E(2.0 * self.v, 2.0 * self.e)


def _e(x):
    return x if isinstance(x, E) else E(x)


def rnd(x):
    mag = np.abs(x.v) + x.e
    return E(x.v, x.e + U * mag + np.where(mag > 0, TINY, 0.0))


def _prod(a, b):
    a, b = _e(a), _e(b)
    return E(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)


def mul_r(a, b):
    return rnd(_prod(a, b))


def fma(a, b, c):
    p, c = _prod(a, b), _e(c)
    return rnd(E(p.v + c.v, p.e + c.e))


def add(a, b):
    a, b = _e(a), _e(b)
    return rnd(E(a.v + b.v, a.e + b.e))


def sub(a, b):
    return add(a, -_e(b))


def div(a, b):
    a, b = _e(a), _e(b)
    assert (np.abs(b.v) > b.e).all(), "a divisor within its own bound of zero"
    q = a.v / b.v
    return rnd(E(q, (a.e + np.abs(q) * b.e) / (np.abs(b.v) - b.e)))


def sqrt(a):
    assert (a.v > a.e).all(), "a square root within its own bound of zero"
    return rnd(E(np.sqrt(a.v), a.e / np.sqrt(a.v - a.e)))


def stack(parts, axis=-1):
    return E(np.stack([p.v for p in parts], axis), np.stack([p.e for p in parts], axis))


GAMMA4 = 4 * U / (1 - 4 * U)


def _is_affine(m):
    """Every matrix of the batch has the last row 0 0 0 1, exactly."""
    return bool((m.v[..., 3, :] == [0.0, 0.0, 0.0, 1.0]).all() and (m.e[..., 3, :] == 0.0).all())


def frob(m):
    """Bounds (..., 2) on the Frobenius norm of the error of the 3 x 3 block and on the length of the error of the translation
    column, for a batch (..., 4, 4) of affine matrices: what a product left (m.f), or the norms of the entrywise bounds."""
    f = np.stack([np.sqrt((m.e[..., :3, :3] ** 2).sum(axis=(-1, -2))), np.sqrt((m.e[..., :3, 3] ** 2).sum(axis=-1))], -1)
    return np.minimum(f, m.f) if m.f is not None else f


def matmul(a, b):
    """The PRODUCT shape of the header over (..., 4, 4) row-major [row][col] arrays: fmaf(a_r3 b_3c, fmaf(a_r2 b_2c, fmaf(a_r1 b_1c, R(a_r0 b_0c)))).
    Two bounds, both valid, the smaller kept per entry.  ENTRYWISE: the running count above.  NORMWISE, for affine factors
    A = [Ra ta; 0 1], B = [Rb tb; 0 1] (the last row of the product is then B's last row exactly: products with 0 and 1), with dRa, dta,
    dRb, dtb the errors the factors arrive with:
        ||d(Ra Rb)||_F   <= ||dRa||_F ||Rb||_2 + ||Ra||_2 ||dRb||_F + ||dRa||_F ||dRb||_F + gamma(4) || ((|A| + EA)(|B| + EB))[:3, :3] ||_F
        |d(Ra tb + ta)|  <= ||dRa||_F (|tb| + |dtb|) + ||Ra||_2 |dtb| + |dta|          + gamma(4) | ((|A| + EA)(|B| + EB))[:3, 3] |
    (the four roundings of an entry are those of a dot product of the factors as they arrive), and an entry's error is at most the
    norm of its block's.  The entrywise count grows by up to sqrt(3) per level of a hierarchy of rotations, where |R1| |R2| ...
    grows; the normwise one adds per level, because a rotation has ||R||_2 = 1 — which is why the deep chain has unit scale.  The
    result carries the two norms as .f for the next product."""
    c = mul_r(a[..., :, 0:1], b[..., 0:1, :])
    for k in (1, 2, 3):
        c = fma(a[..., :, k:k + 1], b[..., k:k + 1, :], c)
    if not (_is_affine(a) and _is_affine(b)):
        return c
    fa, fb = frob(a), frob(b)
    na, nb = np.linalg.norm(a.v[..., :3, :3], 2, axis=(-2, -1)), np.linalg.norm(b.v[..., :3, :3], 2, axis=(-2, -1))
    tb = np.sqrt((b.v[..., :3, 3] ** 2).sum(axis=-1))
    m = np.matmul(np.abs(a.v) + a.e, np.abs(b.v) + b.e)
    fr = fa[..., 0] * nb + na * fb[..., 0] + fa[..., 0] * fb[..., 0] + GAMMA4 * np.sqrt((m[..., :3, :3] ** 2).sum(axis=(-1, -2)))
    ft = fa[..., 0] * (tb + fb[..., 1]) + na * fb[..., 1] + fa[..., 1] + GAMMA4 * np.sqrt((m[..., :3, 3] ** 2).sum(axis=-1))
    c.f = np.stack([fr, ft], -1) * SLACK + 64 * TINY
    c.e[..., 3, :] = 0.0
    c.e[..., :3, :3] = np.minimum(c.e[..., :3, :3], c.f[..., 0, None, None])
    c.e[..., :3, 3] = np.minimum(c.e[..., :3, 3], c.f[..., 1, None])
    return c


def within(got, want):
    """Every float32 value of `got` lies within the bound of the model's `want`."""
    got = np.asarray(got, f64)
    assert got.shape == want.v.shape, (got.shape, want.v.shape)
    bad = ~(np.abs(got - want.v) <= want.e * SLACK)
    assert not bad.any(), (int(bad.sum()), float(np.abs(got - want.v)[bad].max()), float(want.e[bad].max()))


# ----------------------------------------------------------------------------------------------------------------------
# the rule
# ----------------------------------------------------------------------------------------------------------------------
def width(rig, ch):
    return 4 if ch["path"] == ROTATION else int(rig["nodes"][ch["node"]]["weight_count"]) if ch["path"] == WEIGHTS else 3


def wrap(time, duration):
    time = float(f32(time))
    return math.fmod(time, duration) if time > duration and duration > 0 else time


def sample(rig, c, time, time_ulps=0):
    """Channel c at `time` -> (E of the channel's width, 1 when a rotation fell back to the identity, the wrapped time).
    time_ulps: the time is a float32 rounding of what the comparison's other side was evaluated at — that many u |time| of error on
    it (the wrap and the segment are taken to be the same on both sides)."""
    time_err = time_ulps * U * abs(float(f32(time)))
    ch = rig["channels"][c]
    n, w = int(ch["key_count"]), width(rig, ch)
    t = rig["times"][ch["time_offset"]:ch["time_offset"] + n].astype(f64)
    val = rig["values"][ch["value_offset"]:ch["value_offset"] + ch["value_count"]].astype(f64)
    cubic, scalar = ch["method"] == CUBICSPLINE, ch["path"] == WEIGHTS
    # (key, part, component) with part = in-tangent, value, out-tangent for CUBICSPLINE; a weights key holds the parts per target
    if cubic:
        keys = val.reshape(n, w, 3).transpose(0, 2, 1) if scalar else val.reshape(n, 3, w)
    else:
        keys = val.reshape(n, 1, w)
    value = 1 if cubic else 0
    time = wrap(time, t[-1])
    k = int((time > t[1:n - 1]).sum()) if n > 2 else 0
    if n == 1 or time <= t[k]:
        out = E(keys[0, value])
    elif ch["method"] == STEP:
        out = E(keys[k, value])
    else:
        d = sub(t[k + 1], t[k])
        f = div(sub(E(time, time_err), t[k]), d)
        a, b = E(keys[k, value]), E(keys[k + 1, value])
        if ch["method"] == LINEAR:
            out = fma(f, b, mul_r(sub(1.0, f), a))
        else:
            t2 = mul_r(f, f)
            t3 = mul_r(t2, f)
            m0, m1 = mul_r(d, keys[k, 2]), mul_r(d, keys[k + 1, 0])
            h10 = add(fma(-2.0, t2, t3), f)
            h00 = fma(2.0, t3, fma(-3.0, t2, 1.0))
            h01 = fma(-2.0, t3, mul_r(3.0, t2))
            h11 = sub(t3, t2)
            out = fma(m1, h11, fma(b, h01, fma(a, h00, mul_r(m0, h10))))
    if ch["path"] != ROTATION:
        return out, 0, time
    n2 = fma(out[3], out[3], fma(out[2], out[2], fma(out[1], out[1], mul_r(out[0], out[0]))))
    if n2.v == 0.0 or not np.isfinite(n2.v):  # (decided on the exact value: see the module's note on the fallbacks)
        return E([0.0, 0.0, 0.0, 1.0]), 1, time
    assert n2.v > 4 * n2.e, "the fallback decision lies within the norm's bound"
    length = sqrt(n2)
    return div(out, E(np.full(4, length.v), np.full(4, length.e))), 0, time


def local_matrices(rig, trs):
    """local = T R S M for every node: (N, 4, 4) row-major."""
    x, y, z, w = (trs[:, 3 + i] for i in range(4))
    s = [trs[:, 7 + i] for i in range(3)]
    xx, yy, zz, xy, xz, yz = mul_r(x, x), mul_r(y, y), mul_r(z, z), mul_r(x, y), mul_r(x, z), mul_r(y, z)
    xw, yw, zw = mul_r(x, w), mul_r(y, w), mul_r(z, w)

    def diag(p, q):
        return sub(1.0, add(p, q).twice())
    r = [[diag(yy, zz), sub(xy, zw).twice(), add(xz, yw).twice()],
         [add(xy, zw).twice(), diag(xx, zz), sub(yz, xw).twice()],
         [sub(xz, yw).twice(), add(yz, xw).twice(), diag(xx, yy)]]
    n = len(trs.v)
    zero, one = E(np.zeros(n)), E(np.ones(n))
    rows = [stack([mul_r(r[i][0], s[0]), mul_r(r[i][1], s[1]), mul_r(r[i][2], s[2]), trs[:, i]]) for i in range(3)]
    a = stack(rows + [stack([zero, zero, zero, one])], axis=1)
    return matmul(a, rig["_matrix"])


def inverse(m):
    """The closed affine inverse of one (4, 4) row-major matrix -> (E (4, 4), 1 when it fell back to the identity)."""
    a = [[m[r, c] for c in range(3)] for r in range(3)]

    def cof(p, q, r_, s_):
        return fma(p, q, -mul_r(r_, s_))
    C = [[cof(a[1][1], a[2][2], a[1][2], a[2][1]), cof(a[1][2], a[2][0], a[1][0], a[2][2]), cof(a[1][0], a[2][1], a[1][1], a[2][0])],
         [cof(a[0][2], a[2][1], a[0][1], a[2][2]), cof(a[0][0], a[2][2], a[0][2], a[2][0]), cof(a[0][1], a[2][0], a[0][0], a[2][1])],
         [cof(a[0][1], a[1][2], a[0][2], a[1][1]), cof(a[0][2], a[1][0], a[0][0], a[1][2]), cof(a[0][0], a[1][1], a[0][1], a[1][0])]]
    det = fma(a[0][2], C[0][2], fma(a[0][1], C[0][1], mul_r(a[0][0], C[0][0])))
    # (the model decides on the exact value: a rig that means to be singular is built so that float32 computes an exact zero as
    # well — a zero scale on a root with an identity rotation — and any other rig keeps its determinant far from its bound)
    if det.v == 0.0 or not np.isfinite(det.v):
        return E(np.eye(4)), 1, det
    assert abs(det.v) > 4 * det.e, "the fallback decision lies within the determinant's bound"
    inv = [[div(C[c][r], det) for c in range(3)] for r in range(3)]
    t = [m[0, 3], m[1, 3], m[2, 3]]
    rows = [stack(inv[r] + [-fma(inv[r][2], t[2], fma(inv[r][1], t[1], mul_r(inv[r][0], t[0])))]) for r in range(3)]
    return stack(rows + [E([0.0, 0.0, 0.0, 1.0])], axis=0), 0, det


def depths(rig):
    parent = rig["nodes"]["parent"]
    d = np.zeros(len(parent), np.int64)
    for i in range(len(parent)):
        j, k = parent[i], 0
        while j >= 0:
            j, k = parent[j], k + 1
        d[i] = k
    return d


def evaluate(rig, animation, time, input_ulps=0, time_ulps=0):
    """The rig at `time` -> {"trs": E (N, 10), "weights": E, "world": E (N, 4, 4), "joints": [E (J, 4, 4) per skin], "status": ...,
    "det": [E per skin]}.  input_ulps: the base TRS, matrices, weights and inverse bind matrices are float32 roundings of what the
    comparison's other side started from — that many u |x| of error on each; time_ulps: likewise for the time (sample)."""
    nodes = rig["nodes"]
    n = len(nodes)

    def given(x):
        x = np.asarray(x, f64)
        return E(x, input_ulps * U * np.abs(x))
    trs = given(np.concatenate([nodes["translation"], nodes["rotation"], nodes["scale"]], 1))
    weights = given(rig["weights"])
    rig = dict(rig, _matrix=given(nodes["matrix"].reshape(n, 4, 4).transpose(0, 2, 1)))
    rot = 0
    status_time = float(f32(time))
    chans = range(0)
    if animation != BASE_POSE and len(rig["animations"]):
        a = rig["animations"][animation]
        chans = range(int(a["channel_offset"]), int(a["channel_offset"] + a["channel_count"]))
    for c in chans:
        ch = rig["channels"][c]
        out, fell, wrapped = sample(rig, c, time, time_ulps)
        rot += fell
        if c == chans[0]:
            status_time = wrapped
        if ch["path"] == WEIGHTS:
            o = int(nodes[ch["node"]]["weight_offset"])
            weights.v[o:o + len(out.v)], weights.e[o:o + len(out.v)] = out.v, out.e
        else:
            o = {TRANSLATION: 0, ROTATION: 3, SCALE: 7}[int(ch["path"])]
            trs.v[ch["node"], o:o + len(out.v)], trs.e[ch["node"], o:o + len(out.v)] = out.v, out.e
    local = local_matrices(rig, trs)
    world = E(local.v.copy(), local.e.copy())
    world.f = None if local.f is None else local.f.copy()
    d = depths(rig)
    for level in range(1, int(d.max()) + 1 if n else 0):
        idx = np.nonzero(d == level)[0]
        m = matmul(world[nodes["parent"][idx]], local[idx])
        world.v[idx], world.e[idx] = m.v, m.e
        if world.f is not None:
            world.f[idx] = m.f if m.f is not None else frob(m)
    joints, dets, inv_fallbacks = [], [], 0
    ibm = given(rig["inverse_bind"].reshape(-1, 4, 4).transpose(0, 2, 1))
    for sk in rig["skins"]:
        inv, fell, det = inverse(world[int(sk["mesh_node"])])
        inv_fallbacks += fell
        dets.append(det)
        sl = slice(int(sk["joint_offset"]), int(sk["joint_offset"] + sk["joint_count"]))
        wj = world[rig["joints"][sl]]
        inv_b = E(np.broadcast_to(inv.v, wj.v.shape), np.broadcast_to(inv.e, wj.v.shape))
        joints.append(matmul(matmul(inv_b, wj), ibm[sl]))
    return {"trs": trs, "weights": weights, "world": world, "local": local, "joints": joints, "det": dets,
            "status": {"time": status_time, "rotation_fallbacks": rot, "inverse_fallbacks": inv_fallbacks,
                       "animation": animation if len(chans) else BASE_POSE}}


def largest_relative_bound(ev):
    """max over the world, joint and local matrices of (largest bound of the matrix) / (largest |entry| of the matrix)."""
    worst = 0.0
    for m in [ev["world"], ev["local"]] + ev["joints"]:
        if m.v.size:
            worst = max(worst, float((m.e.max(axis=(-1, -2)) / np.abs(m.v).max(axis=(-1, -2))).max()))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# packing rigs
# ----------------------------------------------------------------------------------------------------------------------
def node(parent=-1, t=(0, 0, 0), r=(0, 0, 0, 1), s=(1, 1, 1), m=None, weights=()):
    return dict(parent=parent, t=t, r=r, s=s, m=np.eye(4) if m is None else np.asarray(m, f64), weights=list(weights))


def channel(node_index, path, method, times, values):
    return dict(node=node_index, path=path, method=method, times=np.asarray(times, f32).reshape(-1), values=np.asarray(values, f32).reshape(-1))


def pack(pkg, nodes, skins=(), animations=()):
    """nodes: node(...) dicts; skins: (mesh_node, [joint nodes], inverse bind matrices (J, 4, 4) row-major or None); animations:
    lists of channel(...) dicts -> the tables of abi.RIG_TABLES."""
    abi = pkg.abi
    nd = np.zeros(len(nodes), abi.RIG_NODE_DTYPE)
    weights = []
    for i, x in enumerate(nodes):
        nd[i]["parent"], nd[i]["translation"], nd[i]["rotation"], nd[i]["scale"] = x["parent"], x["t"], x["r"], x["s"]
        nd[i]["matrix"] = np.asarray(x["m"], f64).T.reshape(-1)
        nd[i]["weight_offset"], nd[i]["weight_count"] = len(weights), len(x["weights"])
        weights += x["weights"]
    sk = np.zeros(len(skins), abi.RIG_SKIN_DTYPE)
    joints, ibm = [], []
    for i, (mesh_node, js, mats) in enumerate(skins):
        sk[i]["mesh_node"], sk[i]["joint_offset"], sk[i]["joint_count"] = mesh_node, len(joints), len(js)
        joints += list(js)
        mats = np.tile(np.eye(4), (len(js), 1, 1)) if mats is None else np.asarray(mats, f64).reshape(-1, 4, 4).copy()
        mats[:, 3, :] = [0.0, 0.0, 0.0, 1.0]  # (affine, exactly: an inverse computed in float64 may leave 1e-17 there)
        ibm.append(mats.transpose(0, 2, 1).reshape(-1))
    an = np.zeros(len(animations), abi.RIG_ANIMATION_DTYPE)
    chans, times, values = [], [], []
    nt = nv = 0
    for i, a in enumerate(animations):
        an[i]["channel_offset"], an[i]["channel_count"] = len(chans), len(a)
        for c in a:
            chans.append((c["node"], c["path"], c["method"], len(c["times"]), nt, nv, len(c["values"]), 0))
            times.append(c["times"]), values.append(c["values"])
            nt, nv = nt + len(c["times"]), nv + len(c["values"])
    ch = np.zeros(len(chans), abi.RIG_CHANNEL_DTYPE)
    for i, c in enumerate(chans):
        ch[i] = c

    def cat(parts):
        return np.concatenate(parts).astype(f32) if parts else np.zeros(0, f32)
    return {"nodes": nd, "weights": np.asarray(weights, f32), "skins": sk, "joints": np.asarray(joints, np.uint32), "inverse_bind": cat(ibm),
            "animations": an, "channels": ch, "times": cat(times), "values": cat(values)}


# ----------------------------------------------------------------------------------------------------------------------
# the test rigs: unit scale on the deep chain, scales within [0.5, 2] elsewhere, the mesh node's |det| within [1/8, 8]
# ----------------------------------------------------------------------------------------------------------------------
def _quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _key_values(rng, path, w):
    if path == ROTATION:
        return _quat(rng)
    if path == SCALE:
        return rng.uniform(0.75, 1.3, w)
    return rng.uniform(-1.0, 1.0, w)


def _channel(rng, node_index, path, method, times, w):
    """Keys of a channel; CUBICSPLINE tangents are small, so that a spline of scales stays inside [0.5, 2]."""
    rows = []
    for _ in times:
        v = _key_values(rng, path, w)
        if method == CUBICSPLINE:
            tin, tout = rng.uniform(-0.2, 0.2, w), rng.uniform(-0.2, 0.2, w)
            rows.append(np.stack([tin, v, tout], 1).reshape(-1) if path == WEIGHTS else np.concatenate([tin, v, tout]))
        else:
            rows.append(v)
    return channel(node_index, path, method, times, np.concatenate(rows))


KEY_TIMES = {1: [0.5], 2: [0.25, 1.5], 4: [0.125, 0.5, 1.25, 2.0]}
PATHS = (TRANSLATION, ROTATION, SCALE, WEIGHTS)
METHODS = (STEP, LINEAR, CUBICSPLINE)


def sampling_rig(pkg, key_count, times=None, seed=1):
    """Twelve nodes under one root, one per (path, method), each with its channel of `key_count` keys; every node has two morph
    weights.  One skin over all of them hangs on the root."""
    rng = np.random.default_rng(seed + key_count)
    times = KEY_TIMES[key_count] if times is None else times
    nodes = [node(weights=[0.25, 0.5])]
    chans = []
    for p in PATHS:
        for m in METHODS:
            nodes.append(node(parent=0, t=rng.uniform(-1, 1, 3), r=_quat(rng), s=rng.uniform(0.6, 1.6, 3), weights=[0.125, 0.75]))
            chans.append(_channel(rng, len(nodes) - 1, p, m, times, 2 if p == WEIGHTS else 4 if p == ROTATION else 3))
    return pack(pkg, nodes, [(0, list(range(1, len(nodes))), None)], [chans])


def sampling_times(key_count, times=None):
    """Below the first key, on it, between keys, on an inner key, on the last key, past it (wraps), far past it."""
    t = KEY_TIMES[key_count] if times is None else times
    out = [t[0] - 0.25, t[0], t[-1], t[-1] * 1.375, t[-1] * 2.5, 0.0]
    for a, b in zip(t[:-1], t[1:]):
        out += [0.5 * (a + b), b, float(np.nextafter(f32(b), f32(np.inf)))]
    return [float(f32(x)) for x in out]


def zero_duration_rig(pkg):
    """Key times that end at 0: duration == 0 never wraps; a time past the last key holds the last segment's f > 1 extrapolation."""
    return sampling_rig(pkg, 2, times=[-1.0, 0.0], seed=7)


def many_channels_rig(pkg, count=65):
    """`count` translation channels on `count` nodes under one root (more than one wave of channels)."""
    rng = np.random.default_rng(65)
    nodes = [node()] + [node(parent=0, t=rng.uniform(-1, 1, 3)) for _ in range(count)]
    chans = [_channel(rng, 1 + i, TRANSLATION, METHODS[i % 3], KEY_TIMES[4], 3) for i in range(count)]
    return pack(pkg, nodes, [(0, [1, count], None)], [chans])


def zero_quaternion_rig(pkg):
    """Rotation channels whose keys are zero quaternions (STEP, LINEAR, CUBICSPLINE): three fallbacks; a fourth channel is sound."""
    nodes = [node()] + [node(parent=0) for _ in range(4)]
    t = [0.0, 1.0]
    chans = [channel(1, ROTATION, STEP, t, np.zeros(8)), channel(2, ROTATION, LINEAR, t, np.zeros(8)),
             channel(3, ROTATION, CUBICSPLINE, t, np.zeros(24)), channel(4, ROTATION, LINEAR, t, [0, 0, 0, 1, 0, 1, 0, 0])]
    return pack(pkg, nodes, [(0, [1, 2, 3, 4], None)], [chans])


def hierarchy_rig(pkg, kind, seed=3):
    """kind: "one" 1 node; "roots" 3 roots with a child each; "reversed" children listed before their parents; "chain" depth 40 at
    unit scale; or a node count: a random forest of that many nodes, depth <= 6.  The nodes carry rotation channels, a skin over
    (up to 8 of) the nodes hangs on the first root."""
    rng = np.random.default_rng(seed)

    def rnode(parent, unit=False):
        # (the chain's steps are short: a rotation's error moves everything below it by that angle times the distance, and the
        # bound adds those up over forty levels)
        reach = 0.1 if kind == "chain" else 0.5
        return node(parent=parent, t=rng.uniform(-reach, reach, 3), r=_quat(rng), s=(1, 1, 1) if unit else rng.uniform(0.8, 1.25, 3))
    if kind == "one":
        nodes = [rnode(-1)]
    elif kind == "roots":
        nodes = [rnode(-1), rnode(-1), rnode(-1), rnode(0), rnode(1), rnode(2)]
    elif kind == "reversed":
        nodes = [rnode(i + 1) for i in range(5)] + [rnode(-1)]
    elif kind == "chain":
        nodes = [rnode(i - 1, unit=True) for i in range(41)]
    else:
        nodes, depth = [rnode(-1)], [0]
        while len(nodes) < int(kind):
            p = int(rng.integers(len(nodes)))
            if depth[p] < 6:
                nodes.append(rnode(p, unit=depth[p] >= 3))
                depth.append(depth[p] + 1)
    # (every node of a forest turns; of the deep chain every twentieth: a sampled rotation's matrix carries some hundred u, a given
    # one five, and the chain adds up forty of them)
    chans = [_channel(rng, i, ROTATION, LINEAR, KEY_TIMES[2], 4) for i in range(len(nodes)) if kind != "chain" or i % 20 == 0]
    joints = sorted(set([0, len(nodes) - 1] + [int(j) for j in rng.integers(0, len(nodes), 6)]))
    ibm = [np.linalg.inv(_affine(rng)) for _ in joints]
    root = [i for i, x in enumerate(nodes) if x["parent"] < 0][0]  # (the mesh node: a root, whose inverse is well conditioned)
    return pack(pkg, nodes, [(root, joints, ibm)], [chans])


def _affine(rng, scale=(0.7, 1.4)):
    m = np.eye(4)
    q = _quat(rng)
    x, y, z, w = q
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    m[:3, :3] = r * rng.uniform(scale[0], scale[1], 3)[None, :]
    m[:3, 3] = rng.uniform(-0.5, 0.5, 3)
    return m


def skin_rig(pkg, kind, seed=11):
    """kind: 1 or 65 joints on one skin; "two" two skins in one rig (3 and 5 joints, other mesh nodes); "animated" the mesh node
    itself rotates, translates and scales; "singular" the second skin's mesh node has scale (1, 0, 1): its inverse falls back."""
    rng = np.random.default_rng(seed)

    def rnode(parent, **kw):
        return node(parent=parent, t=rng.uniform(-0.5, 0.5, 3), r=_quat(rng), s=rng.uniform(0.75, 1.3, 3), **kw)
    if kind in (1, 65):
        nodes = [rnode(-1), rnode(0)] + [rnode(1 + int(rng.integers(0, min(1 + i, 3)))) for i in range(kind)]  # (depth <= 4)
        js = list(range(2, 2 + kind))
        skins = [(1, js, [np.linalg.inv(_affine(rng)) for _ in js])]
        chans = [_channel(rng, j, (TRANSLATION, ROTATION, SCALE)[j % 3], METHODS[j % 3], KEY_TIMES[4], 4 if j % 3 == 1 else 3) for j in js]
    else:
        nodes = [rnode(-1), rnode(0), rnode(0), rnode(1), rnode(3), rnode(2), rnode(5), rnode(6)]
        if kind == "singular":
            nodes[2] = node(parent=-1, s=(1.0, 0.0, 1.0))
        skins = [(1, [3, 4, 0], [np.linalg.inv(_affine(rng)) for _ in range(3)]), (2, [5, 6, 7, 1, 4], [np.linalg.inv(_affine(rng)) for _ in range(5)])]
        chans = [_channel(rng, j, ROTATION, CUBICSPLINE if j == 7 else LINEAR, KEY_TIMES[4], 4) for j in (3, 4, 5, 6, 7)]
        if kind == "animated":
            chans += [_channel(rng, 1, ROTATION, LINEAR, KEY_TIMES[4], 4), _channel(rng, 1, TRANSLATION, CUBICSPLINE, KEY_TIMES[4], 3),
                      _channel(rng, 1, SCALE, LINEAR, KEY_TIMES[4], 3)]
    return pack(pkg, nodes, skins, [chans])


def all_rigs(pkg):
    """name -> (rig, times): every rig of the sampling, hierarchy and skin lists."""
    out = {}
    for kc in (1, 2, 4):
        out["sampling %d keys" % kc] = (sampling_rig(pkg, kc), sampling_times(kc))
    out["duration 0"] = (zero_duration_rig(pkg), [-1.5, -1.0, -0.5, 0.0, 0.75])
    out["65 channels"] = (many_channels_rig(pkg), [0.3, 1.25, 4.5])
    out["zero quaternions"] = (zero_quaternion_rig(pkg), [0.0, 0.5, 1.0])
    for kind in ("one", "roots", "reversed", "chain", 65, 300, LDS_NODES, LDS_NODES + 1):
        out["hierarchy %s" % kind] = (hierarchy_rig(pkg, kind), [0.7])
    for kind in (1, 65, "two", "animated", "singular"):
        out["skin %s" % kind] = (skin_rig(pkg, kind), [0.9, 3.1])
    return out


# ----------------------------------------------------------------------------------------------------------------------
# checks on a context (the emulation or the HIP kernels)
# ----------------------------------------------------------------------------------------------------------------------
def read_all(ctx, rig, index=0):
    """Everything rfwhip_read_rig returns for rig `index`, as arrays."""
    out = {"trs": ctx.read_rig(index, "trs"), "world": ctx.read_rig(index, "world"), "status": ctx.read_rig(index, "status"),
           "joints": [ctx.read_rig(index, "joints", s) for s in range(len(rig["skins"]))],
           "weights": np.concatenate([ctx.read_rig(index, "weights", i) for i in range(len(rig["nodes"]))] + [np.zeros(0, f32)])}
    return out


def same_bits(a, b):
    assert a["status"] == b["status"], (a["status"], b["status"])
    for k in ("trs", "world", "weights"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    for x, y in zip(a["joints"], b["joints"]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "joints"


def check_against_model(got, rig, animation, time, serial=None):
    want = evaluate(rig, animation, time)
    within(got["trs"], want["trs"])
    within(got["world"], want["world"])
    # (the weights table is read node by node in node order, which is the table's order for pack()'s rigs)
    within(got["weights"], want["weights"])
    for g, w in zip(got["joints"], want["joints"]):
        within(g, w)
    st = dict(got["status"])
    if serial is not None:
        assert st["serial"] == serial, st
    st.pop("serial")
    assert st == want["status"], (st, want["status"])
    return want


def run_rig(ctx, rig, times, animation=0, index=0):
    """set_rig, then animate at every time: each read-back within the model's bound; returns the read-backs."""
    ctx.set_rig(index, rig)
    out = []
    for k, t in enumerate(times):
        ctx.animate(index, t, animation)
        got = read_all(ctx, rig, index)
        check_against_model(got, rig, animation if len(rig["animations"]) else BASE_POSE, t, serial=k + 1)
        out.append(got)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# rigs that drive meshes: the skinned tube of scenes.skinned_tube_rig, and a two-target morph of an emissive strip
# ----------------------------------------------------------------------------------------------------------------------
def tube_rig(pkg):
    """Node 0 the mesh node, joint 1 the root bone, joint 2 the bone that bends the upper half about (0, 4, 0): a rotation channel
    about z (CUBICSPLINE) and a small translation channel (LINEAR)."""
    def qz(deg):
        a = math.radians(deg) / 2
        return [0.0, 0.0, math.sin(a), math.cos(a)]
    nodes = [node(), node(parent=0), node(parent=1, t=(0.0, 4.0, 0.0))]
    lift = np.eye(4)
    lift[1, 3] = -4.0
    keys = np.concatenate([np.concatenate([np.zeros(4), qz(d), np.zeros(4)]) for d in (0.0, 35.0, -20.0)])
    chans = [channel(2, ROTATION, CUBICSPLINE, [0.0, 1.0, 2.0], keys),
             channel(2, TRANSLATION, LINEAR, [0.0, 2.0], [0.0, 4.0, 0.0, 0.25, 4.0, 0.0])]
    return pack(pkg, nodes, [(0, [1, 2], [np.eye(4), lift])], [chans])


def tube_contexts(pkg, make, count, rings=12, seg=10, w=96, h=64):
    """`count` contexts with the tube scene resident and skinned, pt at 4 spp -> (scene, contexts)."""
    scene = pkg.scenes.skinned_tube(0.0, rings=rings, seg=seg, width=w, height=h)
    v, idx, vn, joints, weights = pkg.scenes.skinned_tube_rig(rings, seg)
    scene.meshes[0]["triangles"] = pkg.scenes.make_triangles(v, idx, normals=vn, material=scene.meshes[0]["triangles"]["material"][0])
    out = []
    for _ in range(count):
        c = make()
        c.init(w, h)
        scene.upload(c)
        c.set_setting("integrator", "pt")
        c.set_setting("spp", 4)
        c.set_mesh_skin(0, joints, weights, vn)
        out.append(c)
    return scene, out


def tube_rays():
    """A fixed fan of rays at the tube from the camera's side, and a few that miss."""
    ys, xs = np.meshgrid(np.linspace(0.2, 8.5, 24), np.linspace(-2.5, 2.5, 16), indexing="ij")
    target = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(xs.size)], 1)
    org = np.tile(np.array([0.3, 5.0, -14.0]), (len(target), 1))
    d = target - org
    return org.astype(f32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def same_scene_bits(pkg, scene, a, b):
    """Two contexts hold the same geometry: the same hits on the fixed rays and the same 96 x 64 image, bit for bit."""
    org, d = tube_rays()
    ha, hb = a.trace_rays(org, d), b.trace_rays(org, d)
    assert (ha["prim"] >= 0).sum() > 50
    for k in ha:
        assert np.array_equal(ha[k].view(np.uint32), hb[k].view(np.uint32)), k
    a.render_frame(scene.camera, pkg.RESET)
    b.render_frame(scene.camera, pkg.RESET)
    ia, ib = a.framebuffer(), b.framebuffer()
    assert np.isfinite(ia).all() and ia[..., :3].mean() > 1e-3
    assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))


def animate_equals_pose(pkg, make, time=1.4):
    """Context A animates; context B is posed with the joint matrices read back from A: the same hits, the same image."""
    scene, (a, b) = tube_contexts(pkg, make, 2)
    rig = tube_rig(pkg)
    a.set_rig(0, rig)
    a.bind_rig(0, 0, skin=0)
    a.animate(0, time)
    a.update()
    mats = a.read_rig(0, "joints", 0)
    within(mats, evaluate(rig, 0, time)["joints"][0])
    assert np.abs(mats[1] - np.eye(4)).max() > 0.1  # (the bone moved: the pose is not the bind pose)
    b.pose_mesh(0, mats)
    b.update()
    same_scene_bits(pkg, scene, a, b)
    return scene, a, b


def strip_rig(pkg):
    """One node with two morph weights and a CUBICSPLINE weights channel (three keys, the interleaved layout)."""
    keys = [0.1, 0.0, -0.1, 0.0, 0.0, 0.2,  -0.2, 0.75, 0.1, 0.1, -0.4, 0.0,  0.0, 0.2, 0.0, 0.0, 0.5, 0.0]
    return pack(pkg, [node(weights=[0.0, 0.0])], [], [[channel(0, WEIGHTS, CUBICSPLINE, [0.0, 1.0, 2.5], keys)]])
