"""float64 model of setting lights_follow_geometry (csrc/light_follow.h; formulas: include/rfwhip.h): the area
lights derived from triangles and transforms (system::update_area_lights, system.cpp:1003-1024), with error bounds counted from
the float32 roundings of the device's work item, and the bottom-up refit of the light tree: exact boxes, and the pairwise union of
the children's cones (Conty Estevez and Kulla 2018, Alg. 1) in float64 with inverse trigonometric functions throughout.  It
shares no arithmetic with the code under test."""
import math

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


def gamma(k):
    """k roundings in sequence (Higham): k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------------------------------------------------------------------
# refresh
# ---------------------------------------------------------------------------------------------------------------------------
def bound_mask(lights, instances):
    """instances: list (by instance index) of None (slot not in use) or a dict with `light_tri` (per triangle of its mesh:
    lightTriIdx >= 0).  A light is bound when instIdx names an instance in use, triIdx one of its triangles, and that a light triangle."""
    out = np.zeros(len(lights), bool)
    for i, l in enumerate(lights):
        ii, ti = int(l["instIdx"]), int(l["triIdx"])
        if 0 <= ii < len(instances) and instances[ii] is not None and 0 <= ti < len(instances[ii]["light_tri"]):
            out[i] = bool(instances[ii]["light_tri"][ti])
    return out


def derive(lights, instances, vertex_err=0.0, normal_err=0.0):
    """Expected geometry fields of the bound lights in float64 and the bound of each, counted from the roundings.

    instances[i]: M (4 x 4 float32 as handed to set_instance, maths convention), Nm (3 x 3 float32), verts (V x 3 float64: the
    object-space vertices, exactly — after pose or morph the float64-deformed ones), tris (T x 3 vertex indices), N (T x 3: the
    face normal of the shading record: float32 for a static mesh, float64 from the deformed vertices otherwise), light_tri (T).
    vertex_err / normal_err: bound of |device vertex - verts| and |device N - N| per coordinate (0 for a static mesh, the
    deformation's own counted roundings otherwise).

    Roundings of the work item (light_follow.h: lf_refresh_item):
      vertex_j coordinate   fma(m2, z, fma(m1, y, fl(m0 x))) + m3           4: gamma(4) (|m0 x| + |m1 y| + |m2 z| + |m3|)
      position coordinate   ((w0 + w1) + w2) * fl(1/3)                      2 sums, 1 product, 1 for the constant: gamma(4) of the
                                                                            magnitudes, plus the mean of the three vertex errors
      normal coordinate     fma(n2, Nz, fma(n1, Ny, fl(n0 Nx)))             3: gamma(3) (|n0 Nx| + |n1 Ny| + |n2 Nz|)
      area                  e1, e2 one rounding per coordinate; each cross component fma(a, b, -fl(c d)): 2 more, on top of the 2
                            of its edge factors: gamma(4) (|a b| + |c d|) per component; |cr|^2 by 3 roundings, the square root 1,
                            the half exact: gamma(4) area + |delta cr| / 2
    """
    mask = bound_mask(lights, instances)
    n = len(lights)
    exp = {k: np.zeros((n, 3)) for k in ("vertex0", "vertex1", "vertex2", "position", "normal")}
    err = {k: np.zeros((n, 3)) for k in exp}
    exp["area"], err["area"] = np.zeros(n), np.zeros(n)
    for i in np.nonzero(mask)[0]:
        inst = instances[int(lights["instIdx"][i])]
        M, Nm = inst["M"].astype(np.float64), inst["Nm"].astype(np.float64)
        tri = inst["tris"][int(lights["triIdx"][i])]
        v = inst["verts"][tri].astype(np.float64)
        w, we = [], []
        for j in range(3):
            w.append(M[:3, :3] @ v[j] + M[:3, 3])
            mag = np.abs(M[:3, :3]) @ np.abs(v[j]) + np.abs(M[:3, 3])
            we.append(gamma(4) * mag + np.abs(M[:3, :3]) @ np.full(3, vertex_err) * (1.0 + gamma(4)))
            exp["vertex%d" % j][i], err["vertex%d" % j][i] = w[j], we[j]
        exp["position"][i] = (w[0] + w[1] + w[2]) / 3.0
        err["position"][i] = (we[0] + we[1] + we[2]) / 3.0 * (1.0 + gamma(4)) + gamma(4) * (np.abs(w[0]) + np.abs(w[1]) + np.abs(w[2])) / 3.0
        N = inst["N"][int(lights["triIdx"][i])].astype(np.float64)
        exp["normal"][i] = Nm @ N
        err["normal"][i] = gamma(3) * (np.abs(Nm) @ np.abs(N)) + np.abs(Nm) @ np.full(3, normal_err) * (1.0 + gamma(3))
        e1, e2 = v[1] - v[0], v[2] - v[0]
        cr = np.cross(e1, e2)
        area = 0.5 * math.sqrt(cr @ cr)
        ea1, ea2 = np.abs(e1) + 2 * vertex_err, np.abs(e2) + 2 * vertex_err
        d1 = U * (np.abs(v[1]) + np.abs(v[0])) + 2 * vertex_err  # an edge coordinate as the device has it against the exact one
        d2 = U * (np.abs(v[2]) + np.abs(v[0])) + 2 * vertex_err
        dcr = np.zeros(3)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            prod = ea1[b] * ea2[c] + ea2[b] * ea1[c]
            dcr[a] = gamma(2) * prod + (d1[b] * ea2[c] + ea1[b] * d2[c] + d2[b] * ea1[c] + ea2[b] * d1[c]) * (1.0 + gamma(2))
        exp["area"][i] = area
        err["area"][i] = gamma(4) * area + 0.5 * math.sqrt(dcr @ dcr) * (1.0 + gamma(4))
    return mask, exp, err


# ---------------------------------------------------------------------------------------------------------------------------
# refit
# ---------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    n = math.sqrt(v @ v)
    return v / n if n > 0 else v


def cone_union(a, ta, b, tb):
    """Alg. 1 in float64: unit axes a, b, half angles ta, tb (pi: every direction) -> (axis, half angle)."""
    if tb > ta:
        a, ta, b, tb = b, tb, a, ta
    if ta >= math.pi:
        return a, math.pi
    td = math.atan2(np.linalg.norm(np.cross(a, b)), a @ b)
    if min(td + tb, math.pi) <= ta:
        return a, ta
    t = 0.5 * (ta + td + tb)
    if t >= math.pi:
        return a, math.pi
    k = np.cross(a, b)
    kl = np.linalg.norm(k)
    if not kl > 1e-300:
        return a, math.pi
    k = k / kl
    tr = t - ta
    r = a * math.cos(tr) + np.cross(k, a) * math.sin(tr)
    return _unit(r), t


def levels_of(nodes):
    """the nodes level by level (lists of indices), root first, following the child pointers"""
    if not len(nodes):
        return []
    out, cur = [], [0]
    while cur:
        out.append(cur)
        nxt = []
        for i in cur:
            c = int(nodes["child"][i])
            if c:
                nxt += [c, c + 1]
        cur = nxt
    return out


def refit(nodes, area, bound):
    """The model's bottom-up refit of `nodes` (as get_light_tree returned them) on the area lights `area` with the given binding.
    Returns touched (per node), lo / hi (float32: exact), and per node the model's cone (unit axis float64, half angle) — for an
    untouched node the stored one."""
    n = len(nodes)
    touched = np.zeros(n, bool)
    lo, hi = nodes["lo"].copy(), nodes["hi"].copy()
    axis = np.zeros((n, 3))
    theta = np.zeros(n)
    for i in range(n):
        axis[i] = _unit(nodes["axis"][i])
        c = float(nodes["cos_o"][i])
        theta[i] = math.acos(min(1.0, c)) if c > -1.0 else math.pi
    for level in reversed(levels_of(nodes)):
        for i in level:
            c = int(nodes["child"][i])
            if not c:
                k = int(nodes["light"][i])
                if k < len(area) and bound[k]:
                    touched[i] = True
                    v = np.stack([area[f][k] for f in ("vertex0", "vertex1", "vertex2")])
                    lo[i], hi[i] = v.min(0), v.max(0)
                    nrm = area["normal"][k].astype(np.float64)
                    if np.all(np.isfinite(nrm)) and np.abs(nrm).max() > 0:
                        axis[i], theta[i] = _unit(nrm / np.abs(nrm).max()), 0.0
                    else:
                        axis[i], theta[i] = np.array([0.0, 0.0, 1.0]), math.pi
            elif touched[c] or touched[c + 1]:
                touched[i] = True
                lo[i], hi[i] = np.minimum(lo[c], lo[c + 1]), np.maximum(hi[c], hi[c + 1])
                axis[i], theta[i] = cone_union(axis[c], theta[c], axis[c + 1], theta[c + 1])
    return touched, lo, hi, axis, theta


def lights_below(nodes):
    """per node the list of lights below it"""
    out = [None] * len(nodes)
    for level in reversed(levels_of(nodes)):
        for i in level:
            c = int(nodes["child"][i])
            out[i] = [int(nodes["light"][i])] if not c else out[c] + out[c + 1]
    return out


def containment_gaps(nodes, area):
    """min over every node with cos_o > -1 and every AREA light below it of (a . n - cos_o), a and n normalised in float64; a light
    with a zero or non-finite normal below a node with cos_o > -1 counts as -inf.  (Point and spot lights need cos_o = -1.)"""
    below = lights_below(nodes)
    worst = math.inf
    for i in range(len(nodes)):
        if i == 1 and len(nodes) > 1:
            continue
        c = float(nodes["cos_o"][i])
        if not c > -1.0:
            continue
        a = _unit(nodes["axis"][i])
        for k in below[i]:
            if k >= len(area):
                return -math.inf
            nrm = area["normal"][k].astype(np.float64)
            if not (np.all(np.isfinite(nrm)) and np.abs(nrm).max() > 0):
                return -math.inf
            worst = min(worst, float(a @ _unit(nrm / np.abs(nrm).max())) - c)
    return worst
