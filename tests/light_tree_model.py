"""float64 model of the light tree (csrc/light_tree.h, rt_core.h lt_importance / lt_sample / lt_pick_prob; formulas:
include/rfwhip.h).  It walks the tree the context built (CoreBinding.get_light_tree) and restates the
importance with inverse functions — asin and acos where the kernel uses sine and cosine identities — so that it shares no
arithmetic with the code under test.  Also the reference's potentials (rt_core.h pot_*) in float64, and the checks of the
tree's invariants."""
import math

import numpy as np

COS_SLACK = 1e-5   # rt_core.h LT_COS_SLACK
R2_FLOOR = 1e-12   # rt_core.h LT_R2_FLOOR


def _unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-300)


def _bound(theta):
    """cos of a clipped angle: 1 at 0, cos + slack cut off at 0 otherwise"""
    return np.where(theta <= 0.0, 1.0, np.maximum(0.0, np.cos(np.minimum(theta, math.pi)) + COS_SLACK))


def importance(node, I, N):
    """The importance of one node (a record of LIGHT_TREE_NODE_DTYPE) for points I (k x 3) with normals N (k x 3)."""
    lo, hi = node["lo"].astype(np.float64), node["hi"].astype(np.float64)
    E = float(node["energy"])
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    r2 = float(h @ h)
    v = I - c
    d2 = (v * v).sum(-1)
    inside = ~(d2 > r2)
    d = np.sqrt(np.where(inside, 1.0, d2))
    theta_u = np.arcsin(np.minimum(1.0, math.sqrt(r2) / d))
    w = v / d[:, None]
    if float(node["cos_o"]) > -1.0:
        theta_o = math.acos(min(1.0, float(node["cos_o"])))
        theta = np.arccos(np.clip(w @ node["axis"].astype(np.float64), -1.0, 1.0))
        t_o = _bound(theta - theta_o - theta_u)
    else:
        t_o = np.ones(len(I))
    theta_i = np.arccos(np.clip(-(N * w).sum(-1), -1.0, 1.0))
    t_i = _bound(theta_i - theta_u)
    return np.where(inside, E / max(r2, R2_FLOOR), E * t_o * t_i / np.where(inside, 1.0, d2))


def pot_dir(dirs, N):
    """rt_core.h pot_dir for every directional light: k x n_dir"""
    if not len(dirs):
        return np.zeros((len(N), 0))
    return dirs["energy"].astype(np.float64)[None, :] * np.maximum(0.0, -(N @ dirs["direction"].astype(np.float64).T))


def light_probabilities(nodes, n_spatial, dirs, I, N):
    """The probability of every light (k x (n_spatial + n_dir)) under lt_sample's rule, and the mass that ends nowhere (k): a node
    with a positive importance whose children both have none."""
    k = len(I)
    pd = pot_dir(dirs, N)
    out = np.zeros((k, n_spatial + len(dirs)))
    lost = np.zeros(k)
    w_root = importance(nodes[0], I, N) if n_spatial else np.zeros(k)
    total = w_root + pd.sum(-1)
    ok = total > 0
    safe = np.where(ok, total, 1.0)
    out[:, n_spatial:] = np.where(ok[:, None], pd / safe[:, None], 0.0)
    if not n_spatial:
        return out, lost
    reach = np.zeros((len(nodes), k))
    reach[0] = np.where(ok, w_root / safe, 0.0)
    for i, nd in enumerate(nodes):  # (breadth-first placement: a parent comes before its children)
        if i == 1 or not nd["count"]:
            continue
        if nd["child"] == 0:
            out[:, nd["light"]] = reach[i]
            continue
        a, b = int(nd["child"]), int(nd["child"]) + 1
        wl, wr = importance(nodes[a], I, N), importance(nodes[b], I, N)
        s = wl + wr
        dead = ~(s > 0)
        lost += np.where(dead, reach[i], 0.0)
        s = np.where(dead, 1.0, s)
        reach[a], reach[b] = reach[i] * np.where(dead, 0.0, wl / s), reach[i] * np.where(dead, 0.0, wr / s)
    return out, lost


def sample(nodes, n_spatial, dirs, I, N, r1):
    """lt_sample's walk for ONE point in float64: the light r1 draws (-1: none) and its probability."""
    I, N = np.asarray(I, np.float64).reshape(1, 3), np.asarray(N, np.float64).reshape(1, 3)
    pd = pot_dir(dirs, N)[0]
    w_root = float(importance(nodes[0], I, N)[0]) if n_spatial else 0.0
    total = w_root + pd.sum()
    if not total > 0:
        return -1, 0.0
    x = r1 * total
    if not (w_root > 0 and (x < w_root or not pd.sum() > 0)):
        acc, pick = 0.0, -1
        for k, p in enumerate(pd):
            if p > 0:
                pick, acc = k, acc + p
                if acc >= x - w_root:
                    break
        return (n_spatial + pick, pd[pick] / total) if pick >= 0 else (-1, 0.0)
    q, u, i = w_root / total, min(x / w_root, 1.0 - 2.0 ** -53), 0
    while nodes[i]["child"] != 0:
        a = int(nodes[i]["child"])
        wl, wr = float(importance(nodes[a], I, N)[0]), float(importance(nodes[a + 1], I, N)[0])
        if not wl + wr > 0:
            return -1, 0.0
        pl = wl / (wl + wr)
        if u < pl:
            q, u, i = q * pl, u / pl, a
        else:
            q, u, i = q * (1.0 - pl), (u - pl) / max(1.0 - pl, 1e-300), a + 1
    return int(nodes[i]["light"]), q


def pot_area(area, I, N, P=None):
    """rt_core.h pot_area in float64 for every area light at its point P (default: its centroid): k x n_area"""
    P = area["position"].astype(np.float64) if P is None else P
    L = P[None, :, :] - I[:, None, :]
    att = 1.0 / np.maximum((L * L).sum(-1), 1e-300)
    L = _unit(L)
    ln = np.maximum(0.0, -(L * area["normal"].astype(np.float64)[None]).sum(-1))
    nl = np.maximum(0.0, (L * N[:, None, :]).sum(-1))
    return area["energy"].astype(np.float64)[None] * ln * nl * att


# ---------------------------------------------------------------------------------------------------------------------------
# invariants of a downloaded tree
# ---------------------------------------------------------------------------------------------------------------------------
def light_geometry(area, point, spot):
    """Per spatial light, in pot_any's order: box lo, hi (n x 3), energy as the tree counts it, unit normal or None-mask."""
    lo, hi, e, nrm, has_n = [], [], [], [], []
    for l in area:
        v = np.stack([l["vertex0"], l["vertex1"], l["vertex2"]]).astype(np.float64)
        lo.append(v.min(0)), hi.append(v.max(0)), e.append(float(l["energy"]))
        n = l["normal"].astype(np.float64)
        nrm.append(n / np.linalg.norm(n)), has_n.append(True)
    for l in list(point) + list(spot):
        p = l["position"].astype(np.float64)
        lo.append(p), hi.append(p), e.append(float(l["energy"])), nrm.append(np.zeros(3)), has_n.append(False)
    e = np.array(e, np.float64)
    e = np.where(e > 0, e, 0.0)  # (negative or NaN: 0)
    return np.array(lo).reshape(-1, 3), np.array(hi).reshape(-1, 3), e, np.array(nrm).reshape(-1, 3), np.array(has_n, bool)


def check_tree(nodes, paths, area, point, spot, n_dir):
    """Every invariant DESIGN.md section 12 states; raises AssertionError naming the first that fails."""
    n = len(area) + len(point) + len(spot)
    assert len(paths) == n + n_dir
    if n == 0:
        assert len(nodes) == 0
        return
    assert len(nodes) == (1 if n == 1 else 2 * n)
    lo, hi, e, nrm, has_n = light_geometry(area, point, spot)
    seen = np.zeros(n, int)
    max_depth = 0
    # (node, depth, bits, ancestors)
    stack = [(0, 0, 0, [])]
    while stack:
        i, depth, bits, anc = stack.pop()
        nd = nodes[i]
        chain = anc + [i]
        if nd["child"] == 0:
            li = int(nd["light"])
            assert li < n and nd["count"] == 1
            seen[li] += 1
            max_depth = max(max_depth, depth)
            assert paths[li]["depth"] == depth and paths[li]["bits"] == bits, "path bits lead to the leaf"
            assert np.all(nd["lo"] <= lo[li]) and np.all(nd["hi"] >= hi[li]), "a leaf's box holds its light"
            assert abs(float(nd["energy"]) - e[li]) <= 1e-6 * max(1.0, e[li])
            for a in chain:  # the leaf's normal inside every cone on its path
                na = nodes[a]
                if float(na["cos_o"]) <= -1.0:
                    continue
                assert has_n[li], "a point or spot light below a node makes its cone the sphere"
                ax = na["axis"].astype(np.float64)
                ang = math.acos(max(-1.0, min(1.0, float(ax @ nrm[li]) / np.linalg.norm(ax))))
                assert ang <= math.acos(min(1.0, float(na["cos_o"]))) + 1e-6, "normal outside an ancestor's cone"
            if not has_n[li]:
                assert float(nd["cos_o"]) == -1.0
            continue
        a, b = int(nd["child"]), int(nd["child"]) + 1
        assert a % 2 == 0 and a >= 2 and b < len(nodes), "sibling pairs start at even indices"
        A, B = nodes[a], nodes[b]
        assert np.all(nd["lo"] <= np.minimum(A["lo"], B["lo"])) and np.all(nd["hi"] >= np.maximum(A["hi"], B["hi"])), "boxes contain their children"
        assert nd["count"] == A["count"] + B["count"] and A["count"] >= B["count"] >= 1 and A["count"] - B["count"] <= 1
        s = float(A["energy"]) + float(B["energy"])
        assert abs(float(nd["energy"]) - s) <= 1e-5 * max(1.0, s), "energies add up"
        assert depth < 32
        stack.append((a, depth + 1, bits, chain))
        stack.append((b, depth + 1, bits | (1 << depth), chain))
    assert np.all(seen == 1), "every spatial light sits in exactly one leaf"
    assert max_depth <= math.ceil(math.log2(n)) if n > 1 else max_depth == 0
    assert np.all(paths["depth"][n:] == 0) and np.all(paths["bits"][n:] == 0)
