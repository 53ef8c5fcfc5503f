"""float64 model of the primary wave's entry snapshot pass (csrc/primary_entry.h), and the per-ray walk its records are held to.

The pass, per 64-slot group of the first sample group of the slot layout (world 1: local rows are image rows): the pyramid of the
group's pixel rectangle — apex cam.pos, four inward unit normals, no difference of nearly equal corners —, the candidate list that
starts as {root} and replaces its top, while that is an inner node, by the children the pyramid may touch (first child on top),
drops a top without touched children, and stops at the first leaf on top or when the list would outgrow K.  Every product and sum
below is one IEEE double operation in the order of the header, so the records must equal the item's word for word.

coverage(): the walk from the ROOT with real rays of the group — an exact float64 slab test, closed (a ray that grazes a box enters
it) — counts the nodes it enters that neither lie under an entry of the record nor were expanded by the pass.  That count must be 0."""
import numpy as np

from primary_order_model import ENTRY_EMPTY, NODE4F  # noqa: F401

ENTRY_LEAF, ENTRY_DONE, ENTRY_INDEX_MASK = 0x80000000, 0xFFFFFFFE, 0x3FFFFFFF
THETA0, THETA1, BETA = 2.0 ** -18, 2.0 ** -21, 2.0 ** -19


def _pix_xy(pix):
    return (pix & 1) | ((pix >> 1) & 2) | ((pix >> 2) & 4), ((pix >> 1) & 1) | ((pix >> 2) & 2) | ((pix >> 3) & 4)


def group_pixels(W, H, g, group):
    """The pixels (x, y) of a group that lie in the image (world 1)."""
    tiles_x = (W + 7) // 8
    tile, pix0 = (group * 64) // (64 * g), ((group * 64) // g) % 64
    ty, tx = divmod(tile, tiles_x)
    out = []
    for j in range(64 // g):
        px, py = _pix_xy(pix0 + j)
        x, y = tx * 8 + px, ty * 8 + py
        if x < W and y < H:
            out.append((x, y))
    return out


def groups_of(W, H, g):
    return ((W + 7) // 8) * ((H + 7) // 8) * 64 * g // 64


class View:
    """pos, p1, right, up (float32 vectors), inv_w, inv_h (float32)"""
    def __init__(self, pos, p1, right, up, inv_w, inv_h):
        self.pos, self.p1, self.right, self.up = (np.asarray(v, np.float32).astype(np.float64) for v in (pos, p1, right, up))
        self.inv_w, self.inv_h = float(np.float32(inv_w)), float(np.float32(inv_h))


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def pyramid(view, pixels):
    """None: no pixel; else dict(ok, c, n[4], theta, c1)."""
    if not pixels:
        return None
    xs, ys = [p[0] for p in pixels], [p[1] for p in pixels]
    u0, u1 = float(min(xs)) * view.inv_w, (float(max(xs)) + 1.0) * view.inv_w
    v0, v1 = float(min(ys)) * view.inv_h, (float(max(ys)) + 1.0) * view.inv_h
    c, rt, up = view.pos, view.right, view.up
    q = view.p1 - c
    a = [q + rt * u0, q + rt * u1, q + up * v0, q + up * v1]
    ru = _cross(rt, up)
    with np.errstate(all="ignore"):
        area, triple = np.sqrt(_dot(ru, ru)), _dot(ru, q)
        d = np.float64(abs(triple)) / area
        sk = ((np.abs(view.p1) + np.abs(rt)) + np.abs(up)) + np.abs(c)
        S = np.sqrt(_dot(sk, sk))
        py = {"ok": False, "c": c, "c1": abs(c[0]) + abs(c[1]) + abs(c[2]), "theta": THETA0 + (THETA1 * S) / d}
    if not (d > 0.0) or not (py["theta"] < 0.125):
        return py
    s = 1.0 if triple > 0.0 else -1.0
    n = []
    for j, sg in enumerate((s, -s, -s, s)):
        m = _cross(up if j < 2 else rt, a[j])
        ln = np.sqrt(_dot(m, m))
        if not (ln > 0.0):
            return py
        n.append((m * sg) / ln)
    py["n"], py["ok"] = n, True
    return py


def touched(py, lo, hi):
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    if (lo > hi).any():
        return False
    d0, d1 = lo - py["c"], hi - py["c"]
    m = np.maximum(d0 * d0, d1 * d1)
    r2 = (0.0 + m[0]) + m[1] + m[2]
    x = np.maximum(np.abs(lo), np.abs(hi))
    x1 = (0.0 + x[0]) + x[1] + x[2]
    margin = py["theta"] * np.sqrt(r2) + BETA * (x1 + py["c1"])
    for n in py["n"]:
        f = np.maximum(n * d0, n * d1)
        if (f[0] + f[1]) + f[2] < -margin:
            return False
    return True


def record(nodes, root, view, pixels, K=8):
    """(the K words, the set of entries the pass expanded or dropped)"""
    py = pyramid(view, pixels)
    lst, expanded = [], set()
    if root != ENTRY_DONE and py is not None:
        lst = [root]
    while py is not None and py["ok"] and lst:
        top = lst[-1]
        if top & ENTRY_LEAF:
            break
        nd = nodes[top & ENTRY_INDEX_MASK]
        t = [int(nd["entry"][k]) for k in range(4) if nd["entry"][k] != ENTRY_EMPTY and touched(py, nd["lo"][:, k], nd["hi"][:, k])]
        if t and len(lst) - 1 + len(t) > K:
            break
        lst.pop()
        expanded.add(top)
        lst += t[::-1]
    return lst + [ENTRY_DONE] * (K - len(lst)), expanded


# ---- the rays of a group, and the walk from the root ---------------------------------------------------------------------------
def rays(view, pixels, per_pixel, rng):
    """Directions (n x 3, float64, not normalised: a slab test does not care) of pt_primary_ray's rays of these pixels: jitter at the
    four corners 0 / nextafter(1, 0) and `per_pixel` random ones, through the float32 shapes of the ray (u and v rounded to float32,
    the point and the difference rounded per component)."""
    f32 = np.float32
    top = np.nextafter(f32(1.0), f32(0.0))
    out = []
    for x, y in pixels:
        r = rng.random((per_pixel, 2)).astype(f32)
        r = np.concatenate([r, f32([[0, 0], [0, top], [top, 0], [top, top]])])
        u = ((f32(x) + r[:, 0]) * f32(view.inv_w)).astype(np.float64)
        v = ((f32(y) + r[:, 1]) * f32(view.inv_h)).astype(np.float64)
        p = (view.p1[None] + view.right[None] * u[:, None]).astype(f32).astype(np.float64)
        p = (p + view.up[None] * v[:, None]).astype(f32).astype(np.float64)
        out.append((p - view.pos[None]).astype(f32).astype(np.float64))
    return np.concatenate(out)


def _enters(o, d, lo, hi):
    """which rays (rows of d, from o) meet the box at t >= 0 — exact in float64 up to its own rounding, closed"""
    with np.errstate(all="ignore"):
        t0, t1 = (lo[None] - o[None]) / d, (hi[None] - o[None]) / d
    tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
    par = d == 0.0
    inside = (o[None] >= lo[None]) & (o[None] <= hi[None])
    tn = np.where(par, np.where(inside, -np.inf, np.inf), tn)
    tf = np.where(par, np.where(inside, np.inf, -np.inf), tf)
    return np.maximum(tn.max(1), 0.0) <= tf.min(1)


def coverage(nodes, root, view, words, expanded, d):
    """(nodes entered from the root that the record does not cover, nodes entered)"""
    rec = {int(w) for w in words if w != ENTRY_DONE}
    o = view.pos
    bad = seen = 0
    stack = [(root, np.ones(len(d), bool))] if root != ENTRY_DONE else []
    while stack:
        e, m = stack.pop()
        seen += 1
        if e in rec:
            continue
        if (e & ENTRY_LEAF) or e not in expanded:
            bad += 1
            continue
        nd = nodes[e & ENTRY_INDEX_MASK]
        for k in range(4):
            if nd["entry"][k] == ENTRY_EMPTY or (nd["lo"][:, k] > nd["hi"][:, k]).any():
                continue
            mk = m.copy()
            mk[m] = _enters(o, d[m], nd["lo"][:, k].astype(np.float64), nd["hi"][:, k].astype(np.float64))
            if mk.any():
                stack.append((int(nd["entry"][k]), mk))
    return bad, seen
