"""float64 model of the primary wave's ordering item (csrc/primary_order.h): for one rt::Node4f and an origin C, the four
children permuted by
    (empty last, squared distance from C to the child's box — 0 inside —, squared distance from C to the box centre, slot).
A node is a record of 32 words: lo[3][4], hi[3][4] (float32), entry[4], pad[4] (uint32) — NODE4F below.  An unused slot has
entry ENTRY_EMPTY or a box inverted on some axis; it goes last, in slot order, as it is."""
import numpy as np

ENTRY_EMPTY = 0xFFFFFFFC
NODE4F = np.dtype([("lo", np.float32, (3, 4)), ("hi", np.float32, (3, 4)), ("entry", np.uint32, (4,)), ("pad", np.uint32, (4,))])
assert NODE4F.itemsize == 128


def keys(node, origin):
    """Per slot: (empty, d2 to the box, d2 to the centre) in float64."""
    lo, hi = node["lo"].astype(np.float64), node["hi"].astype(np.float64)
    c = np.asarray(origin, np.float64)[:, None]
    empty = (node["entry"] == ENTRY_EMPTY) | (lo > hi).any(0)
    d = np.maximum(np.maximum(lo - c, c - hi), 0.0)
    dc = (lo + hi) * 0.5 - c
    return empty, (d * d).sum(0), (dc * dc).sum(0)


def permutation(node, origin):
    empty, d2, dc2 = keys(node, origin)
    return sorted(range(4), key=lambda k: (True, 0.0, 0.0, k) if empty[k] else (False, d2[k], dc2[k], k))


def order(nodes, origin):
    """The ordered table of `nodes` (a NODE4F array)."""
    out = nodes.copy()
    for i, n in enumerate(nodes):
        p = permutation(n, origin)
        out[i]["lo"], out[i]["hi"] = n["lo"][:, p], n["hi"][:, p]
        out[i]["entry"], out[i]["pad"] = n["entry"][p], n["pad"][p]
    return out


def random_nodes(rng, n, grid=None, empty_rate=0.2, span=8.0):
    """n nodes of random boxes in [-span, span]^3.  grid: every plane is a multiple of 1 / grid (with origins on the same grid every
    key is exact in float32 AND float64, so the two orders must agree to the last tie); None: any float32."""
    nodes = np.zeros(n, NODE4F)
    a, b = rng.uniform(-span, span, (n, 3, 4)), rng.uniform(-span, span, (n, 3, 4))
    if grid:
        a, b = np.round(a * grid) / grid, np.round(b * grid) / grid
    nodes["lo"], nodes["hi"] = np.minimum(a, b), np.maximum(a, b)
    nodes["entry"] = rng.integers(0, 1 << 27, (n, 4), dtype=np.uint32)  # (distinct enough to tell the children apart)
    nodes["pad"] = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint32)
    # unused slots of both kinds: by entry (the box any), and inverted as the float table has them (lo = 1e30, hi = -1e30)
    kill = rng.random((n, 4)) < empty_rate
    by_entry = kill & (rng.random((n, 4)) < 0.5)
    nodes["entry"][by_entry] = ENTRY_EMPTY
    inv = kill & ~by_entry
    for ax in range(3):
        nodes["lo"][:, ax, :][inv] = np.float32(1e30)
        nodes["hi"][:, ax, :][inv] = np.float32(-1e30)
    nodes["entry"][inv & (rng.random((n, 4)) < 0.5)] = ENTRY_EMPTY  # (the rest: inverted under a live entry — still unused)
    return nodes
