"""Exact checker of the TRAVERSED tree of one mesh: the compressed 4-wide nodes (rt::Node4c), their float expansion
(rt::Node4f), the leaf-ordered triangles and the recorded stack need, as rfwhip_get_bvh4 reads them back from the device.

Plain numpy with no product code: the entry layout, the plane decode fma(q, scale, org) and the definition of the stack
need (bvh::stack_need4) are restated here from rt_types.h.  Every comparison is exact — no epsilon anywhere: a child box that
was quantised inward by one step fails, even though it would lose only grazing rays."""
import numpy as np

ENTRY_LEAF = 0x80000000
ENTRY_TLAS = 0x40000000
ENTRY_EMPTY = 0xFFFFFFFC
ENTRY_FIRST_MASK = 0x07FFFFFF
ENTRY_INDEX_MASK = 0x3FFFFFFF
TRI_EPS = np.float32(1e-6)
NO_SRC = 0xFFFFFFFF


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _qbytes(words):
    """(n, 3) uint32 words -> (n, 3, 4) plane bytes, byte k = child k."""
    return (words[..., None] >> (8 * np.arange(4, dtype=np.uint32))) & 0xFF


def decode_planes(nodes4c):
    """The planes the traversal decodes, fma(q, scale, org), as (lo, hi) float32 arrays of shape (n, 3, 4).  Computed in
    float64 and rounded once to float32: q * 2^e and org are exact there, so the float64 sum is the exact sum — asserted
    (TwoSum error term zero) rather than assumed — and one rounding of the exact sum is what fmaf returns."""
    org = nodes4c["org"].astype(np.float64)[:, :, None]
    scale = np.stack([nodes4c["scale_x"], nodes4c["scale_y"], nodes4c["scale_z"]], -1)
    m, _ = np.frexp(scale)
    assert np.all(scale > 0) and np.all(m == 0.5), "scale is not a power of two"
    scale = scale.astype(np.float64)[:, :, None]
    out = []
    for words in (nodes4c["qlo"], nodes4c["qhi"]):
        p = _qbytes(words).astype(np.float64) * scale
        s = p + org
        bv = s - p
        err = (p - (s - bv)) + (org - bv)
        assert np.all(err == 0), "a decoded plane is not exact in float64: the float64 decode would not equal fmaf"
        out.append(s.astype(np.float32))
    return out[0], out[1]


def _levels(child, n4):
    """Breadth-first levels of node indices (0-based) from the root; asserts every node is reached exactly once."""
    seen = np.zeros(n4, np.int32)
    levels = [np.array([0])]
    seen[0] = 1
    while True:
        c = child[levels[-1]].ravel()
        c = c[c >= 0]
        if not len(c):
            break
        np.add.at(seen, c, 1)
        assert seen.max() == 1, "a 4-wide node is reached twice (or the tree has a cycle)"
        levels.append(c)
    assert seen.min() == 1, "%d 4-wide nodes are not reached from the root" % int((seen == 0).sum())
    return levels


def check_bvh4(b, vertices, indices, max_leaf, nodes2=None, stamps=()):
    """b: CoreBinding.get_bvh4(mesh); vertices / indices: the mesh as set_mesh received it (vertices n x 3 or n x 4, or
    None for a mesh posed on the device; indices None or n x 3); max_leaf: the builder's largest leaf; nodes2:
    CoreBinding.get_bvh(mesh)[0] (the BVH2 boxes src4 names), or None to skip that part; stamps: the mesh's instances — v1.w is 1.0 as built, or the index of the instance that is
    linked into the top-level tree directly ("flat", rfwhip_update stamps it into every v1.w).  Returns a few figures."""
    n4, nt = int(b["n4_count"]), int(b["tri_count"])
    base, tb = int(b["n4_base"]), int(b["tri_base"])
    c4, f4, src4, tv = b["nodes4c"], b["nodes4f"], b["src4"], b["tri_verts"]
    assert len(c4) == n4 and len(f4) == n4 and src4.shape == (n4, 4) and tv.shape == (nt, 3, 4)

    # ---- triangles: a permutation of the mesh's, bit for bit ----
    prim = _bits(tv[:, 0, 3])
    assert np.array_equal(np.sort(prim), np.arange(nt, dtype=np.uint32)), "leaf slots are not a permutation of the primitives"
    if vertices is not None:   # (None: vertices posed on the device — the boxes are checked against the slots' own vertices)
        v = np.asarray(vertices, np.float32)[:, :3]
        corners = (np.asarray(indices, np.int64).reshape(-1, 3)[prim] if indices is not None
                   else 3 * prim.astype(np.int64)[:, None] + np.arange(3))
        assert np.array_equal(_bits(tv[:, :, :3]), _bits(v[corners])), "a leaf slot's vertices differ from its primitive's"
    w1 = np.unique(_bits(tv[:, 1, 3]))
    assert len(w1) <= 1 and (not len(w1) or w1[0] == _bits(np.float32(1.0)) or int(w1[0]) in set(stamps)), "unexpected v1.w"
    assert np.all(_bits(tv[:, 2, 3]) == _bits(TRI_EPS)), "unexpected v2.w"
    lo_t, hi_t = tv[:, :, :3].min(1), tv[:, :, :3].max(1)   # per slot, float32

    if n4 == 0:   # the root is a leaf: no 4-wide node
        assert 1 <= nt <= max_leaf and int(b["stack_need"]) == 0
        return {"n4": 0, "leaves": 1, "depth": 0, "stack_need": 0}

    # ---- entries ----
    e = c4["entry"].astype(np.int64)
    empty = e == ENTRY_EMPTY
    leaf = ~empty & ((e & ENTRY_LEAF) != 0)
    inner = ~empty & ~leaf
    assert not np.any((e & ENTRY_TLAS)[~empty]), "a mesh entry carries the top-level bit"
    assert np.all((inner | leaf).sum(1) >= 2), "a 4-wide node with fewer than two children"
    ci = e & ENTRY_INDEX_MASK
    assert np.array_equal(ci[inner], e[inner]), "an inner entry carries flag bits"
    assert np.all((ci[inner] >= base) & (ci[inner] < base + n4)), "an inner entry outside [n4_base, n4_base + n4_count)"
    child = np.where(inner, ci - base, -1)
    levels = _levels(child, n4)
    first = e & ENTRY_FIRST_MASK
    cnt = ((e >> 27) & 7) + 1
    assert np.all((cnt[leaf] >= 1) & (cnt[leaf] <= max_leaf)), "a leaf larger than the builder's maximum"
    assert np.all((first[leaf] >= tb) & (first[leaf] + cnt[leaf] <= tb + nt)), "a leaf outside [tri_base, tri_base + tri_count)"
    lf, lc = first[leaf], cnt[leaf]
    order = np.argsort(lf, kind="stable")
    lf, lc = lf[order], lc[order]
    assert lf[0] == tb and np.array_equal(lf[1:], lf[:-1] + lc[:-1]) and lf[-1] + lc[-1] == tb + nt, \
        "leaf ranges overlap or leave slots uncovered"

    # ---- empty slots: inverted box, no source ----
    ql, qh = _qbytes(c4["qlo"]), _qbytes(c4["qhi"])                # (n4, 3, 4)
    em3 = np.broadcast_to(empty[:, None, :], ql.shape)
    assert np.all(ql[em3] == 255) and np.all(qh[em3] == 0), "an unused slot without the inverted box"
    assert np.all(src4[empty] == NO_SRC)
    assert np.all(ql[~em3] <= qh[~em3]), "a used slot with an inverted (never hit) box"

    # ---- decoded boxes contain everything below them, exactly ----
    lo, hi = decode_planes(c4)                                       # (n4, 3, 4)
    ext_lo = np.full((n4, 4, 3), np.inf, np.float32)
    ext_hi = np.full((n4, 4, 3), -np.inf, np.float32)
    li, lk = np.nonzero(leaf)
    s0 = (first[li, lk] - tb).astype(np.int64)
    srt = np.argsort(s0)                                             # leaf ranges cover the slots in this order
    ext_lo[li[srt], lk[srt]] = np.minimum.reduceat(lo_t, s0[srt], axis=0)
    ext_hi[li[srt], lk[srt]] = np.maximum.reduceat(hi_t, s0[srt], axis=0)
    for lev in reversed(levels):                                     # bottom-up: a node's extremes are its children's
        sub = child[lev]
        pi, pk = np.nonzero(sub >= 0)
        ch = sub[pi, pk]
        ext_lo[lev[pi], pk] = ext_lo[ch].min(1)
        ext_hi[lev[pi], pk] = ext_hi[ch].max(1)
    used = ~empty
    dlo, dhi = lo.transpose(0, 2, 1)[used], hi.transpose(0, 2, 1)[used]   # (slots, 3)
    bad = (dlo > ext_lo[used]) | (dhi < ext_hi[used])
    assert not bad.any(), "%d decoded child planes cut a triangle below them (first: node %d)" % (
        int(bad.sum()), int(np.nonzero(used)[0][np.nonzero(bad.any(1))[0][0]]))
    if nodes2 is not None:
        s = src4[used].astype(np.int64)
        assert np.all(s < len(nodes2)), "src4 names no BVH2 node of the mesh"
        assert np.all(dlo <= nodes2["bmin"][s]) and np.all(dhi >= nodes2["bmax"][s]), \
            "a decoded child box does not contain the BVH2 box it was quantised from"

    # ---- the float form is the decode, bit for bit ----
    assert np.array_equal(f4["entry"], c4["entry"]) and not f4["pad"].any()
    want_lo = np.where(empty[:, None, :], np.float32(1e30), lo)
    want_hi = np.where(empty[:, None, :], np.float32(-1e30), hi)
    assert np.array_equal(_bits(f4["lo"]), _bits(want_lo)) and np.array_equal(_bits(f4["hi"]), _bits(want_hi)), \
        "Node4f differs from the decode of its Node4c"

    # ---- stack need (bvh::stack_need4): entries pending above a node + its children - 1, worst over the tree ----
    kids = used.sum(1)
    here = np.zeros(n4, np.int64)
    above = np.zeros(n4, np.int64)
    for lev in levels:
        here[lev] = above[lev] + np.maximum(kids[lev] - 1, 0)
        sub = child[lev]
        pi, pk = np.nonzero(sub >= 0)
        above[sub[pi, pk]] = here[lev[pi]]
    assert int(b["stack_need"]) == int(here.max()), "recorded stack need %d, the tree needs %d" % (b["stack_need"], here.max())
    return {"n4": n4, "leaves": int(leaf.sum()), "depth": len(levels), "stack_need": int(here.max())}
