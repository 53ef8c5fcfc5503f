"""numpy restatement of the motion part of the denoiser's temporal stage (setting "denoise_motion", include/rfwhip.h;
rendering-fw_amd/csrc/denoise.h dn_motion_point / denoise_temporal_body.h).  Two halves:

  previous_points   float64 (the yardstick) or float32 (the stage model's input): the previous position X_P of each pixel's surface
                    point and its normal n'_p carried back to the previous presented frame, from the hit's primitive and
                    barycentrics (rfwhip_trace_rays along the guide's centre ray), the HOST's vertices then and now and the
                    instance's transforms then and now;
  temporal          float32: tests/denoise_temporal_model.py's frame with X and n_p replaced by those at the pixels of MOVED
                    instances (state 2), pixels of RESTART instances (state 3) fresh, everything else as there.
"""
import numpy as np

import denoise_temporal_model as T
from denoise_model import ALBEDO_MIN, F, depth_gradient, lum

INVALID, STILL, MOVED, RESTART = 0, 1, 2, 3


def centre_hits(ctx, camera, valid, z):
    """Per pixel the hit the guide pass kept along the centre ray: instance, primitive, u, v (rfwhip_trace_rays; -1 / 0 where the
    guide is invalid).  Alpha-tested layers are passed as the guide pass does, until the distance is the guide's z."""
    h, w = valid.shape
    cam = T.camera_of(ctx, camera)
    d = T.centre_dirs(cam, w, h).reshape(-1, 3)
    o = np.broadcast_to(cam[0], d.shape).astype(np.float32).copy()
    ids, prim = np.full(h * w, -1, np.int64), np.full(h * w, -1, np.int64)
    u, v = np.zeros(h * w, np.float32), np.zeros(h * w, np.float32)
    todo = valid.reshape(-1).copy()
    dist = np.zeros(h * w, np.float32)
    zz = z.reshape(-1)
    for _ in range(9):
        if not todo.any():
            break
        k = np.flatnonzero(todo)
        hit = ctx.trace_rays(np.ascontiguousarray(o[k]), np.ascontiguousarray(d[k]))
        dist[k] += hit["t"]
        done = np.abs(dist[k] - zz[k]) <= 1e-4 * zz[k] + 1e-5
        kd = k[done]
        ids[kd], prim[kd], u[kd], v[kd] = hit["inst"][done], hit["prim"][done], hit["u"][done], hit["v"][done]
        todo[kd] = False
        nk = k[~done]
        o[nk] = o[nk] + d[nk] * hit["t"][~done, None] + d[nk] * F(1e-5)
        dist[nk] += F(1e-5)
    return {"ids": ids.reshape(h, w), "prim": prim.reshape(h, w), "u": u.reshape(h, w), "v": v.reshape(h, w)}


def _xform(m, v):
    """rows 0..2 of m on points v (n x 3), summed left to right as dn_xform does."""
    return np.stack([m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1] + m[r, 2] * v[:, 2] + m[r, 3] for r in range(3)], -1)


def previous_points(hits, normal, moved, dtype=np.float64):
    """moved: {instance: dict(cur=V x 3 current object-space vertices, prev=V x 3 the ones at the previous presented frame,
    indices=T x 3 or None, m_f=4 x 4 transform now, m_p=4 x 4 transform then)}.  Returns (X_P, n'_p, ok), H x W x 3 / H x W; ok is
    False outside the moved instances and on degenerate triangles.  dtype float64: the yardstick of the positions and normals;
    float32: dn_motion_point's arithmetic in its order, the input of the float32 stage model below (the bilinear weights of the
    reprojection magnify a position error by the image's pixels per unit length: the tolerances of the stage's values are those of
    the same float32 arithmetic, as in tests/denoise_temporal_model.py)."""
    ids, prim = hits["ids"], hits["prim"]
    u, v = hits["u"].astype(dtype), hits["v"].astype(dtype)
    xp = np.zeros(ids.shape + (3,), dtype)
    nn = np.zeros(ids.shape + (3,), dtype)
    ok = np.zeros(ids.shape, bool)
    one = dtype(1)
    for inst, r in moved.items():
        sel = (ids == inst) & (prim >= 0)
        if not sel.any():
            continue
        k = prim[sel]
        if r.get("indices") is None:  # (unindexed: triangle k has the vertices 3 k .. 3 k + 2)
            idx = np.arange(len(r["cur"]) // 3 * 3).reshape(-1, 3)[k]
        else:
            idx = np.asarray(r["indices"], np.int64).reshape(-1, 3)[k]
        m_f, m_p = np.asarray(r["m_f"], dtype), np.asarray(r["m_p"], dtype)
        a = np.asarray(r["cur"], dtype)[:, :3][idx]   # n x 3 (corner) x 3
        b = np.asarray(r["prev"], dtype)[:, :3][idx]
        us, vs = u[sel][:, None], v[sel][:, None]
        w = one - us - vs
        A0, B0 = _xform(m_f, a[:, 0]), _xform(m_p, b[:, 0])
        e1, e2 = _xform(m_f, a[:, 1]) - A0, _xform(m_f, a[:, 2]) - A0
        f1, f2 = _xform(m_p, b[:, 1]) - B0, _xform(m_p, b[:, 2]) - B0
        x = _xform(m_p, b[:, 0] * w + b[:, 1] * us + b[:, 2] * vs)
        ca, cb = np.cross(e1, e2), np.cross(f1, f2)
        la, d = np.sqrt((ca * ca).sum(-1)), np.sqrt((cb * cb).sum(-1))
        good = (la > 0) & (d > 0) & np.isfinite(la) & np.isfinite(d)
        with np.errstate(divide="ignore", invalid="ignore"):
            na, nb = ca * (one / la)[:, None], cb * (one / d)[:, None]
            n = normal[sel].astype(dtype)
            c1, c2, c3 = (e1 * n).sum(-1), (e2 * n).sum(-1), (na * n).sum(-1)
            r3 = (np.cross(f2, nb) * c1[:, None] + np.cross(nb, f1) * c2[:, None]) * (one / d)[:, None] + nb * c3[:, None]
            lr = np.sqrt((r3 * r3).sum(-1))
            good &= (lr > 0) & np.isfinite(lr)
            r3 = r3 * (one / lr)[:, None]
        xp[sel] = np.where(good[:, None], x, 0).astype(dtype)
        nn[sel] = np.where(good[:, None], r3, 0).astype(dtype)
        ok[sel] = good
    return xp, nn, ok


def reproject(cam, prev, guides, ids, state, xp, npv):
    """tests/denoise_temporal_model.py reproject with per-pixel states: STILL pixels as there, MOVED pixels through xp / npv
    (float32, H x W x 3; a pixel with a zero npv — a degenerate triangle — is fresh), everything else fresh.  Returns (tap indices,
    renormalised weights, the consistent taps' bilinear weights, and which taps pass every test but the weight's)."""
    valid, normal, z = guides["valid"], guides["normal"], guides["z"]
    h, w = z.shape
    wq = np.zeros((h, w, 4), np.float32)
    qi = np.zeros((h, w, 4), np.int64)
    cons = np.zeros((h, w, 4), bool)
    if prev is None:
        return qi, wq, wq, cons
    pos_p, p1, right, up = prev["cam"]
    d = T.centre_dirs(cam, w, h)
    moved = state == MOVED
    x = np.where(moved[..., None], xp.astype(np.float32), cam[0] + d * z[..., None]).astype(np.float32)
    normal = np.where(moved[..., None], npv.astype(np.float32), normal).astype(np.float32)
    usable = (state == STILL) | (moved & (np.abs(npv).sum(-1) > 0))
    e = (x - pos_p).astype(np.float32)
    pn = np.cross(right, up).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.dot(p1 - pos_p, pn) / (e @ pn)
        q = pos_p + e * s[..., None] - p1
        rr, ru, uu = np.dot(right, right), np.dot(right, up), np.dot(up, up)
        qr, qu = q @ right, q @ up
        det = rr * uu - ru * ru
        xf = (qr * uu - qu * ru) / det * F(w) - F(0.5)
        yf = (qu * rr - qr * ru) / det * F(h) - F(0.5)
        ok = valid & (s > 0) & (xf > -1) & (xf < w) & (yf > -1) & (yf < h)
        xf, yf = np.where(ok, xf, F(0)), np.where(ok, yf, F(0))
    fx0, fy0 = np.floor(xf), np.floor(yf)
    fx, fy = (xf - fx0).astype(np.float32), (yf - fy0).astype(np.float32)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    dist = np.linalg.norm(e, axis=-1).astype(np.float32)
    pv, pz, pgx, pgy, pnrm, pid = prev["valid"], prev["z"], prev["gx"], prev["gy"], prev["normal"], prev["ids"]
    same = ok & (ids >= 0) & usable
    for k in range(4):
        qx, qy = x0 + (k & 1), y0 + (k >> 1)
        bw = ((fx if k & 1 else F(1) - fx) * (fy if k >> 1 else F(1) - fy)).astype(np.float32)
        inside = (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
        cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
        good = same & inside & pv[cy, cx] & (pid[cy, cx] == ids)
        good &= np.abs(pz[cy, cx] - dist) <= T.DEPTH_GRAD * (np.abs(pgx[cy, cx]) + np.abs(pgy[cy, cx])) + T.DEPTH_REL * dist
        good &= np.sum(normal * pnrm[cy, cx], -1) >= T.NORMAL
        cons[..., k] = good
        wq[..., k] = np.where(good & (bw > 0), bw, F(0))
        qi[..., k] = cy * w + cx
    ws = wq.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        wn = np.where((ws >= T.MIN_WEIGHT)[..., None], wq / ws[..., None], F(0)).astype(np.float32)
    return qi, wn, wq, cons


def temporal(rgba, guides, ids, cam, prev, state, xp, npv, alpha=0.2, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0):
    """One presented frame, as denoise_temporal_model.temporal, with the motion states.  The state returned also holds "taps": how
    many of the 4 bilinear taps were consistent (4: the reprojection lost nothing)."""
    rgba = np.asarray(rgba, np.float32)
    albedo, valid, normal, z = guides["albedo"], guides["valid"], guides["normal"], guides["z"]
    gx, gy = depth_gradient(z, valid)
    irr = rgba[..., :3] / np.maximum(albedo, ALBEDO_MIN)
    l = lum(irr[..., 0], irr[..., 1], irr[..., 2])
    qi, wq, raw_w, cons = reproject(cam, prev, guides, ids, state, xp, npv)
    fresh = ~(wq.sum(-1) > 0)
    mscale = np.stack([np.abs(l), l * l], -1).astype(np.float32)
    if prev is not None:
        pm = np.abs(prev["moments"].reshape(-1, 2)[qi])
        # (with a still camera a still pixel lands on a pixel centre of P to within rounding: a neighbouring tap then has the weight
        # 0 or 1e-7 by the last bit of x', here or in the stage.  The scale covers every tap the stage may have read — those that
        # pass all tests but the weight's — so that a firefly's moments times 1e-7 are measured against the firefly)
        mscale = np.maximum(mscale, np.where(cons[..., None], pm, F(0)).max(-2))
    n = np.ones(z.shape, np.float32)
    pre = np.concatenate([irr, l[..., None]], -1).astype(np.float32)
    m1, m2 = l.copy(), (l * l).astype(np.float32)
    if prev is not None and (~fresh & valid).any():
        hc = prev["history"].reshape(-1, 4)[qi][..., :3]
        hm = prev["moments"].reshape(-1, 2)[qi]
        hn = prev["length"].reshape(-1)[qi]
        wk = np.where(fresh[..., None], F(0), wq)
        h_rgb = (wk[..., None] * np.nan_to_num(hc)).sum(-2)
        h1, h2 = (wk * np.nan_to_num(hm[..., 0])).sum(-1), (wk * np.nan_to_num(hm[..., 1])).sum(-1)
        n_b = np.minimum((wk * hn).sum(-1) + F(1), T.MAX_N)
        a = np.maximum(F(alpha), F(1) / n_b)
        rgb = (F(1) - a)[..., None] * h_rgb + a[..., None] * irr
        blend = np.concatenate([rgb, lum(rgb[..., 0], rgb[..., 1], rgb[..., 2])[..., None]], -1)
        pre = np.where(fresh[..., None], pre, blend).astype(np.float32)
        m1 = np.where(fresh, m1, (F(1) - a) * h1 + a * l).astype(np.float32)
        m2 = np.where(fresh, m2, (F(1) - a) * h2 + a * (l * l)).astype(np.float32)
        n = np.where(fresh, n, n_b).astype(np.float32)
    v3 = T.variance3x3(l, valid, normal, z, gx, gy, sigma_n, sigma_z)
    var = np.where(n >= T.VAR_N, np.maximum(F(0), m2 - m1 * m1), v3).astype(np.float32)
    pre = np.where(valid[..., None], pre, F(0)).astype(np.float32)
    var = np.where(valid, var, F(0)).astype(np.float32)
    out, hist = T.atrous(rgba, albedo, valid, normal, z, gx, gy, pre, var, iterations, sigma_l, sigma_n, sigma_z)
    st = {"cam": cam, "valid": valid, "z": z, "gx": gx, "gy": gy, "normal": normal, "ids": np.where(valid, ids, -1),
          "pre": pre, "var": var, "history": np.where(valid[..., None], hist, F(0)).astype(np.float32),
          "moments": np.where(valid[..., None], np.stack([m1, m2], -1), F(0)).astype(np.float32),
          "length": np.where(valid, n, F(0)).astype(np.float32), "mscale": mscale,
          "taps": np.where(valid, (raw_w > 0).sum(-1), 0)}
    return out, st


def pixel_states(valid, ids, inst_state):
    """Per pixel: 0 invalid, else the state of its instance (inst_state: per instance 1 / 2 / 3)."""
    inst_state = np.asarray(inst_state, np.int64)
    return np.where(valid & (ids >= 0), inst_state[np.clip(ids, 0, len(inst_state) - 1)], INVALID)
