"""Regenerate tests/golden/asset_animation.npz (development container only: reads the reference checkout's assets).

Per file — CesiumMan.gltf ("cesiumman"), AnimatedMorphCube.glb ("morphcube") and InterpolationTest.glb ("interpolation": STEP, LINEAR
and CUBICSPLINE samplers on translations, rotations and scales) — the packed rig tables of Gltf.rig() (records as their 32-bit
words) and, at five times, what gltf.py computes in float64: local TRS (N, 10), world matrices (N, 4, 4), the joint matrices of
every rig skin one after the other (J, 4, 4) and the weight table.  The times: 0, a time exactly on an inner key, a time between
keys, the last key, 2.5 durations.

gltf.py starts from the file's doubles; the rig holds float32.  So that the recorded values are those of the PACKED rig, gltf.py's
state (T, R, S, M, W) is set to the rig's float32 values before every evaluation (key times and values, and the inverse bind
matrices, are float32 in the files already).  Everything after that is gltf.py's own code: set_time, local, combined.

    python tests/golden/make_golden_animation.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

ASSETS = "/root/reference/assets/models"
FILES = (("cesiumman", os.path.join("CesiumMan", "CesiumMan.gltf")), ("morphcube", "AnimatedMorphCube.glb"),
         ("interpolation", "InterpolationTest.glb"))


def reset(g, rig):
    """gltf.py's animated state = the packed rig's base values."""
    nd = rig["nodes"]
    for i in range(len(nd)):
        g.T[i], g.R[i], g.S[i] = (nd[i][k].astype(np.float64) for k in ("translation", "rotation", "scale"))
        g.M[i] = nd[i]["matrix"].astype(np.float64).reshape(4, 4).T
        if g.W[i] is not None:
            o = int(nd[i]["weight_offset"])
            g.W[i] = rig["weights"][o:o + int(nd[i]["weight_count"])].astype(np.float64)


def record(g, rig, time):
    reset(g, rig)
    g.set_time(float(time))
    n = len(g.nodes)
    trs = np.stack([np.concatenate([g.T[i], g.R[i], g.S[i]]) for i in range(n)])
    world = np.stack([g.combined(i) for i in range(n)])
    weights = np.concatenate([g.W[i] for i in range(n) if g.W[i] is not None] + [np.zeros(0)])
    joints = []
    for sk in rig["skins"]:
        inv = np.linalg.inv(g.combined(int(sk["mesh_node"])))
        for j in range(int(sk["joint_offset"]), int(sk["joint_offset"] + sk["joint_count"])):
            ibm = rig["inverse_bind"][16 * j:16 * j + 16].astype(np.float64).reshape(4, 4).T
            joints.append(inv @ g.combined(int(rig["joints"][j])) @ ibm)
    return trs, world, weights, np.stack(joints) if joints else np.zeros((0, 4, 4))


def main():
    pkg = load_package()
    out = {}
    for name, rel in FILES:
        try:
            g = pkg.gltf.Gltf(os.path.join(ASSETS, rel))
            rig = g.rig()
        except Exception as e:  # (a file gltf.py cannot read is left out, and said so)
            print("%s: left out (%s: %s)" % (name, type(e).__name__, e))
            continue
        ch0 = rig["channels"][0]
        t0 = rig["times"][ch0["time_offset"]:ch0["time_offset"] + ch0["key_count"]]
        duration = float(max(rig["times"][c["time_offset"] + c["key_count"] - 1] for c in rig["channels"]))
        inner = t0[len(t0) // 2] if len(t0) > 2 else t0[0]
        between = np.float32(0.5 * (float(t0[1]) + float(t0[min(2, len(t0) - 1)]))) if len(t0) > 2 else np.float32(0.5 * (float(t0[0]) + float(t0[-1])))
        times = np.array([0.0, inner, between, duration, 2.5 * duration], np.float32)
        rec = [record(g, rig, t) for t in times]
        for k, _ in pkg.abi.RIG_TABLES:
            a = np.ascontiguousarray(rig[k])
            out["%s/rig/%s" % (name, k)] = a if a.dtype in (np.float32, np.uint32) else a.view(np.uint32)
        out[name + "/times"] = times
        for k, key in enumerate(("trs", "world", "weights", "joints")):
            out["%s/%s" % (name, key)] = np.stack([r[k] for r in rec])
        print("%s: %d nodes, %d skins, %d joints, %d channels, %d key values; times %s" % (
            name, len(rig["nodes"]), len(rig["skins"]), len(rig["joints"]), len(rig["channels"]), len(rig["values"]), list(times)))
    path = os.path.join(HERE, "asset_animation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
