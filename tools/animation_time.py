"""Time a frame's animation step on one device along two paths (include/rfwhip.h, rfwhip_animate; csrc/animation.h), for CesiumMan's
rig from the committed fixtures (tests/golden/asset_animation.npz: the packed rig; asset_cesiumman.npz: the mesh and its skin) and for
64 copies of it, each with its own mesh, at 64 different times:
  host    the path of the commits before rfwhip_animate: gltf.py's set_time and joint matrices on the host (its own code, run over
          the fixture's tables: Gltf.set_time, Gltf.combined, inverse(mesh node) x joint x inverse bind in float64), then
          rfwhip_pose_mesh per character
  device  rfwhip_animate: one call per frame, whatever the number of characters
A frame is timed between two ctx.wait() fences and holds the animation step alone: no rfwhip_update, no render.  Each path warms up
first; the figure is the median of `frames` frames.  host_only_ms is the host path's Python part by itself, rig_kernel_ms the
rig kernel's own time (hipEvents: stage_timing = 1, kernel family 18) per call.  No time here is a pass criterion, and no ratio is
asserted anywhere: the file records what was measured and on what.
Usage: python tools/animation_time.py [out=profiles/animation_time.json] [frames=40]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_rig(pkg, rig):
    """gltf.py's Gltf over the packed tables instead of a file: its animated state and its animations, for set_time and combined."""
    import numpy as np
    g = pkg.gltf.Gltf.__new__(pkg.gltf.Gltf)
    nd = rig["nodes"]
    n = len(nd)
    g.nodes = [{} for _ in range(n)]
    g.parents = [int(p) for p in nd["parent"]]
    g.T = [nd[i]["translation"].astype(np.float64) for i in range(n)]
    g.R = [nd[i]["rotation"].astype(np.float64) for i in range(n)]
    g.S = [nd[i]["scale"].astype(np.float64) for i in range(n)]
    g.M = [nd[i]["matrix"].astype(np.float64).reshape(4, 4).T for i in range(n)]
    g.W = [rig["weights"][int(nd[i]["weight_offset"]):int(nd[i]["weight_offset"] + nd[i]["weight_count"])].astype(np.float64) for i in range(n)]
    paths = {v: k for k, v in pkg.abi.RIG_PATHS.items()}
    methods = {v: k for k, v in pkg.abi.RIG_METHODS.items()}
    g.animations = []
    for a in rig["animations"]:
        samplers, chans = [], []
        for c in rig["channels"][int(a["channel_offset"]):int(a["channel_offset"] + a["channel_count"])]:
            times = rig["times"][int(c["time_offset"]):int(c["time_offset"] + c["key_count"])].astype(np.float64)
            vals = rig["values"][int(c["value_offset"]):int(c["value_offset"] + c["value_count"])].astype(np.float64)
            width = 4 if paths[int(c["path"])] == "rotation" else 1 if paths[int(c["path"])] == "weights" else 3
            samplers.append({"method": methods[int(c["method"])], "times": times, "keys": vals.reshape(-1, width)})
            chans.append({"sampler": len(samplers) - 1, "node": int(c["node"]), "path": paths[int(c["path"])]})
        g.animations.append({"samplers": samplers, "channels": chans})
    sk = rig["skins"][0]
    sl = slice(int(sk["joint_offset"]), int(sk["joint_offset"] + sk["joint_count"]))
    ibm = rig["inverse_bind"].reshape(-1, 4, 4)[sl].astype(np.float64).transpose(0, 2, 1)
    joints, mesh_node = [int(j) for j in rig["joints"][sl]], int(sk["mesh_node"])

    def joint_matrices():  # (Gltf.joint_matrices, with the skin's tables at hand instead of the file's accessors)
        inv = np.linalg.inv(g.combined(mesh_node))
        return np.stack([inv @ g.combined(j) @ ibm[k] for k, j in enumerate(joints)]).astype(np.float32)
    return g, joint_matrices


def measure(pkg, torch, characters, frames):
    import numpy as np
    from test_animation import _fixture_rig
    gold = os.path.join(ROOT, "tests", "golden")
    rig = _fixture_rig(pkg, np.load(os.path.join(gold, "asset_animation.npz")), "cesiumman")
    fx = np.load(os.path.join(gold, "asset_cesiumman.npz"))
    g, joint_matrices = host_rig(pkg, rig)
    s = pkg.scenes.Scene()
    mat = s.add_material(color=(0.75, 0.55, 0.35), roughness=0.6)
    for k in range(characters):
        t = np.array(fx["node_transform"], np.float64)
        t[0, 3] += 1.5 * (k % 8)
        t[2, 3] += 1.5 * (k // 8)
        s.add_instance(s.add_mesh(fx["positions"], fx["indices"], normals=fx["normals"], material=mat), t)
    s.add_point_light((2.0, 4.0, -3.0), (40.0, 38.0, 35.0))
    s.set_test_sky(64, 32)
    c = pkg.RenderContext(device=0)
    c.init(64, 48)
    s.upload(c)
    c.set_setting("stage_timing", 1)
    for k in range(characters):
        c.set_mesh_skin(k, fx["joints"], fx["weights"], fx["normals"])
        c.set_rig(k, rig)
        c.bind_rig(k, k, skin=0)
    duration = float(rig["times"].max())
    ids = np.arange(characters)

    def times_of(frame):
        return ((frame * 0.033 + ids * duration / characters) % duration).astype(np.float32)

    def host_frame(frame, only_host=False):
        for k, t in enumerate(times_of(frame)):
            g.set_time(float(t))
            m = joint_matrices()
            if not only_host:
                c.pose_mesh(k, m)

    def device_frame(frame):
        c.animate(ids, times_of(frame), 0)

    def run(step):
        for f in range(5):  # (warm-up: allocations, code objects)
            step(f)
        c.wait()
        out = []
        for f in range(frames):
            c.wait()
            t0 = time.perf_counter()
            step(f)
            c.wait()
            out.append((time.perf_counter() - t0) * 1e3)
        return out
    host = run(host_frame)
    host_only = run(lambda f: host_frame(f, True))
    c.get_kernel_time("rig", reset=True)
    device = run(device_frame)
    rig_ms, rig_calls = c.get_kernel_time("rig")
    # the two paths leave the same geometry up to the host's float64 against the device's float32 joint matrices
    device_frame(0)
    dev = c.read_rig(characters - 1, "joints", 0)
    g.set_time(float(times_of(0)[-1]))
    diff = float(np.abs(dev - joint_matrices()).max())
    c.destroy()
    med = lambda v: round(sorted(v)[len(v) // 2], 4)  # noqa: E731
    return {"characters": characters, "nodes": len(rig["nodes"]), "joints": int(rig["skins"][0]["joint_count"]), "channels": len(rig["channels"]),
            "vertices_per_character": len(fx["positions"]), "frames": frames, "host_ms_median": med(host), "host_only_ms_median": med(host_only),
            "device_ms_median": med(device), "rig_kernel_ms_per_call": round(rig_ms / max(rig_calls, 1), 5), "rig_kernel_calls": rig_calls,
            "largest_joint_matrix_difference": diff, "host_ms": [round(x, 3) for x in host], "device_ms": [round(x, 3) for x in device]}


def main():
    import torch  # (first: torch's HIP runtime before librfwhip.so)
    from __graft_entry__ import load_package
    args = sys.argv[1:]
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "animation_time.json")
    frames = max(30, int(args[1])) if len(args) > 1 else 40
    pkg = load_package()
    rows = []
    for characters in (1, 64):
        rows.append(measure(pkg, torch, characters, frames))
        print(json.dumps({k: v for k, v in rows[-1].items() if not k.endswith("_ms")}), flush=True)
    result = {"what": "tools/animation_time.py: a frame's animation step (no update, no render) between two ctx.wait() fences: gltf.py's set_time and "
                      "joint matrices on the host + rfwhip_pose_mesh per character, against one rfwhip_animate call",
              "device": torch.cuda.get_device_name(0), "stage_timing": 1,
              "not_measured": ["rfwhip_update and the render behind the step", "morph rigs", "groups of several devices"], "rows": rows}
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
