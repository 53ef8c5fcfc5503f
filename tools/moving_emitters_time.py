"""Time moving emitters (setting lights_follow_geometry; include/rfwhip.h, csrc/light_follow.h) on one device, everything from ONE
process, written as one JSON file.  The lamp scene (scenes.lamp_scene: ground, two boxes, a lamp of n emissive triangles, two point
lights, a spot, a directional light) at 480 x 270, light_sampling=tree; the lamp's instance moves before every update.
  update    wall ms of rfwhip_set_instance + rfwhip_update per move, median / min / max of `repeats` moves, for
              device  lights_follow_geometry=1: the refresh kernel and the refit of the tree on the device inside the update
              host    today's route: the host derives the lamp's lights from its own triangles (vectorised numpy, timed apart as
                      host_derive_ms), hands them to rfwhip_set_lights — which rebuilds the tree on one host core — and updates
  variance  the per-pixel variance of `tree` after the lamp has moved by 0.5, 2 and 8 of its diameters, refit (the tree built where the
            lamp was) against freshly rebuilt (rfwhip_set_lights of the refreshed lights): mean over pixels of the variance of
            `frames` single frames of `spp` samples, and the ratio — when a host should force a rebuild
Usage: python tools/moving_emitters_time.py [out=profiles/moving_emitters_time.json] [repeats=7] [frames=16] [n ...=16 256 4096 65536]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: torch's HIP runtime before librfwhip.so)

from __graft_entry__ import load_package  # noqa: E402

W, H = 480, 270


def spread(v):
    s = sorted(v)
    return {"values": [round(x, 4) for x in v], "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 4), "min": round(s[0], 4), "max": round(s[-1], 4)}


def shift(k, step=0.05):
    m = np.eye(4)
    m[:3, 3] = (step * k, 0.0, 0.02 * k)
    return m


def setup(pkg, n, follow):
    scene = pkg.scenes.lamp_scene(n, W, H)
    scene.camera.clampValue = 1e9  # (clamping is not linear: two picking rules with different fireflies would differ in the mean)
    c = pkg.RenderContext(device=0)
    c.init(W, H)
    scene.upload(c)
    for k, v in dict(integrator="pt", spp=4, max_depth=2, light_sampling="tree", lights_follow_geometry=follow).items():
        c.set_setting(k, v)
    c.update()
    c.render_frame(scene.camera, pkg.RESET)  # (allocations, the tree)
    return scene, c, len(scene.instances) - 1


def host_lights(scene, lights, n, m):
    """the lamp's n lights under the transform m, as Scene.update_area_lights derives them (vectorised)"""
    out = lights.copy()
    r, t = m[:3, :3], m[:3, 3]
    v = [(lights[f][:n].astype(np.float64) @ r.T + t).astype(np.float32) for f in ("vertex0", "vertex1", "vertex2")]
    out["vertex0"][:n], out["vertex1"][:n], out["vertex2"][:n] = v
    out["position"][:n] = (v[0] + v[1] + v[2]) * np.float32(1.0 / 3.0)
    out["normal"][:n] = (lights["normal"][:n].astype(np.float64) @ np.linalg.inv(r)).astype(np.float32)
    return out


def time_updates(pkg, n, repeats):
    res = {}
    scene, c, inst = setup(pkg, n, 1)
    mesh = scene.instances[inst]["mesh"]
    ms = []
    for k in range(1, repeats + 2):
        t0 = time.perf_counter()
        c.set_instance(inst, mesh, shift(k))
        c.update()
        ms.append(1e3 * (time.perf_counter() - t0))
    res["device"] = dict(update_ms=spread(ms[1:]), lights_bound=int(c.get_setting("lights_bound")), refits=int(c.get_setting("light_tree_refits")))
    c.destroy()
    scene, c, inst = setup(pkg, n, 0)
    _, p, s, d = scene.light_arrays()
    ms, derive = [], []
    for k in range(1, repeats + 2):
        t0 = time.perf_counter()
        lights = host_lights(scene, scene.area_lights, n, shift(k))
        t1 = time.perf_counter()
        c.set_instance(inst, mesh, shift(k))
        c.set_lights(lights, p, s, d)
        c.update()
        ms.append(1e3 * (time.perf_counter() - t1))
        derive.append(1e3 * (t1 - t0))
    res["host"] = dict(update_ms=spread(ms[1:]), host_derive_ms=spread(derive[1:]))
    c.destroy()
    return res


def frame_variance(pkg, c, scene, frames):
    imgs, prev = [], None
    for k in range(1, frames + 1):
        c.render_frame(scene.camera, pkg.RESET if k == 1 else pkg.CONVERGE)
        m = c.framebuffer()[..., :3].astype(np.float64)
        imgs.append(m if prev is None else k * m - (k - 1) * prev)
        prev = m
    f = np.stack(imgs)
    return float(f.var(0, ddof=1).mean()), float(f.mean())


def variance_after_moves(pkg, n, frames):
    out = []
    diameter = 2.4  # (lamp_scene: radius 1.2)
    for d in (0.5, 2.0, 8.0):
        scene, c, inst = setup(pkg, n, 1)
        c.set_setting("spp", 8)
        m = np.eye(4)
        m[:3, 3] = (d * diameter * 0.6, 0.0, d * diameter * 0.8)
        c.set_instance(inst, scene.instances[inst]["mesh"], m)
        c.update()
        refits = int(c.get_setting("light_tree_refits"))
        v_refit, mean_refit = frame_variance(pkg, c, scene, frames)
        _, p, s, dd = scene.light_arrays()
        c.set_lights(c.read_area_lights(), p, s, dd)  # (the documented way to force a rebuild)
        c.update()
        v_built, mean_built = frame_variance(pkg, c, scene, frames)
        out.append(dict(diameters=d, refits=refits, refits_after_rebuild=int(c.get_setting("light_tree_refits")), variance_refit=v_refit,
                        variance_rebuilt=v_built, ratio=round(v_refit / max(v_built, 1e-30), 4), mean_refit=mean_refit, mean_rebuilt=mean_built))
        c.destroy()
    return out


def main():
    args = sys.argv[1:]
    out = args[0] if args else os.path.join(ROOT, "profiles", "moving_emitters_time.json")
    repeats = int(args[1]) if len(args) > 1 else 7
    frames = int(args[2]) if len(args) > 2 else 16
    sizes = [int(a) for a in args[3:]] or [16, 256, 4096, 65536]
    pkg = load_package()
    res = {"resolution": [W, H], "repeats": repeats, "frames": frames, "update": {}, "variance": {}}
    for n in sizes:
        res["update"][str(n)] = time_updates(pkg, n, repeats)
        print(json.dumps({"n": n, **res["update"][str(n)]}), flush=True)
    for n in (256, 4096):
        if n in sizes:
            res["variance"][str(n)] = variance_after_moves(pkg, n, frames)
            print(json.dumps({"n": n, "variance": res["variance"][str(n)]}), flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
