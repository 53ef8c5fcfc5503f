"""Time the three light_sampling modes (reference | linear | tree; csrc/light_tree.h) on the lamp scene
(scenes.lamp_scene: a bumpy ground, two boxes, a lamp of n emissive triangles) at 1920 x 1080, spp 1, max_depth 2.  One JSON line
per light count and mode:
  frame_ms   wall time of a frame (render + wait), the best of `frames`
  shade_ms   the shade stage's kernels per frame (hipEvents: stage_timing=1, kernel family "shade"), in a run of its own
  variance   the mean per-pixel variance of the frames of a converging sequence (`linear` and `tree` have the same expectation, so their
             ratio is the price of the tree's coarser choice), with the image mean beside it
A mode whose frame would take too long is skipped: `reference` and `linear` evaluate every light at every vertex, and beyond
--linear-max lights (default 4096) only `tree` runs.
Usage: python tools/light_tree_time.py [--lights 16,256,4096,65536] [--frames 8] [--linear-max 4096] [--size 1920x1080]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: torch's HIP runtime before librfwhip.so)
import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def measure(pkg, scene, w, h, mode, frames):
    ctx = pkg.RenderContext(device=0)
    ctx.init(w, h)
    scene.upload(ctx)
    for k, v in {"integrator": "pt", "spp": 1, "max_depth": 2, "light_sampling": mode}.items():
        ctx.set_setting(k, v)
    ctx.render_frame(scene.camera, pkg.RESET)  # (warm-up: allocations, the tree)
    best, s1, s2, prev = 1e9, 0.0, 0.0, None
    for k in range(1, frames + 1):  # (a converging sequence: every frame has samples of its own)
        t0 = time.perf_counter()
        ctx.render_frame(scene.camera, pkg.RESET if k == 1 else pkg.CONVERGE)
        best = min(best, time.perf_counter() - t0)
        m = ctx.framebuffer()[..., :3].astype(np.float64)
        f = m if prev is None else k * m - (k - 1) * prev  # (this frame's own samples out of the running mean)
        prev = m
        s1, s2 = s1 + f, s2 + f * f
    var = float(((s2 - s1 * s1 / frames) / max(1, frames - 1)).mean())
    ctx.set_setting("stage_timing", 1)
    ctx.render_frame(scene.camera, pkg.RESET)
    ctx.get_kernel_time("shade", reset=True)
    for _ in range(frames):
        ctx.render_frame(scene.camera, pkg.RESET)
    ms, launches = ctx.get_kernel_time("shade", reset=True)
    out = {"mode": mode, "light_tree": int(ctx.get_setting("light_tree")), "frame_ms": round(best * 1e3, 3),
           "shade_ms": round(ms / frames, 3), "shade_launches": launches // frames, "variance": var, "mean": float((s1 / frames).mean())}
    ctx.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lights", default="16,256,4096,65536")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--linear-max", type=int, default=4096)
    ap.add_argument("--size", default="1920x1080")
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.split("x"))
    pkg = load_package()
    for n in (int(x) for x in a.lights.split(",")):
        scene = pkg.scenes.lamp_scene(n, w, h, extras=False)
        scene.camera.clampValue = 1e9
        for mode in ("reference", "linear", "tree"):
            if mode != "tree" and n > a.linear_max:
                print(json.dumps({"lights": n, "mode": mode, "skipped": "more than --linear-max lights"}), flush=True)
                continue
            print(json.dumps(dict(lights=n, **measure(pkg, scene, w, h, mode, a.frames))), flush=True)


if __name__ == "__main__":
    main()
