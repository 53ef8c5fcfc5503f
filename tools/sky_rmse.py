"""RMSE at equal time of sky_sampling=0 / 1 against a converged image, on the 1080p bench terrain with and without its lights.

usage (on the GPU box): python tools/sky_rmse.py [--ref-spp 4096] [--budget-ms 200] [--width 1920 --height 1080]

For each scene: the reference is --ref-spp samples of the default estimator (sky_sampling=0; with lights the two estimators
converge to slightly different images, DESIGN.md section 11, so the "lights" line also carries that offset).  Each mode's time per
sample is measured with 16-spp frames (best of 3, after a warm-up frame, on the context that then renders); the mode then renders as many samples as fit in --budget-ms (a multiple of 4) and its RMSE
against the reference is printed as one JSON line per scene and mode."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__  # noqa: E402


def context(pkg, scene, w, h, sky):
    c = pkg.RenderContext(device=0)
    c.init(w, h)
    scene.upload(c)
    for k, v in {"integrator": "pt", "max_depth": 2, "sky_sampling": sky}.items():
        c.set_setting(k, v)
    return c


def render(pkg, c, scene, spp, batch=256):
    """spp samples in calls of `batch`, read back; seconds from the first call to the image on the host."""
    done = 0
    t0 = time.perf_counter()
    while done < spp:
        n = min(batch, spp - done)
        c.set_setting("spp", n)
        c.render_frame(scene.camera, pkg.RESET if done == 0 else pkg.CONVERGE)
        done += n
    img = c.framebuffer()[..., :3].astype(np.float64)
    return img, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--budget-ms", type=float, default=200.0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    for lights in (False, True):
        scene = pkg.scenes.terrain(n=708, width=a.width, height_px=a.height, lights=lights)
        ref, ref_s = render(pkg, context(pkg, scene, a.width, a.height, 0), scene, a.ref_spp)
        for sky in (0, 1):
            c = context(pkg, scene, a.width, a.height, sky)
            render(pkg, c, scene, 16, batch=16)  # (warm-up: code objects, buffers, the table)
            t16 = min(render(pkg, c, scene, 16, batch=16)[1] for _ in range(3))
            spp = max(4, int(a.budget_ms / 1e3 / (t16 / 16)) // 4 * 4)
            img, t = render(pkg, c, scene, spp, batch=spp)
            rmse = float(np.sqrt(((img - ref) ** 2).mean()))
            print(json.dumps({"scene": "terrain" + ("" if lights else "_no_lights"), "sky_sampling": sky, "spp": spp,
                              "ms": round(1e3 * t, 2), "ms_per_spp": round(1e3 * t16 / 16, 3), "rmse": rmse,
                              "ref_spp": a.ref_spp, "ref_s": round(ref_s, 1)}), flush=True)


if __name__ == "__main__":
    main()
