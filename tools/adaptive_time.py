"""Time adaptive sampling (include/rfwhip.h, rfwhip_get_adaptive; csrc/adaptive.h) on one device: the bench's config 3 (terrain_1002k,
1920 x 1080, pt integrator depth 2) at `spp` samples per call (default: 256 and 1), everything from ONE process, written as one JSON
file.  A block is a RESET call and then `steps` pipelined CONVERGE calls with one wait; its figure is the wall time of those calls
per call.  The settings ALTERNATE block by block, `repeats` blocks each: the spread (max - min) of a setting's own blocks is the
yardstick for a difference between two settings.
  overhead  nothing retires (noise_threshold 1e-12): adaptive_sampling = 1 at adaptive_every 1 and 4 against noise_estimate = 1 alone,
            whose kernels are the parent commit's instruction for instruction (tools/dev/isa_same.py --labels).  The difference of the
            medians in units of the spread of the noise_estimate blocks: the masked primary wave, the per-tile resolve, k_adaptive_step
            and k_adaptive_connections on every call, the metric and the event wait on the decision calls.
  masks     forced masks (rfwhip_adaptive_set_tiles behind the RESET call) with 75 / 50 / 25 / 0 % of the tiles active, beside the
            100 % of the overhead blocks.  Expectation, written down before the run: time = fixed + active share x rest, where fixed is
            the 0 % figure (full-size launches whose waves leave at once, the resolve's early returns, the bookkeeping kernels) and rest
            is the 100 % figure minus it.  `expected_ms` and `measured / expected` say whether it holds.
Usage: python tools/adaptive_time.py [out=profiles/adaptive_time.json] [steps=6] [repeats=5] [spp ...=256 1]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: torch's HIP runtime before librfwhip.so)

from __graft_entry__ import load_package  # noqa: E402

W, H = 1920, 1080


def spread(v):
    s = sorted(v)
    return {"values": v, "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 4), "min": s[0], "max": s[-1]}


def measure(pkg, ctx, scene, spp, steps, repeats):
    ctx.set_setting("spp", spp)

    def block(adaptive, every=4, quarters=4):
        """ms per CONVERGE call; quarters < 4: that many of every four tiles stay active"""
        ctx.set_setting("adaptive_sampling", adaptive)
        ctx.set_setting("adaptive_every", every)
        ctx.render_frame(scene.camera, pkg.RESET)
        share = 1.0
        if adaptive and quarters < 4:
            n, _ = ctx.read_adaptive_tiles()
            yy, xx = np.mgrid[:n.shape[0], :n.shape[1]]
            ctx.adaptive_set_tiles((yy + xx) % 4 < quarters)
            st = ctx.get_adaptive()
            share = st["active_pixels"] / st["pixels"]
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.render_async(scene.camera, pkg.CONVERGE)
        ctx.wait()
        return round((time.perf_counter() - t0) * 1e3 / steps, 4), share

    block(0), block(1, 1), block(1, 4, 0)  # (warm up: buffers, clocks)
    kinds = [("noise_estimate", (0,)), ("adaptive_every_1", (1, 1)), ("adaptive_every_4", (1, 4))] + \
            [("active_%d" % (25 * q), (1, 4, q)) for q in (3, 2, 1, 0)]
    ms, shares = {k: [] for k, _ in kinds}, {}
    for r in range(repeats):
        for k, args in kinds:
            t, shares[k] = block(*args)
            ms[k].append(t)
            print(json.dumps({"spp": spp, "repeat": r, "block": k, "ms_per_call": t, "active_share": round(shares[k], 4)}), flush=True)
    base = spread(ms["noise_estimate"])
    yard = round(base["max"] - base["min"], 4)
    out = {"spp": spp, "steps_per_block": steps, "repeats": repeats, "noise_estimate_ms": base, "spread_of_noise_estimate_ms": yard, "overhead": {}, "masks": {}}
    for k in ("adaptive_every_1", "adaptive_every_4"):
        s = spread(ms[k])
        d = round(s["median"] - base["median"], 4)
        out["overhead"][k] = {"ms": s, "difference_of_medians_ms": d, "in_spreads_of_noise_estimate": round(d / yard, 2) if yard > 0 else None}
    full, fixed = spread(ms["adaptive_every_4"])["median"], spread(ms["active_0"])["median"]
    out["masks"]["fixed_ms_at_0"] = fixed
    out["masks"]["rest_ms"] = round(full - fixed, 4)
    for k in ("active_75", "active_50", "active_25", "active_0"):
        s = spread(ms[k])
        want = round(fixed + shares[k] * (full - fixed), 4)
        out["masks"][k] = {"active_share": round(shares[k], 4), "ms": s, "expected_ms": want, "measured_over_expected": round(s["median"] / want, 3)}
    return out


def main():
    args = sys.argv[1:]
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "adaptive_time.json")
    steps, repeats = (int(args[i]) if len(args) > i else d for i, d in ((1, 6), (2, 5)))
    spps = [int(a) for a in args[3:]] or [256, 1]
    pkg = load_package()
    scene = pkg.scenes.terrain(width=W, height_px=H)
    ctx = pkg.RenderContext(device=0)
    ctx.init(W, H)
    scene.upload(ctx)
    for k, v in dict(integrator="pt", max_depth=2, noise_estimate=1, noise_threshold="1e-12", adaptive_min_samples=2).items():
        ctx.set_setting(k, v)
    result = {"what": "tools/adaptive_time.py: adaptive sampling at 1920 x 1080 on one MI355X, terrain_1002k, pt integrator depth 2; wall ms "
                      "per pipelined CONVERGE call",
              "expectation": "time = fixed (the 0 % figure) + active share x (the 100 % figure - fixed)",
              "runs": [measure(pkg, ctx, scene, spp, steps if spp > 16 else steps * 8, repeats) for spp in spps]}
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for run in result["runs"]:
        print(json.dumps({"spp": run["spp"], "overhead": {k: v["in_spreads_of_noise_estimate"] for k, v in run["overhead"].items()},
                          "masks": {k: v["measured_over_expected"] for k, v in run["masks"].items() if isinstance(v, dict)}}))
    ctx.destroy()


if __name__ == "__main__":
    main()
