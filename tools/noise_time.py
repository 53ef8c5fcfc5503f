"""Time the noise estimate (include/rfwhip.h, rfwhip_get_noise; csrc/noise.h) on one device: the bench's config 3 (terrain_1002k,
1920 x 1080, pt integrator, `spp` samples per step), everything from ONE process, written as one JSON file:
  resolve  the resolve launch of a render call with hipEvents (stage_timing=1, kernel family "finalize": the resolve is its only
           launch here), noise_estimate=0 — k_resolve, whose code is the parent commit's instruction for instruction
           (tools/dev/isa_same.py --labels) — against noise_estimate=1, k_resolve_noise.  The two ALTERNATE, `repeats` blocks each
           of a RESET call and `steps` CONVERGE calls: the spread of a setting's own blocks is the yardstick for the difference.
  metric   k_noise_tiles + k_noise_final (kernel family "noise", two launches per query), `queries` queries in a row per block,
           and the wall time of a query as the host sees it (launches + 32-byte copy + wait) on an idle stream.
Usage: python tools/noise_time.py [out=profiles/noise_time.json] [spp=256] [steps=6] [repeats=5] [queries=200]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: torch's HIP runtime before librfwhip.so)

from __graft_entry__ import load_package  # noqa: E402

W, H = 1920, 1080
PIXELS = W * H


def spread(v):
    s = sorted(v)
    return {"values": v, "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 3), "min": s[0], "max": s[-1]}


def main():
    args = sys.argv[1:]
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "noise_time.json")
    spp, steps, repeats, queries = (int(args[i]) if len(args) > i else d for i, d in ((1, 256), (2, 6), (3, 5), (4, 200)))
    pkg = load_package()
    scene = pkg.scenes.terrain(width=W, height_px=H)
    ctx = pkg.RenderContext(device=0)
    ctx.init(W, H)
    scene.upload(ctx)
    for k, v in dict(integrator="pt", spp=spp, max_depth=2, stage_timing=1).items():
        ctx.set_setting(k, v)

    def block(noise):
        ctx.set_setting("noise_estimate", noise)
        ctx.render_frame(scene.camera, pkg.RESET)
        ctx.get_kernel_time("finalize", reset=True)
        for _ in range(steps):
            ctx.render_async(scene.camera, pkg.CONVERGE)
        ctx.wait()
        ms, launches = ctx.get_kernel_time("finalize", reset=True)
        assert launches == steps, (launches, steps)
        return round(ms * 1e3 / launches, 2)

    block(0), block(1)  # (warm up: buffers, clocks)
    us = {0: [], 1: []}
    metric_us, query_us = [], []
    for r in range(repeats):
        for noise in (0, 1):
            us[noise].append(block(noise))
            print(json.dumps({"repeat": r, "noise_estimate": noise, "resolve_us": us[noise][-1]}), flush=True)
        # (the moments of the block above are live: the metric on them)
        ctx.get_noise()
        ctx.get_kernel_time("noise", reset=True)
        t0 = time.perf_counter()
        for _ in range(queries):
            st = ctx.get_noise()
        wall = time.perf_counter() - t0
        ctx.wait()
        ms, launches = ctx.get_kernel_time("noise", reset=True)
        assert launches == 2 * queries, (launches, queries)
        metric_us.append(round(ms * 1e3 / queries, 2))
        query_us.append(round(wall * 1e6 / queries, 2))
        print(json.dumps({"repeat": r, "metric_us": metric_us[-1], "query_wall_us": query_us[-1], "stats": st}), flush=True)
    slot_bytes = PIXELS * spp * 32  # a radiance and a connection record per sample
    off, on = spread(us[0]), spread(us[1])
    result = {"what": "tools/noise_time.py: the noise estimate at 1920 x 1080 on one MI355X, terrain_1002k, pt integrator depth 2, "
                      "%d spp per step" % spp,
              "spp": spp, "steps_per_block": steps, "repeats": repeats, "queries_per_block": queries,
              "resolve": {"k_resolve_us": off, "k_resolve_noise_us": on,
                          "difference_of_medians_us": round(on["median"] - off["median"], 3),
                          "spread_of_k_resolve_us": round(off["max"] - off["min"], 3),
                          "slot_bytes_read_per_launch": slot_bytes, "moment_bytes_per_launch": PIXELS * 16,
                          "k_resolve_GBps_of_slot_bytes": round(slot_bytes / off["median"] / 1e3, 1),
                          "k_resolve_noise_GBps_of_slot_bytes": round(slot_bytes / on["median"] / 1e3, 1)},
              "metric": {"kernels_us_per_query": spread(metric_us), "wall_us_per_query": spread(query_us),
                         "bytes_per_query": PIXELS * 12, "last_stats": st}}
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["resolve"]))
    ctx.destroy()


if __name__ == "__main__":
    main()
