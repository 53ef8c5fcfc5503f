"""Time the primary wave with and without the camera-ordered node table (csrc/primary_order.h) on one device: the bench's config 3
(terrain_1002k, 1920 x 1080, pt integrator depth 2) at streams=1, spp=64 — one sub-batch alone on the chip, stage by stage
(stage_timing=1).  One child process per value of RFWHIP_PRIMARY_ORDER (it is read when a context is created), alternating,
`repeats` each.  Printed per child, as JSON lines:
  primary_ms   the primary stage alone (rfwhip_get_stats: primaryTime), per call, over `frames` calls with the camera at rest
  pass_us      the ordering pass's own time (rfwhip_get_kernel_time, family 11) per pass, over `frames` calls that each move the
               camera by a millimetre (=1 only), and the table's bytes
Usage: python tools/primary_order_time.py [frames=6] [repeats=3] [grid=708]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080


def child(frames, grid):
    import torch  # noqa: F401  (first: torch's HIP runtime before librfwhip.so)
    from __graft_entry__ import load_package
    pkg = load_package()
    scene = pkg.scenes.terrain(n=grid, width=W, height_px=H)
    ctx = pkg.RenderContext(device=0)
    ctx.init(W, H)
    scene.upload(ctx)
    for k, v in (("integrator", "pt"), ("spp", 64), ("max_depth", 2), ("streams", 1), ("stage_timing", 1)):
        ctx.set_setting(k, v)
    cam = scene.camera
    ctx.render_frame(cam, pkg.RESET)
    ctx.get_kernel_time("primary_order", reset=True)
    prim = []
    for _ in range(frames):
        ctx.render_frame(cam, pkg.RESET)
        prim.append(round(ctx.get_stats().primaryTime, 4))
    at_rest = ctx.get_kernel_time("primary_order", reset=True)[1]
    x = cam.position[0]
    for k in range(frames):
        cam.position = (x + 0.001 * (k + 1), cam.position[1], cam.position[2])
        ctx.render_frame(cam, pkg.RESET)
    ms, n = ctx.get_kernel_time("primary_order")
    print(json.dumps({"RFWHIP_PRIMARY_ORDER": os.environ.get("RFWHIP_PRIMARY_ORDER"), "primary_ms": prim, "primary_ms_median": sorted(prim)[len(prim) // 2],
                      "passes_at_rest": at_rest, "passes_moving": n, "pass_us": round(1000.0 * ms / n, 2) if n else None}), flush=True)
    ctx.destroy()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
        sys.exit(0)
    frames, repeats, grid = [int(a) for a in (sys.argv[1:4] + ["6", "3", "708"][len(sys.argv) - 1:])]
    for _ in range(repeats):
        for order in ("0", "1"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(frames), str(grid)],
                               env=dict(os.environ, RFWHIP_PRIMARY_ORDER=order), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit("child failed (RFWHIP_PRIMARY_ORDER=%s, exit %d):\n%s" % (order, r.returncode, r.stderr[-2000:]))
            print(r.stdout.strip().splitlines()[-1], flush=True)
