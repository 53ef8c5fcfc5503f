"""Time the primary wave with and without its entry snapshot (csrc/primary_entry.h) on one device: the bench's config 3
(terrain_1002k, 1920 x 1080, pt integrator depth 2) at streams=1, spp=64 — one sub-batch alone on the chip, stage by stage
(stage_timing=1).  One child process per value of the setting `primary_entry`, alternating, `repeats` each ("none": the setting is
left alone — for a library from before it existed).  Printed per child, as JSON lines:
  primary_ms   the primary stage alone (rfwhip_get_stats: primaryTime), per call, over `frames` calls with the camera at rest
  pass_us      the snapshot pass's own time (rfwhip_get_kernel_time, family 16) per pass, over `frames` calls that each ROTATE the
               camera a little (the ordered table stays, the records do not), and the passes counted at rest and moving
Usage: python tools/primary_entry_time.py [frames=6] [repeats=2] [grid=708] [values=0,1]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080


def child(frames, grid, value):
    import torch  # noqa: F401  (first: torch's HIP runtime before librfwhip.so)
    from __graft_entry__ import load_package
    pkg = load_package()
    scene = pkg.scenes.terrain(n=grid, width=W, height_px=H)
    ctx = pkg.RenderContext(device=0)
    ctx.init(W, H)
    scene.upload(ctx)
    for k, v in (("integrator", "pt"), ("spp", 64), ("max_depth", 2), ("streams", 1), ("stage_timing", 1)):
        ctx.set_setting(k, v)
    known = value != "none"
    if known:
        ctx.set_setting("primary_entry", value)
    cam = scene.camera
    ctx.render_frame(cam, pkg.RESET)
    if known:
        ctx.get_kernel_time(16, reset=True)
    prim = []
    for _ in range(frames):
        ctx.render_frame(cam, pkg.RESET)
        prim.append(round(ctx.get_stats().primaryTime, 4))
    out = {"primary_entry": value, "primary_ms": prim, "primary_ms_median": sorted(prim)[len(prim) // 2]}
    if known:
        out["on"] = ctx.get_setting("primary_entry_on")
        out["passes_at_rest"] = ctx.get_kernel_time(16, reset=True)[1]
        d = cam.direction
        for k in range(frames):
            cam.direction = (d[0] + 1e-4 * (k + 1), d[1], d[2])
            ctx.render_frame(cam, pkg.RESET)
        ms, n = ctx.get_kernel_time(16)
        out["passes_moving"], out["pass_us"] = n, round(1000.0 * ms / n, 2) if n else None
    print(json.dumps(out), flush=True)
    ctx.destroy()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
        sys.exit(0)
    frames, repeats, grid = [int(a) for a in (sys.argv[1:4] + ["6", "2", "708"][len(sys.argv) - 1:])]
    values = (sys.argv[4] if len(sys.argv) > 4 else "0,1").split(",")
    for _ in range(repeats):
        for value in values:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(frames), str(grid), value],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit("child failed (primary_entry=%s, exit %d):\n%s" % (value, r.returncode, r.stderr[-2000:]))
            print(r.stdout.strip().splitlines()[-1], flush=True)
