"""Time the display stage (include/rfwhip.h, rfwhip_read_display; csrc/display.h) on one device at 1920 x 1080, on the terrain
(BASELINE config 3's scene) rendered at 1 spp per frame.  Two measurements, written as one JSON file:
  kernel   k_display alone, with hipEvents (stage_timing=1, kernel family 7), FXAA on and off, RGBA8 and RGBA32F: the stage on the
           rendered frame, `frames` times per variant (rfwhip_read_display_device: only the display launch is in the family)
  present  wall time per frame of the pipelined present loop of a group of one device — render(k), present into slot k % 2, wait
           for slot (k + 1) % 2: two frames in flight — once with the float pair (rfwhip_group_present_async / _wait: what the
           library did before the stage existed, 16 B per pixel over PCIe) and once with the display pair
           (rfwhip_group_present_display_async / _wait, RGBA8: 4 B per pixel).  The two loops ALTERNATE, `repeats` times each, in
           one process: the spread of a loop's repeats is the yardstick for the difference between the two.
Usage: python tools/display_time.py [out=profiles/display_time.json] [frames=300] [repeats=4]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: torch's HIP runtime before librfwhip.so)

from __graft_entry__ import load_package  # noqa: E402

W, H = 1920, 1080
PIXELS = W * H
SLOTS = 2


def kernel_times(pkg, scene, frames):
    ctx = pkg.RenderContext(device=0)
    ctx.init(W, H)
    scene.upload(ctx)
    for k, v in dict(integrator="pt", spp=1, stage_timing=1).items():
        ctx.set_setting(k, v)
    ctx.render_frame(scene.camera, pkg.RESET)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    rows = []
    for fxaa in (1, 0):
        ctx.set_setting("display_fxaa", fxaa)
        for fmt, bpp in (("rgba8", 4), ("rgba32f", 16)):
            def run(n):
                for _ in range(n):
                    ctx.read_display_device(out.data_ptr(), fmt)
                ctx.wait()  # (resolves the timed spans)
            run(10)
            ctx.get_kernel_time("display", reset=True)
            run(frames)
            ms, launches = ctx.get_kernel_time("display", reset=True)
            us = ms * 1e3 / max(launches, 1)
            nbytes = PIXELS * (16 + bpp)  # the image read once, the output written once
            rows.append({"fxaa": fxaa, "format": fmt, "launches": launches, "us_per_launch": round(us, 2),
                         "bytes_unique": nbytes, "GBps_unique": round(nbytes / us / 1e3, 1)})
            print(json.dumps(rows[-1]), flush=True)
    ctx.destroy()
    return rows


def present_loops(pkg, scene, frames, repeats):
    g = pkg.render_group([0], "peer")
    g.init(W, H)
    scene.upload(g)
    for k, v in dict(integrator="pt", spp=1).items():
        g.set_setting(k, v)

    def loop(display, n):
        post = (lambda s: g.present_display_async(s, "rgba8")) if display else g.present_async
        wait = g.present_display_wait if display else g.present_wait
        checksum = 0
        for k in range(n):
            g.render_async(scene.camera, pkg.RESET)
            post(k % SLOTS)
            if k >= SLOTS - 1:
                checksum += int(wait((k + 1) % SLOTS)[0, 0, 0] > -1)  # (touch the landed image)
        for k in range(n - SLOTS + 1, n):
            wait(k % SLOTS)
        g.wait()
        return checksum

    out = {"float": [], "display": []}
    for r in range(repeats):
        for name, display in (("float", False), ("display", True)):
            loop(display, 20)  # (warm up: also re-labels the slots for this kind)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(display, frames)
            torch.cuda.synchronize()
            out[name].append(round((time.perf_counter() - t0) * 1e3 / frames, 4))
            print(json.dumps({"loop": name, "repeat": r, "ms_per_frame": out[name][-1]}), flush=True)
    g.destroy()
    res = {}
    for name, bpp in (("float", 16), ("display", 4)):
        v = sorted(out[name])
        res[name] = {"ms_per_frame": out[name], "median_ms_per_frame": round((v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, 4),
                     "min_ms_per_frame": v[0], "max_ms_per_frame": v[-1], "copy_bytes_per_frame": PIXELS * bpp}
    return res


def main():
    args = sys.argv[1:]
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "display_time.json")
    frames = int(args[1]) if len(args) > 1 else 300
    repeats = int(args[2]) if len(args) > 2 else 4
    pkg = load_package()
    scene = pkg.scenes.terrain(width=W, height_px=H)
    result = {"what": "tools/display_time.py: the display stage at 1920 x 1080 on one MI355X, terrain_1002k, 1 spp per frame",
              "frames": frames, "repeats": repeats, "slots_in_flight": SLOTS,
              "kernel": kernel_times(pkg, scene, frames), "present": present_loops(pkg, scene, frames, repeats)}
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["present"]))


if __name__ == "__main__":
    main()
