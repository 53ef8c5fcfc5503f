"""Time the exposure meter (include/rfwhip.h, rfwhip_get_meter; csrc/metering.h) on one device at 1920 x 1080.  Two measurements,
written as one JSON file:
  kernel   with hipEvents (stage_timing=1), `frames` launches per row, through rfwhip_display_stream on an image in device memory
           (display_exposure = auto: every call is one step — k_meter_hist, k_meter_reduce — and one exposed display launch):
           k_meter_hist (family 9) and k_meter_reduce (family 10) on three images — the rendered terrain frame, gamma noise (every
           wave meets many bins) and a constant (every lane of every wave meets ONE bin: the worst case for LDS atomics, which
           the wave-uniform path of k_meter_hist answers with one atomic per wave) — and the display kernels (family 7) in the same
           run: k_display (manual, ev 0) beside its exposed twin k_display_exposed (manual, ev 1), FXAA on and off, both formats.
           The yardstick for k_meter_hist is k_display<false> to RGBA32F: it reads the same 33 MB and also writes 33 MB.
  present  wall time per frame of the pipelined present loop of a group of one device (two frames in flight, RGBA8 through
           rfwhip_group_present_display_async / _wait) with display_exposure = manual and = auto, ALTERNATING, `repeats` times
           each, in one process: the spread of a loop's repeats is the yardstick for the difference between the two.
Usage: python tools/metering_time.py [out=profiles/metering_time.json] [frames=300] [repeats=4]"""
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
    rendered = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    ctx.read_framebuffer_device(rendered.data_ptr())
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    noise = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0").exponential_(0.5, generator=gen) ** 2
    constant = torch.full((H, W, 4), 0.5, dtype=torch.float32, device="cuda:0")
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    families = ("meter_hist", "meter_reduce", "display")
    side = torch.cuda.Stream(device="cuda:0")  # (a stream of the caller's, not the null stream: the hipEvents ride it)
    torch.cuda.synchronize()

    def timed(image, fmt, n):
        def run(k):
            for _ in range(k):
                ctx.display_stream(image.data_ptr(), out.data_ptr(), fmt, side.cuda_stream)
            side.synchronize()
            ctx.wait()  # (resolves the timed spans)
        run(10)
        for f in families:
            ctx.get_kernel_time(f, reset=True)
        run(n)
        res = {}
        for f in families:
            ms, launches = ctx.get_kernel_time(f, reset=True)
            res[f] = (round(ms * 1e3 / max(launches, 1), 2), launches)
        return res

    meter, display = [], []
    ctx.set_setting("display_exposure", "auto")
    ctx.set_setting("display_fxaa", 0)
    for name, image in (("rendered", rendered), ("noise", noise), ("constant", constant)):
        r = timed(image, "rgba32f", frames)
        us = r["meter_hist"][0]
        meter.append({"image": name, "launches": r["meter_hist"][1], "k_meter_hist_us": us, "k_meter_reduce_us": r["meter_reduce"][0],
                      "k_display_exposed_us": r["display"][0], "hist_bytes": PIXELS * 16, "hist_GBps": round(PIXELS * 16 / max(us, 1e-9) / 1e3, 1),
                      "valid_pixels": ctx.meter()["valid"]})
        print(json.dumps(meter[-1]), flush=True)
    ctx.set_setting("display_exposure", "manual")
    for fxaa in (1, 0):
        ctx.set_setting("display_fxaa", fxaa)
        for fmt in ("rgba8", "rgba32f"):
            row = {"fxaa": fxaa, "format": fmt}
            for ev, key in ((0, "k_display_us"), (1, "k_display_exposed_us"), (0, "k_display_again_us")):
                ctx.set_setting("display_exposure_ev", ev)
                row[key] = timed(rendered, fmt, frames)["display"][0]
            display.append(row)
            print(json.dumps(row), flush=True)
    ctx.destroy()
    return {"meter": meter, "display": display}


def present_loops(pkg, scene, frames, repeats):
    g = pkg.render_group([0], "peer")
    g.init(W, H)
    scene.upload(g)
    for k, v in dict(integrator="pt", spp=1).items():
        g.set_setting(k, v)

    def loop(n):
        checksum = 0
        for k in range(n):
            g.render_async(scene.camera, pkg.RESET)
            g.present_display_async(k % SLOTS, "rgba8")
            if k >= SLOTS - 1:
                checksum += int(g.present_display_wait((k + 1) % SLOTS)[0, 0, 0] > -1)  # (touch the landed image)
        for k in range(n - SLOTS + 1, n):
            g.present_display_wait(k % SLOTS)
        g.wait()
        return checksum

    out = {"manual": [], "auto": []}
    for r in range(repeats):
        for mode in ("manual", "auto"):
            g.set_setting("display_exposure", mode)
            loop(20)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(frames)
            torch.cuda.synchronize()
            out[mode].append(round((time.perf_counter() - t0) * 1e3 / frames, 4))
            print(json.dumps({"loop": mode, "repeat": r, "ms_per_frame": out[mode][-1]}), flush=True)
    steps = g.meter()["steps"]
    g.destroy()
    res = {"auto_steps": steps}
    for mode in ("manual", "auto"):
        v = sorted(out[mode])
        res[mode] = {"ms_per_frame": out[mode], "median_ms_per_frame": round((v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, 4),
                     "min_ms_per_frame": v[0], "max_ms_per_frame": v[-1]}
    return res


def main():
    args = sys.argv[1:]
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "metering_time.json")
    frames = int(args[1]) if len(args) > 1 else 300
    repeats = int(args[2]) if len(args) > 2 else 4
    pkg = load_package()
    scene = pkg.scenes.terrain(width=W, height_px=H)
    result = {"what": "tools/metering_time.py: the exposure meter at 1920 x 1080 on one MI355X, terrain_1002k, 1 spp per frame",
              "frames": frames, "repeats": repeats, "slots_in_flight": SLOTS,
              "kernel": kernel_times(pkg, scene, frames), "present": present_loops(pkg, scene, frames, repeats)}
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["present"]))


if __name__ == "__main__":
    main()
