"""Time bloom (include/rfwhip.h, rfwhip_bloom_image; csrc/bloom.h) on one device at 1920 x 1080.  Two measurements, written as one
JSON file:
  kernel   with hipEvents (stage_timing=1, one span per launch), `frames` calls per row, through rfwhip_display_stream on an image in
           device memory with display_bloom = 1: each kernel of the chain (the read-only setting display_bloom_time splits family 12
           into k_bloom_down0, k_bloom_down, k_bloom_up, k_bloom_apply), the whole chain, and the display kernel of the same run —
           on the rendered terrain frame and on HDR noise, with display_bloom_levels = 1 .. 8: the growth from one level count to the
           next is one down and one up launch on ever smaller levels, the tail of small launches.  The yardstick for one full-image
           pass is k_display<false> to RGBA32F with bloom off, timed in the same run: it reads and writes 33 MB each.
  present  wall time per frame of the pipelined present loop of a group of one device (two frames in flight, RGBA8 through
           rfwhip_group_present_display_async / _wait) with display_bloom = 0 and = 1, ALTERNATING, `repeats` times each, in one
           process: the spread of a loop's repeats is the yardstick for the difference between the two.
Usage: python tools/bloom_time.py [out=profiles/bloom_time.json] [frames=300] [repeats=4]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: torch's HIP runtime before librfwhip.so)

from __graft_entry__ import load_package  # noqa: E402

W, H = 1920, 1080
SLOTS = 2
KERNELS = ("k_bloom_down0", "k_bloom_down", "k_bloom_up", "k_bloom_apply")


def kernel_times(pkg, scene, frames):
    ctx = pkg.RenderContext(device=0)
    ctx.init(W, H)
    scene.upload(ctx)
    for k, v in dict(integrator="pt", spp=1, stage_timing=1, display_fxaa=0).items():
        ctx.set_setting(k, v)
    ctx.render_frame(scene.camera, pkg.RESET)
    rendered = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    ctx.read_framebuffer_device(rendered.data_ptr())
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    noise = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0").exponential_(0.5, generator=gen) ** 2
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    side = torch.cuda.Stream(device="cuda:0")  # (a stream of the caller's, not the null stream: the hipEvents ride it)
    torch.cuda.synchronize()

    def timed(image, n):
        def run(k):
            for _ in range(k):
                ctx.display_stream(image.data_ptr(), out.data_ptr(), "rgba32f", side.cuda_stream)
            side.synchronize()
            ctx.wait()  # (resolves the timed spans)
        run(10)
        for f in ("bloom", "display"):
            ctx.get_kernel_time(f, reset=True)
        run(n)
        v = ctx.get_setting("display_bloom_time").split()
        ms, launches = [float(x) for x in v[:4]], [int(x) for x in v[4:]]
        row = {name + "_us": round(ms[i] * 1e3 / launches[i], 2) if launches[i] else None for i, name in enumerate(KERNELS)}
        row.update({name + "_launches_per_chain": launches[i] // n for i, name in enumerate(KERNELS)})
        chain_ms, chain_launches = ctx.get_kernel_time("bloom", reset=True)
        row["chain_us"] = round(chain_ms * 1e3 / n, 2)
        row["chain_launches"] = chain_launches // n
        row["k_display_us"] = round(ctx.get_kernel_time("display", reset=True)[0] * 1e3 / n, 2)
        return row

    rows = []
    yard = {}
    for name, image in (("rendered", rendered), ("noise", noise)):
        ctx.set_setting("display_bloom", 0)
        yard[name] = timed(image, frames)["k_display_us"]
        ctx.set_setting("display_bloom", 1)
        for levels in (1, 2, 3, 4, 5, 6, 7, 8):
            ctx.set_setting("display_bloom_levels", levels)
            row = dict({"image": name, "levels": levels}, **timed(image, frames))
            row["k_display_pointwise_rgba32f_bloom_off_us"] = yard[name]
            rows.append(row)
            print(json.dumps(row), flush=True)
    ctx.destroy()
    # the tail: what the levels behind the third (below 240 x 135) add to the default chain of six
    by = {(r["image"], r["levels"]): r for r in rows}
    tail = {name: {"chain_6_us": by[(name, 6)]["chain_us"], "chain_3_us": by[(name, 3)]["chain_us"],
                   "levels_4_to_6_us": round(by[(name, 6)]["chain_us"] - by[(name, 3)]["chain_us"], 2),
                   "share_of_chain_6": round((by[(name, 6)]["chain_us"] - by[(name, 3)]["chain_us"]) / max(by[(name, 6)]["chain_us"], 1e-9), 3)}
            for name in ("rendered", "noise")}
    return {"rows": rows, "tail": tail}


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

    out = {"off": [], "on": []}
    for r in range(repeats):
        for mode in ("off", "on"):
            g.set_setting("display_bloom", int(mode == "on"))
            loop(20)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(frames)
            torch.cuda.synchronize()
            out[mode].append(round((time.perf_counter() - t0) * 1e3 / frames, 4))
            print(json.dumps({"loop": mode, "repeat": r, "ms_per_frame": out[mode][-1]}), flush=True)
    g.destroy()
    res = {}
    for mode in ("off", "on"):
        v = sorted(out[mode])
        res[mode] = {"ms_per_frame": out[mode], "median_ms_per_frame": round((v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, 4),
                     "min_ms_per_frame": v[0], "max_ms_per_frame": v[-1]}
    return res


def main():
    args = sys.argv[1:]
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "bloom_time.json")
    frames = int(args[1]) if len(args) > 1 else 300
    repeats = int(args[2]) if len(args) > 2 else 4
    pkg = load_package()
    scene = pkg.scenes.terrain(width=W, height_px=H)
    result = {"what": "tools/bloom_time.py: bloom at 1920 x 1080 on one MI355X, terrain_1002k, 1 spp per frame",
              "frames": frames, "repeats": repeats, "slots_in_flight": SLOTS,
              "kernel": kernel_times(pkg, scene, frames), "present": present_loops(pkg, scene, frames, repeats)}
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["kernel"]["tail"]))
    print(json.dumps(result["present"]))


if __name__ == "__main__":
    main()
