"""Time the JPEG encoder (include/rfwhip.h, rfwhip_read_display_jpeg; csrc/display_jpeg.h) on one device at 1920 x 1080, on the
terrain (BASELINE config 3's scene) rendered at 1 spp per frame.  Two measurements, written as one JSON file:
  kernel   every kernel of family 14 with hipEvents (stage_timing=1; the read-only setting display_jpeg_time) and the stream's bytes
           at quality 90 / "420", 90 / "444" and 100 / "444" on the rendered frame, `frames` streams per variant, the variants in
           alternating blocks, `blocks` times each
  present  wall time per frame of the pipelined present loop of a group of one device — render(k), present into slot k % 2, wait
           for slot (k + 1) % 2: two frames in flight — with the display pair (rfwhip_group_present_display_async / _wait, RGBA8:
           4 B per pixel over PCIe) and with the JPEG pair (rfwhip_group_present_jpeg_async / _wait: the record, then the stream's
           bytes).  The two loops ALTERNATE, `repeats` times each, in one process: the RGBA8 loop of this run is the yardstick and
           the spread of a loop's repeats the margin.
Usage: python tools/jpeg_time.py [out=profiles/jpeg_time.json] [frames=200] [repeats=4]"""
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
VARIANTS = ((90, "420"), (90, "444"), (100, "444"))
KERNELS = ("k_jpeg_blocks", "k_jpeg_entropy", "k_jpeg_offsets", "k_jpeg_pack")


def _configure(c, quality, sub):
    c.set_setting("display_jpeg_quality", quality)
    c.set_setting("display_jpeg_subsampling", sub)


def kernel_times(pkg, scene, frames, blocks):
    ctx = pkg.RenderContext(device=0)
    ctx.init(W, H)
    scene.upload(ctx)
    for k, v in dict(integrator="pt", spp=1, stage_timing=1).items():
        ctx.set_setting(k, v)
    ctx.render_frame(scene.camera, pkg.RESET)
    frame = ctx.display("rgba8")
    rows = {v: {"quality": v[0], "subsampling": v[1], "us": {k: [] for k in KERNELS}} for v in VARIANTS}
    for b in range(blocks + 1):  # (block 0 warms up)
        for v in VARIANTS:
            _configure(ctx, *v)
            ctx.get_kernel_time("jpeg", reset=True)
            for _ in range(frames if b else 5):
                stream = ctx.jpeg_image(frame)
            ctx.wait()  # (resolves the timed spans)
            f = ctx.get_setting("display_jpeg_time").split()
            if b:
                for i, k in enumerate(KERNELS):
                    rows[v]["us"][k].append(round(float(f[i]) * 1e3 / max(int(f[4 + i]), 1), 2))
            rows[v]["stream_bytes"] = len(stream)
            rows[v]["stuffed_bytes"] = ctx.jpeg_record()["stuffed_bytes"]
    out = []
    for v in VARIANTS:
        r = rows[v]
        r["us_median_sum"] = round(sum(sorted(x)[len(x) // 2] for x in r["us"].values()), 2)
        out.append(r)
        print(json.dumps(r), flush=True)
    ctx.destroy()
    return out


def present_loops(pkg, scene, frames, repeats):
    g = pkg.render_group([0], "peer")
    g.init(W, H)
    scene.upload(g)
    for k, v in dict(integrator="pt", spp=1).items():
        g.set_setting(k, v)
    cap = g.jpeg_bound()
    streams = []

    def loop(jpeg, n):
        post = g.present_jpeg_async if jpeg else (lambda s: g.present_display_async(s, "rgba8"))
        wait = (lambda s: g.present_jpeg_wait(s, cap)) if jpeg else g.present_display_wait
        for k in range(n):
            g.render_async(scene.camera, pkg.RESET)
            post(k % SLOTS)
            if k >= SLOTS - 1:
                got = wait((k + 1) % SLOTS)
                if jpeg:
                    streams.append(len(got))
        for k in range(n - SLOTS + 1, n):
            wait(k % SLOTS)
        g.wait()

    out = {"rgba8": [], "jpeg": []}
    for r in range(repeats):
        for name, jpeg in (("rgba8", False), ("jpeg", True)):
            loop(jpeg, 20)  # (warm up: also re-labels the slots for this kind)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(jpeg, frames)
            torch.cuda.synchronize()
            out[name].append(round((time.perf_counter() - t0) * 1e3 / frames, 4))
            print(json.dumps({"loop": name, "repeat": r, "ms_per_frame": out[name][-1]}), flush=True)
    g.destroy()
    res = {}
    for name in ("rgba8", "jpeg"):
        v = sorted(out[name])
        res[name] = {"ms_per_frame": out[name], "median_ms_per_frame": round((v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, 4),
                     "min_ms_per_frame": v[0], "max_ms_per_frame": v[-1],
                     "copy_bytes_per_frame": W * H * 4 if name == "rgba8" else 32 + sorted(streams)[len(streams) // 2]}
    return res


def main():
    args = sys.argv[1:]
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "jpeg_time.json")
    frames = int(args[1]) if len(args) > 1 else 200
    repeats = int(args[2]) if len(args) > 2 else 4
    pkg = load_package()
    scene = pkg.scenes.terrain(width=W, height_px=H)
    result = {"what": "tools/jpeg_time.py: the JPEG encoder at 1920 x 1080 on one MI355X, terrain_1002k, 1 spp per frame",
              "frames": frames, "repeats": repeats, "slots_in_flight": SLOTS,
              "not_measured": "not measured here: groups of more than one device (one MI355X per run: the loop is a group of one), a stream's way through a network or into a viewer, settings other than the three variants, Ri other than 8",
              "kernel": kernel_times(pkg, scene, frames, repeats), "present": present_loops(pkg, scene, frames, repeats)}
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["present"]))


if __name__ == "__main__":
    main()
