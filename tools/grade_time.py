"""Time the graded display kernel (include/rfwhip.h, rfwhip_set_display_lut; csrc/display_grade.h) on one device at 1920 x 1080,
FXAA on, both formats, in one process.  With hipEvents (stage_timing=1), through rfwhip_display_stream on the rendered terrain frame in
device memory under a manual exposure of one stop (so that the parent's kernel is k_display_exposed):
  baseline   display_grade = 0: k_display_exposed, the parent's code (family 7)
  defaults   display_grade = 1, every parameter at its default: k_display_graded with every step skipped (family 13)
  wb_cdl     white balance, slope / offset / power and saturation
  lut33      wb_cdl and a 33^3 LUT
  dither     wb_cdl, the LUT and the dither (RGBA8 alone is affected)
in ALTERNATING blocks — baseline, defaults, wb_cdl, lut33, dither, `blocks` times over, `frames` launches per block.  The yardstick
for a difference is the baseline's own max - min over its blocks.
Usage: python tools/grade_time.py [out=profiles/grade_time.json] [frames=200] [blocks=5]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: torch's HIP runtime before librfwhip.so)

from __graft_entry__ import load_package  # noqa: E402

W, H = 1920, 1080
WB_CDL = {"display_wb_temperature": 5200, "display_grade_slope": "1.1 0.95 1.05", "display_grade_offset": "0.01 0 -0.02",
          "display_grade_power": "0.95 1 1.08", "display_grade_saturation": 0.8}
IDENTITY = {"display_wb_temperature": 6500, "display_grade_slope": 1, "display_grade_offset": 0, "display_grade_power": 1,
            "display_grade_saturation": 1}
CONFIGS = ("baseline", "defaults", "wb_cdl", "lut33", "dither")


def look(n):
    g = np.linspace(0.0, 1.0, n)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    s = lambda x: x * x * (3.0 - 2.0 * x)
    return np.stack([0.6 * s(r) + 0.4 * r, 0.5 * s(gg) + 0.5 * gg, 0.7 * s(b) + 0.3 * b], -1).astype(np.float32)


def configure(ctx, name):
    ctx.set_setting("display_grade", 0 if name == "baseline" else 1)
    for k, v in (IDENTITY if name in ("baseline", "defaults") else WB_CDL).items():
        ctx.set_setting(k, v)
    ctx.set_display_lut(look(33) if name in ("lut33", "dither") else None)
    ctx.set_setting("display_dither", 1 if name == "dither" else 0)


def main():
    args = sys.argv[1:]
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "grade_time.json")
    frames = int(args[1]) if len(args) > 1 else 200
    blocks = int(args[2]) if len(args) > 2 else 5
    pkg = load_package()
    scene = pkg.scenes.terrain(width=W, height_px=H)
    ctx = pkg.RenderContext(device=0)
    ctx.init(W, H)
    scene.upload(ctx)
    for k, v in dict(integrator="pt", spp=1, stage_timing=1, display_fxaa=1, display_exposure="manual", display_exposure_ev=1).items():
        ctx.set_setting(k, v)
    ctx.render_frame(scene.camera, pkg.RESET)
    rendered = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    ctx.read_framebuffer_device(rendered.data_ptr())
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    side = torch.cuda.Stream(device="cuda:0")  # (a stream of the caller's, not the null stream: the hipEvents ride it)
    torch.cuda.synchronize()

    def timed(fmt, family, n):
        def run(k):
            for _ in range(k):
                ctx.display_stream(rendered.data_ptr(), out.data_ptr(), fmt, side.cuda_stream)
            side.synchronize()
            ctx.wait()  # (resolves the timed spans)
        run(10)
        ctx.get_kernel_time(family, reset=True)
        run(n)
        ms, launches = ctx.get_kernel_time(family, reset=True)
        assert launches == n, (family, launches, n)
        return round(ms * 1e3 / n, 3)

    rows = []
    for fmt in ("rgba8", "rgba32f"):
        us = {name: [] for name in CONFIGS}
        for _ in range(blocks):
            for name in CONFIGS:
                configure(ctx, name)
                us[name].append(timed(fmt, "display" if name == "baseline" else "grade", frames))
        base = sorted(us["baseline"])
        row = {"format": fmt, "fxaa": 1, "baseline_spread_us": round(base[-1] - base[0], 3)}
        for name in CONFIGS:
            v = sorted(us[name])
            row[name] = {"us": us[name], "median_us": v[len(v) // 2], "minus_baseline_us": round(v[len(v) // 2] - base[len(base) // 2], 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.destroy()
    result = {"what": "tools/grade_time.py: k_display_exposed<true> (the parent's code) against k_display_graded<true> at 1920 x 1080 on one "
                      "MI355X, terrain_1002k, hipEvents, alternating blocks in one process",
              "frames_per_block": frames, "blocks": blocks, "rows": rows}
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
