"""Time the shade stage with the setting material_maps (csrc/rt_core.h: pt_maps_alpha / pt_maps_params) on the
textured atrium (scenes.atrium, BASELINE config 4) at 1920 x 1080, max_depth 2, on one device.  One JSON line per state:
  off        the setting off: k_shade_pt<true>
  on_nomaps  the setting on, the scene as it is — no material has such a map, so the same kernel runs (material_maps_on = 0)
  on_maps    the setting on, a metallic-roughness map on the materials of the room (floor, walls, gallery) and an alpha mask on the
             columns': k_shade_pt_maps
  off_maps   that scene with the setting off (the maps travel to the device and are ignored): what the maps' scene costs without them
shade_ms is the shade stage's kernels per frame (hipEvents: stage_timing=1, kernel family "shade"): the median of `frames` frames
behind `warmup` frames; frame_ms the median wall time of a frame in a run of its own without stage_timing.  No time here is a pass
criterion, and no ratio is asserted.
Usage: python tools/material_maps_time.py [--frames 9] [--warmup 3] [--spp 8] [--size 1920x1080]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: torch's HIP runtime before librfwhip.so)
import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def add_maps(pkg, scene, size=256):
    """The room's materials (scenes.atrium: 8..21) get one metallic-roughness texture, the columns' (2..5) a mask with holes."""
    rng = np.random.default_rng(25)
    mr = rng.integers(0, 256, (size, size, 4), dtype=np.uint8)
    mr[..., 3] = 255
    t_mr = scene.add_texture(pkg.scenes.make_texture_rgba8(mr))
    cells = np.kron(rng.random((16, 16)) < 0.75, np.ones((size // 16, size // 16))).astype(np.uint8) * 255
    t_mask = scene.add_texture(pkg.scenes.make_texture_rgba8(np.repeat(cells[..., None], 4, -1)))
    for m in scene.host_materials[8:22]:
        m.update(roughnessmap=t_mr, metallicmap=t_mr)
    for m in scene.host_materials[2:6]:
        m.update(alphamap=t_mask)


def measure(pkg, scene, w, h, spp, setting, frames, warmup):
    ctx = pkg.RenderContext(device=0)
    ctx.init(w, h)
    scene.upload(ctx)
    for k, v in {"integrator": "pt", "spp": spp, "max_depth": 2, "material_maps": setting}.items():
        ctx.set_setting(k, v)
    wall = []
    for k in range(warmup + frames):
        t0 = time.perf_counter()
        ctx.render_frame(scene.camera, pkg.RESET)
        wall.append(time.perf_counter() - t0)
    ctx.set_setting("stage_timing", 1)
    shade, launches = [], 0
    for k in range(warmup + frames):
        ctx.get_kernel_time("shade", reset=True)
        ctx.render_frame(scene.camera, pkg.RESET)
        ms, launches = ctx.get_kernel_time("shade", reset=True)
        shade.append(ms)
    st = ctx.get_stats()
    out = {"material_maps": setting, "material_maps_on": int(ctx.get_setting("material_maps_on")), "textured": int(ctx.get_setting("textured")),
           "shade_ms": round(float(np.median(shade[warmup:])), 3), "shade_ms_min": round(float(np.min(shade[warmup:])), 3),
           "shade_ms_max": round(float(np.max(shade[warmup:])), 3), "shade_launches": int(launches),
           "frame_ms": round(float(np.median(wall[warmup:])) * 1e3, 3),
           "rays": {"primary": int(st.primaryCount), "secondary": int(st.secondaryCount), "deep": int(st.deepCount), "shadow": int(st.shadowCount)}}
    ctx.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--size", default="1920x1080")
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.split("x"))
    pkg = load_package()
    plain, mapped = pkg.scenes.atrium(w, h), pkg.scenes.atrium(w, h)
    add_maps(pkg, mapped)
    head = {"tool": "tools/material_maps_time.py", "device": torch.cuda.get_device_name(0), "scene": plain.name, "size": [w, h], "spp": a.spp,
            "max_depth": 2, "frames": a.frames, "warmup": a.warmup, "stage_timing": 1}
    print(json.dumps(head), flush=True)
    for state, scene, setting in (("off", plain, 0), ("on_nomaps", plain, 1), ("on_maps", mapped, 1), ("off_maps", mapped, 0),
                                  ("off", plain, 0), ("on_maps", mapped, 1)):  # (off and on_maps once more: the run-to-run spread)
        print(json.dumps(dict(state=state, **measure(pkg, scene, w, h, a.spp, setting, a.frames, a.warmup))), flush=True)


if __name__ == "__main__":
    main()
