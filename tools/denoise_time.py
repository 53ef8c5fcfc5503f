"""Time the denoiser (setting "denoise", csrc/denoise.h) on the 1920 x 1080 terrain (BASELINE config 3's scene), 1 spp per frame,
with hipEvents (stage_timing=1, kernel family 6).  One JSON line per variant:
  filter   a still camera: the guides are computed once, every present runs demodulation + the a-trous passes
  guides   the camera moves a little every frame: every present runs the guide pass too
  frame    wall time of a 1-spp frame (render + wait + present into device memory) with denoise off and on
With --temporal ("denoise_temporal" = 1) instead:
  temporal the camera pans every frame, RESET every frame: every present runs the guide pass, the demodulation, the temporal
           stage and the a-trous passes; TEMPORAL_BYTES is the stage's estimated traffic per pixel (the kernel's own time:
           a rocprofv3 --kernel-trace --stats run of this tool, k_dn_temporal)
  frame    wall time of such a frame with denoise off and with denoise + denoise_temporal on
With --motion ("denoise_temporal" = 1, "denoise_motion" = 0 then 1) the scene is BASELINE config 5's: the skinned CesiumMan of
tests/golden/asset_cesiumman.npz over a floor, 1920 x 1080, posed on the device before every frame (the fixture's three poses in
turn), RESET every frame, a still camera:
  motion   per setting: the denoiser's time per frame (guide pass with / without the surface record, demodulation, the stage's
           kernel k_dn_temporal / k_dn_temporal_motion, the passes) and the pose + refit kernels' time per frame (kernel times of
           their own: a rocprofv3 --kernel-trace --stats run of this tool)
  frame    wall time of such a frame (pose, update, render, present) per setting; with "1" it includes the snapshot copy in front
           of each pose (a device-to-device copy of 16 B per vertex outside the timed spans)
Usage: python tools/denoise_time.py [--temporal | --motion] [frames=200] [iterations=5]"""
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
# bytes a pass names per pixel: 25 taps x (irradiance 16 + variance 4 + guide 16) + 9 variance taps + centre albedo 16 + input 16,
# written: irradiance 16 + variance 4 (the last pass: the image, 16).  Unique per pass: the five planes once.
TAP_BYTES = 25 * 36 + 9 * 4 + 16 + 16 + 20
UNIQUE_BYTES = 16 + 4 + 16 + 16 + 16 + 20
# bytes the temporal stage names per pixel: the demodulation's I 16, guide 16, id 4, and per bilinear tap P's guide 16 + id 4 + colour
# 16 + moments 8 + length 4; written: I~ 16, var 4, moments 8, length 4, and pass 0's colour history 16
TEMPORAL_BYTES = 16 + 16 + 4 + 4 * (16 + 4 + 16 + 8 + 4) + 16 + 4 + 8 + 4 + 16


def temporal(pkg, ctx, scene, out, frames):
    ctx.set_setting("denoise_temporal", 1)
    base = scene.camera.position

    def run(n):
        for f in range(n):
            scene.camera.position = (base[0] + 0.05 * (f % 40), base[1], base[2])  # a slow pan, RESET every frame
            ctx.render_frame(scene.camera, pkg.RESET)
            ctx.read_framebuffer_device(out.data_ptr())
        ctx.wait()

    run(10)
    ctx.get_kernel_time("denoise", reset=True)
    run(frames)
    ms, launches = ctx.get_kernel_time("denoise", reset=True)
    print(json.dumps({"variant": "temporal", "frames": frames, "launches": launches, "denoise_ms_per_frame": round(ms / frames, 4),
                      "temporal_bytes_per_pixel_est": TEMPORAL_BYTES, "temporal_bytes_est": PIXELS * TEMPORAL_BYTES}), flush=True)
    ctx.set_setting("stage_timing", 0)
    for dn in (0, 1):
        ctx.set_setting("denoise", dn)
        run(10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(frames)
        torch.cuda.synchronize()
        print(json.dumps({"variant": "frame", "denoise": dn, "denoise_temporal": dn, "frames": frames,
                          "ms_per_frame": round((time.perf_counter() - t0) * 1e3 / frames, 4)}), flush=True)


def rig_scene(pkg, fx):
    """The fixture's mesh under its node transform on a floor, lit by a point light, an area light and a sky."""
    import numpy as np
    pos, t = fx["positions"], np.asarray(fx["node_transform"], np.float64)
    s = pkg.scenes.Scene()
    s.name = "cesiumman"
    body = s.add_material(color=(0.75, 0.55, 0.35), roughness=0.6)
    floor = s.add_material(color=(0.6, 0.6, 0.6), roughness=0.9)
    s.add_instance(s.add_mesh(pos, fx["indices"], normals=fx["normals"], material=body), t)
    lo = (t[:3, :3] @ pos.T.astype(np.float64)).T + t[:3, 3]
    c, r = (lo.min(0) + lo.max(0)) / 2, float(np.linalg.norm(lo.max(0) - lo.min(0)))
    y0 = float(lo[:, 1].min()) - 0.02 * r
    fv = np.array([[c[0] - 2 * r, y0, c[2] - 2 * r], [c[0] + 2 * r, y0, c[2] - 2 * r], [c[0] + 2 * r, y0, c[2] + 2 * r],
                   [c[0] - 2 * r, y0, c[2] + 2 * r]], np.float32)
    s.add_instance(s.add_mesh(fv, np.array([[0, 2, 1], [0, 3, 2]], np.uint32), material=floor))
    s.add_point_light((c[0] + r, c[1] + 1.5 * r, c[2] - 1.2 * r), (40.0 * r * r, 38.0 * r * r, 35.0 * r * r))
    s.add_area_light_quad((0.0, -1.0, 0.0), (c[0], c[1] + 2.0 * r, c[2]), r, r, (10.0, 10.0, 10.0))
    s.set_test_sky(64, 32)
    cam = pkg.Camera(aperture=0.0, FOV=40.0)
    cam.look_at((c[0] + 0.3 * r, c[1] + 0.2 * r, c[2] - 2.2 * r), tuple(c))
    cam.resize(W, H)
    s.camera = cam
    return s


def motion(pkg, frames, iterations):
    import numpy as np
    fx = np.load(os.path.join(ROOT, "tests", "golden", "asset_cesiumman.npz"))
    scene = rig_scene(pkg, fx)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    poses = fx["joint_matrices"]
    for on in (0, 1):
        ctx = pkg.RenderContext(device=0)
        ctx.init(W, H)
        scene.upload(ctx)
        for k, v in dict(integrator="pt", spp=1, stage_timing=1, denoise=1, denoise_iterations=iterations, denoise_temporal=1,
                         denoise_motion=on).items():
            ctx.set_setting(k, v)
        ctx.set_mesh_skin(0, fx["joints"], fx["weights"], fx["normals"])

        def run(n):
            for f in range(n):
                ctx.pose_mesh(0, poses[f % len(poses)])
                ctx.update()
                ctx.render_frame(scene.camera, pkg.RESET)
                ctx.read_framebuffer_device(out.data_ptr())
            ctx.wait()

        run(10)
        ctx.get_kernel_time("denoise", reset=True), ctx.get_kernel_time("refit", reset=True)
        run(frames)
        ms, launches = ctx.get_kernel_time("denoise", reset=True)
        rms, _ = ctx.get_kernel_time("refit", reset=True)
        print(json.dumps({"variant": "motion", "denoise_motion": on, "frames": frames, "launches": launches,
                          "denoise_ms_per_frame": round(ms / frames, 4), "pose_refit_ms_per_frame": round(rms / frames, 4)}), flush=True)
        ctx.set_setting("stage_timing", 0)
        run(10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(frames)
        torch.cuda.synchronize()
        print(json.dumps({"variant": "frame", "denoise_motion": on, "frames": frames,
                          "ms_per_frame": round((time.perf_counter() - t0) * 1e3 / frames, 4)}), flush=True)
        ctx.destroy()


def main():
    args = [a for a in sys.argv[1:] if a not in ("--temporal", "--motion")]
    frames = int(args[0]) if len(args) > 0 else 200
    iterations = int(args[1]) if len(args) > 1 else 5
    pkg = load_package()
    if "--motion" in sys.argv[1:]:
        return motion(pkg, frames, iterations)
    scene = pkg.scenes.terrain(width=W, height_px=H)
    ctx = pkg.RenderContext(device=0)
    ctx.init(W, H)
    scene.upload(ctx)
    for k, v in dict(integrator="pt", spp=1, stage_timing=1, denoise=1, denoise_iterations=iterations).items():
        ctx.set_setting(k, v)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    if "--temporal" in sys.argv[1:]:
        return temporal(pkg, ctx, scene, out, frames)
    cam = scene.camera

    def run(n, moving):
        for f in range(n):
            if moving:  # a camera that differs by value every frame: the guides are stale at every present
                cam.clampValue = 10.0 + 1e-3 * (f % 2 + 1)
            ctx.render_frame(cam, pkg.RESET if moving else pkg.CONVERGE)
            ctx.read_framebuffer_device(out.data_ptr())
        ctx.wait()  # (the last present's spans are resolved by the next wait)

    results = {}
    for variant, moving in (("filter", False), ("guides", True)):
        run(10, moving)
        ctx.get_kernel_time("denoise", reset=True)
        run(frames, moving)
        ms, launches = ctx.get_kernel_time("denoise", reset=True)
        results[variant] = ms / frames
        line = {"variant": variant, "frames": frames, "iterations": iterations, "launches": launches,
                "denoise_ms_per_frame": round(ms / frames, 4)}
        if variant == "filter":
            line["ms_per_pass"] = round(ms / frames / (iterations + 1), 4)
            line["bytes_per_pass_taps"] = PIXELS * TAP_BYTES
            line["bytes_per_pass_unique"] = PIXELS * UNIQUE_BYTES
            line["tap_GBps"] = round(PIXELS * TAP_BYTES / (ms / frames / (iterations + 1)) / 1e6, 1)
        else:
            line["guide_pass_ms"] = round(ms / frames - results["filter"], 4)
        print(json.dumps(line), flush=True)
    ctx.set_setting("stage_timing", 0)
    for dn in (0, 1):
        ctx.set_setting("denoise", dn)
        run(10, False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(frames, False)
        torch.cuda.synchronize()
        print(json.dumps({"variant": "frame", "denoise": dn, "frames": frames,
                          "ms_per_frame": round((time.perf_counter() - t0) * 1e3 / frames, 4)}), flush=True)


if __name__ == "__main__":
    main()
