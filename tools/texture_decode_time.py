"""Time the image-texture decoder (include/rfwhip.h, rfwhip_set_texture_sources; csrc/texture_decode.h) on one device.  For 1024 x 1024
and 2048 x 2048 synthetic images at 4:4:4 and 4:2:0, with Ri in {8, 128, none}, on both entropy paths (texture_entropy = device | host):
  wall_ms   rfwhip_set_texture_sources of the one texture, end to end on the host's clock: the walk, the uploads, the kernels (and on
            the host path the serial entropy decoding), the mip chain, the wait for the record
  kernel_us every kernel of family 15 by hipEvents (stage_timing = 1; the read-only setting texture_decode_time) and its share of the
            kernels' sum
The streams come from the device's own encoder (rfwhip_jpeg_image, quality 90); "none" is the stream encoded with Ri = 65535 — one
interval where the image has at most 65535 MCUs — with its DRI segment cut out.  No time here is a pass criterion and no ceiling is
claimed: the parent commit has no decoder to compare with.  The file records what was measured and on what.
Usage: python tools/texture_decode_time.py [out=profiles/texture_decode_time.json] [repeats=5]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first: torch's HIP runtime before librfwhip.so)

from __graft_entry__ import load_package  # noqa: E402

KERNELS = ("k_texdec_zero", "k_texdec_entropy", "k_texdec_idct", "k_texdec_color", "k_tex_mips", "k_texdec_finish")


def without_dri(stream):
    i = stream.index(b"\xff\xdd")
    return stream[:i] + stream[i + 6:]


def main():
    import jpeg_model as jm
    args = sys.argv[1:]
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "texture_decode_time.json")
    repeats = int(args[1]) if len(args) > 1 else 5
    pkg = load_package()
    rows, skipped = [], []
    for size in (1024, 2048):
        img = jm.smooth(size, size)
        enc = pkg.RenderContext(device=0)
        enc.init(size, size)
        enc.set_setting("display_jpeg_quality", 90)
        for sub in ("444", "420"):
            enc.set_setting("display_jpeg_subsampling", sub)
            mcus = (size // (16 if sub == "420" else 8)) ** 2
            for ri in (8, 128, None):
                if ri is None and mcus > 65535:
                    skipped.append("%d x %d %s without DRI: %d MCUs are more than one interval of the encoder" % (size, size, sub, mcus))
                    continue
                enc.set_setting("display_jpeg_restart", ri or 65535)
                stream = enc.jpeg_image(img)
                if ri is None:
                    stream = without_dri(stream)
                for mode in ("device", "host"):
                    c = pkg.RenderContext(device=0)
                    c.set_setting("texture_entropy", mode)
                    c.set_setting("stage_timing", 1)
                    c.init(8, 8)
                    src = [{"kind": "jpeg", "data": stream, "flags": 0}]
                    wall, us = [], {k: [] for k in KERNELS}
                    for r in range(repeats + 1):  # (round 0 warms up: allocations)
                        c.get_kernel_time("texture_decode", reset=True)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        c.set_textures(src)
                        dt = (time.perf_counter() - t0) * 1e3
                        c.wait()  # (resolves the timed spans)
                        f = c.get_setting("texture_decode_time").split()
                        if r:
                            wall.append(round(dt, 3))
                            for i, k in enumerate(KERNELS):
                                us[k].append(round(float(f[i]) * 1e3, 2) if int(f[6 + i]) else None)
                    rec = c.texture_record(0)
                    med = {k: sorted(v)[len(v) // 2] for k, v in us.items() if v[0] is not None}
                    total = sum(med.values())
                    row = {"size": size, "subsampling": sub, "ri": ri, "texture_entropy": mode, "stream_bytes": len(stream),
                           "intervals": rec["intervals"], "blocks": rec["blocks"], "wall_ms": wall, "wall_ms_median": sorted(wall)[len(wall) // 2],
                           "kernel_us_median": med, "kernel_share": {k: round(v / total, 3) for k, v in med.items()},
                           "kernels_us_sum": round(total, 2)}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    c.destroy()
        enc.destroy()
    result = {"what": "tools/texture_decode_time.py: rfwhip_set_texture_sources of one JPEG texture on one MI355X (decode + five-level mip chain)",
              "device": torch.cuda.get_device_name(0), "repeats": repeats, "quality": 90, "image": "jpeg_model.smooth",
              "not_measured": skipped + ["photographic images", "several textures in one call", "4:2:2 and grey streams", "PNG sources"],
              "rows": rows}
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
