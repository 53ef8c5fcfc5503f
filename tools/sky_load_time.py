"""Time the sky's loaders (include/rfwhip.h, rfwhip_set_sky_hdr and sky_table; csrc/sky_load.h) on one device.  For a synthetic sky
(a gradient, a sun, a dark ground: runs in the exponent plane, literals in the mantissas) of 512 x 256, 2048 x 1024 and 5120 x 2560
texels — the last is the size of the reference's own test sky — from the same run:
  kernel_us        every kernel of family 17 by hipEvents (stage_timing = 1; the read-only setting sky_load_time), warm, the median
                   of `repeats` builds
  decode_wall_ms   rfwhip_set_sky_hdr end to end on the host's clock: the walk, the uploads, the two kernels, the wait
  table_wall_ms    the rebuild of the alias table after a new sky (update_sky_sampling, entered through rfwhip_read_sky_table) with
                   sky_table = device and with sky_table = host — the host path is the parent commit's code and the baseline
  model_decode_ms  the numpy model's decode of the same file on the host (tests/sky_load_model.py), once
Every size runs in a child process of its own under a time limit of its own; a child that fails or runs out of time ends the run
there.  No time here is a pass criterion.  The file records what was measured and on what.
Usage: python tools/sky_load_time.py [out=profiles/sky_load_time.json] [repeats=5]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("k_skyhdr_planes", "k_skyhdr_texels", "k_skytab_weights", "k_skytab_total", "k_skytab_scan_block", "k_skytab_scan_super",
           "k_skytab_scan_top", "k_skytab_scan_apply", "k_skytab_assign")
SIZES = ((512, 256, 120), (2048, 1024, 180), (5120, 2560, 420))  # width, height, the child's time limit in seconds


def synthetic_sky(w, h):
    import numpy as np
    y, x = np.mgrid[0:h, 0:w]
    up = np.clip(1.0 - y / (h * 0.5), 0.0, 1.0)[..., None]
    rgb = np.where(y[..., None] < h // 2, up * np.array([0.2, 0.4, 1.0]) + (1 - up) * np.array([0.9, 0.9, 1.0]), 0.05 * np.ones(3))
    sun = np.exp(-(((x - w * 0.3) / (w * 0.004)) ** 2 + ((y - h * 0.2) / (h * 0.008)) ** 2))[..., None]
    noise = np.random.default_rng(1).random((h, w, 1)) * 0.02
    return (rgb + 2000.0 * sun * np.array([1.0, 0.9, 0.7]) + noise * (y[..., None] < h // 2)).astype(np.float32)


def encode_segments(rgbe, seg=64):
    """A vectorised RLE encoder for widths that are multiples of `seg`: a segment of equal bytes is a run, any other a literal."""
    import numpy as np
    h, w = rgbe.shape[:2]
    planes = np.ascontiguousarray(rgbe.transpose(0, 2, 1)).reshape(h, 4, w // seg, seg)
    equal = (planes == planes[..., :1]).all(-1)
    head = bytes((2, 2, w >> 8, w & 255))
    out = [b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w)]
    run, lit = bytes((128 + seg,)), bytes((seg,))
    for y in range(h):
        out.append(head)
        for c in range(4):
            row, eq = planes[y, c], equal[y, c]
            out.extend(run + row[k, :1].tobytes() if eq[k] else lit + row[k].tobytes() for k in range(w // seg))
    return b"".join(out)


def child(w, h, repeats):
    import numpy as np
    import torch  # (first: torch's HIP runtime before librfwhip.so)
    from __graft_entry__ import load_package
    import sky_load_model as sm
    pkg = load_package()
    rgbe = pkg.images.rgbe_from_float(synthetic_sky(w, h))
    data = encode_segments(rgbe)
    t0 = time.perf_counter()
    want = sm.decode(data)
    model_ms = (time.perf_counter() - t0) * 1e3
    scene = pkg.scenes.cornell(64, 48)
    c = pkg.RenderContext(device=0)
    c.init(64, 48)
    scene.upload(c)
    c.set_setting("stage_timing", 1)
    c.set_setting("sky_sampling", 1)
    src = np.frombuffer(data, np.uint8)
    set_hdr, read_table, n_entries, rec = c._fn("set_sky_hdr"), c._fn("read_sky_table"), pkg.abi.C.c_size_t(), pkg.abi.SkyTableRecord()
    decode_ms, table_ms, us, built = [], {"device": [], "host": []}, {k: [] for k in KERNELS}, {}
    for r in range(repeats + 1):  # (round 0 warms up: allocations, code objects)
        for mode in ("device", "host"):
            c.set_setting("sky_table", mode)
            c.get_kernel_time("sky_load", reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c._check(set_hdr(c._ctx, src.ctypes.data, src.size, 0))
            t1 = time.perf_counter()
            c._check(read_table(c._ctx, None, 0, pkg.abi.C.byref(n_entries), pkg.abi.C.byref(rec)))  # (a new sky: the table is rebuilt here)
            t2 = time.perf_counter()
            c.wait()  # (resolves the timed spans)
            f = c.get_setting("sky_load_time").split()
            if r:
                decode_ms.append(round((t1 - t0) * 1e3, 3))
                table_ms[mode].append(round((t2 - t1) * 1e3, 3))
                if mode == "device":
                    built = rec.as_dict()  # (the device's record: the host's path fills S alone)
                    for i, k in enumerate(KERNELS):
                        us[k].append(round(float(f[i]) * 1e3, 2))
    ok = bool(np.array_equal(c.read_sky().view(np.uint32), want.view(np.uint32)))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    row = {"width": w, "height": h, "texels": w * h, "file_bytes": len(data), "decode_equals_model": ok, "model_decode_ms": round(model_ms, 1),
           "decode_wall_ms": decode_ms, "decode_wall_ms_median": med(decode_ms),
           "table_wall_ms": table_ms, "table_wall_ms_median": {m: med(v) for m, v in table_ms.items()},
           "kernel_us_median": {k: med(v) for k, v in us.items()},
           "table_kernels_us_sum": round(sum(med(us[k]) for k in KERNELS[2:]), 2), "device_record": built,
           "device": torch.cuda.get_device_name(0)}
    c.destroy()
    print("ROW " + json.dumps(row), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(int(args[1]), int(args[2]), int(args[3]))
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "sky_load_time.json")
    repeats = int(args[1]) if len(args) > 1 else 5
    rows, stopped = [], None
    for w, h, limit in SIZES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(w), str(h), str(repeats)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            stopped = "%d x %d: no result within %d s" % (w, h, limit)
            break
        line = [l for l in r.stdout.splitlines() if l.startswith("ROW ")]
        if r.returncode != 0 or not line:
            stopped = "%d x %d: exit status %d: %s" % (w, h, r.returncode, r.stderr[-400:])
            break
        rows.append(json.loads(line[0][4:]))
        print(line[0][4:], flush=True)
    result = {"what": "tools/sky_load_time.py: a Radiance HDR sky decoded on the device and the alias table of sky_sampling rebuilt for it, "
                      "sky_table = device against sky_table = host (the parent's path), on one device",
              "device": rows[0]["device"] if rows else None, "repeats": repeats, "sky": "synthetic: gradient, sun, dark ground; RLE in segments of 64",
              "not_measured": ["photographic skies", "flat files", "groups of several devices"] + ([stopped] if stopped else []), "rows": rows}
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
