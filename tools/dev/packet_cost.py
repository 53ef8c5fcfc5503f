"""CPU probe (host emulation built with -DRT_DEV_PACKET_COST): what the packet form of the pt primary wave WALKS — wave-level node
steps and leaf triangle tests — with the per-wave sort, with the camera-ordered node table (RFWHIP_PRIMARY_ORDER=1), with the
ordered table plus one comparator (RT_DEV_ORDER_PLANB=1), and with the ordered table plus the entry snapshot (setting primary_entry,
records of 8 and of 16 words: the latter is a build of its own, -DRT_PRIMARY_ENTRY_K=16).  The bench camera on the terrain at reduced resolution, 64 spp so that a
wave is one pixel.  usage: packet_cost.py [grid] [width] [height]        (each variant runs in a child process: the environment
variable is read when the context is created, and the counters are printed by the library on stderr)"""
import os
import re
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))


def child(grid, w, h, entry, k):
    import ctypes
    import build_emu
    from __graft_entry__ import load_package
    pkg = load_package()
    lib = ctypes.CDLL(build_emu.build(defines=("-DRT_DEV_PACKET_COST", "-DRT_PRIMARY_ENTRY_K=%d" % k), tag="_cost%d" % k))
    ctx = pkg._binding.CoreBinding(lib, "rfwhip_", 0, 0, 1)
    scene = pkg.scenes.terrain(n=grid, width=w, height_px=h)
    ctx.init(w, h)
    scene.upload(ctx)
    for k, v in (("integrator", "pt"), ("spp", 64), ("max_depth", 0), ("refill", 15), ("primary_entry", entry)):
        ctx.set_setting(k, v)
    ctx.render_frame(scene.camera, pkg.RESET)
    print("passes", ctx.get_kernel_time("primary_order")[1], "entry", ctx.get_setting("primary_entry_on"), "image sum %.9g" % float(ctx.framebuffer().astype("float64").sum()))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*[int(a) for a in sys.argv[2:7]])
        sys.exit(0)
    grid, w, h = [int(a) for a in (sys.argv[1:4] + ["708", "240", "135"][len(sys.argv) - 1:])]
    base = None
    for name, env, entry, k in (("sorted per wave", {"RFWHIP_PRIMARY_ORDER": "0"}, 0, 8), ("camera order", {"RFWHIP_PRIMARY_ORDER": "1"}, 0, 8),
                                ("camera order + 1 comparator", {"RFWHIP_PRIMARY_ORDER": "1", "RT_DEV_ORDER_PLANB": "1"}, 0, 8),
                                ("camera order + snapshot K=8", {"RFWHIP_PRIMARY_ORDER": "1"}, 1, 8),
                                ("camera order + snapshot K=16", {"RFWHIP_PRIMARY_ORDER": "1"}, 1, 16)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(grid), str(w), str(h), str(entry), str(k)], env=dict(os.environ, **env),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-2000:])
        m = re.search(r"packet_cost ordered=(\d) node_steps=(\d+) leaf_tris=(\d+)", r.stderr)
        nodes, tris = int(m.group(2)), int(m.group(3))
        base = base or (nodes, tris)
        print("%-28s node steps %10d (x %.4f)  leaf triangle tests %10d (x %.4f)  %s" % (
            name, nodes, nodes / base[0], tris, tris / base[1], r.stdout.strip()), flush=True)
