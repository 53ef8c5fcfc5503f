#!/usr/bin/env python3
"""bench.py — Msamples/s of the HIP wavefront rendercore on BASELINE.json's headline workload.

  python bench.py --gpus N --steps K --warmup W           (N > 1: launched by torch.distributed.run, one rank per GPU)
  python bench.py ... --dump-outputs DIR                  (also writes the image of the last timed step: DIR/framebuffer.npy)
  python bench.py ... --full                              (also everything below the headline: counters, roofline, CPU baselines)

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the result line; roofline, sampler_bluenoise,
cpu_baseline, cpu_baseline_parity, parity_vs_cpu_baseline and, for N > 1, ranks.gather_enqueue_to_done_ms are null in it.
--full measures and checks them as well, outside the timed region (a minute or more at the default size).

Workload (BASELINE.json configs[2]): synthetic ~1 M-triangle displaced grid (1 002 528 triangles, seed 0x5EED) +
synthetic HDR sky + 8 emissive light triangles + 2 point lights, 1920x1080, wavefront path-tracing integrator
(primary generate -> BVH traverse + Moller-Trumbore -> shade with next-event estimation -> compaction -> connect),
MAX_PATH_LENGTH 2 like the reference (settings.h:5).  One *step* = one frame of `--spp` samples per pixel enqueued as
one wavefront batch, plus — for N > 1 — the gather of the rank-local strips into the root's HBM and the de-interleave
there (rfwhip_comm_*: RCCL send / recv issued by the library itself; torch.distributed only carries the 128-byte
communicator id, the barriers and the max-over-ranks of the elapsed time).  Inputs (scene, BVH, path buffers) are
resident in HBM before the timed region starts.

The JSON line of a --full run carries, besides the driver contract fields:
  roofline      the kernel that dominates the default command by time — k_trace_fused: the bounce and shadow waves of a depth in
                one launch — in the units of what binds it (bound "valu": achieved = VALU wave-instructions per second of the launch,
                peak = 1024 SIMDs x 2.4 GHz / 2, frac = achieved / peak, lane_weighted_frac beside it; its bytes — algorithmic per
                SURVEY §8(d) from an instrumented replay, and HBM by the counters — under roofline.bytes; bound "hbm": algorithmic
                bytes per second against the 8 TB/s peak); launch durations from hipEvents on the launch's own stream, one sub-batch
                alone on the chip.  roofline.hbm_kernel: the shade kernel, the one stage whose time is bytes.  roofline.stages:
                primary / bounce / shadow / shade each alone on the chip with algorithmic bytes, counter bytes, VALU instructions and
                lanes per instruction.  The counters are THIS run's (--pmc auto: four `rocprofv3 --pmc` passes of a 2-step child run
                before the timed region; roofline.traffic_source says where they came from), else profiles/stage_counters.json when
                it carries the hash of the running sources.
  cpu_baseline  the CPU oracle's restatement of the same integrator ("port") on the host cores, bounded sample; the GPU
                image of the same sample indices is compared with the oracle's (parity_vs_cpu_baseline, with a pass rule).
  cpu_baseline_parity  the Embree rendercore's algorithm (EmbreeRT/src/Context.cpp:104-300: 1 primary + one shadow ray per
                light, the `parity` integrator) on the same scene: oracle on the host cores beside the GPU rate.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8 TB/s spec (6.29 TB/s measured copy peak)
L2_PEAK_GBS = 34500.0  # same guide, §L2: 8 XCDs x 4 MiB, ~34.5 TB/s aggregate
# a CU's vector L1 serves ONE divergent 16-byte lane-load per clock (profiles/micro/gather_micro.hip: 75 G 128-byte
# records/s with 8 loads each, whatever the table size)
LANE_LOADS_PEAK = 600.0e9
# VALU issue, per the guide (§CU: a wave64 instruction issues over 2 cycles on a SIMD-32): 256 CUs x 4 SIMDs x 2.4 GHz / 2.
# Compares, selects, conversions and min/max measure about half of that (profiles/micro/valu_micro.hip: 550-600 G/s,
# v_fma_f32 660-970), so a traversal kernel's mix cannot reach 1.0; the fraction is reported against the guide's figure.
VALU_ISSUE_PEAK = 1024 * 2.4e9 / 2
NODE_BYTES = 64.0  # rt::Node4c: four 16-byte rows (csrc/rt_types.h) — also SURVEY §8(d)'s "64 B per popped inner node"
NODE_ROWS = 4.0
def stage_kernels(ctx, sample_group):
    """The kernels a pt render call launches for each stage, from what the library says about its variants (read-only settings):
    the textured shade kernel when some material carries a map, the packet form of the primary wave when the scene's trees fit its
    stack and the samples of a pixel sit side by side (sample groups >= 2).  bounce / shadow: the kernels of the un-fused launches
    (fuse=0: the per-stage table and the counter passes); the default launches both bodies as ONE kernel per depth, `fused`."""
    textured = ctx.get_setting("textured") == "1"
    packet = ctx.get_setting("packet") == "1" and sample_group >= 2
    # round 6: the connection wave of the primary vertices in packet form (k_shadow_packet) where the library chose it
    shadow0 = "k_shadow_packet<false>" if (ctx.get_setting("shadow_packets_on") == "1" and sample_group >= 8) else None
    return {"primary": "k_primary_packet<false>" if packet else "k_extend<1, false>", "bounce": "k_trace_stream<false, false>",
            "shadow": "k_trace_stream<true, false>", "shadow0": shadow0, "shade": "k_shade_pt<true>" if textured else "k_shade_pt<false>",
            "fused": "k_trace_fused<false>"}


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def oracle_flags():
    """Compiler and flags of the cpu_baseline's library, from oracle/Makefile (no -march=native: the prebuilt .so travels to the GPU box)."""
    try:
        txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        cc = re.search(r"^CC\s*\?=\s*(\S+)", txt, re.M).group(1)
        fl = re.search(r"^CFLAGS\s*\?=\s*(.+)$", txt, re.M).group(1).strip()
        ver = subprocess.run([cc, "-dumpfullversion"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
        return "%s %s %s" % (cc, ver, fl)
    except Exception:
        return None


def usable_cores():
    """Host cores this process may really use: min(affinity mask, cgroup cpu.max quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def probe_embree():
    """is an Embree the CPU baseline could call discoverable on this box?  (ldconfig cache, the usual library
    directories, CMake package files.)  Returns a short description or None."""
    import ctypes.util
    import glob
    for name in ("embree3", "embree4", "embree"):
        found = ctypes.util.find_library(name)
        if found:
            return found
    for pat in ("/usr/lib*/**/libembree*.so*", "/usr/local/lib*/**/libembree*.so*", "/opt/**/libembree*.so*",
                "/usr/lib*/cmake/embree*", "/usr/local/lib*/cmake/embree*"):
        hit = glob.glob(pat, recursive=True)
        if hit:
            return hit[0]
    return None


def csrc_hash():
    """Identity of the sources a single-GPU measurement belongs to: sha1 over the files of rendering-fw_amd/csrc/ that make
    up the render path (kernels, device functions, data layout, host-side launch logic and BVH builders; sorted, names +
    contents — not the multi-GPU gather of rfwhip_group.cpp, which no single-GPU kernel passes through).
    profiles/stage_counters.json records it when tools/evidence.sh derives the file; figures taken on other sources are
    reported as null."""
    h = hashlib.sha1()
    d = os.path.join(ROOT, "rendering-fw_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".h", ".hip", ".cpp")) and f not in ("rfwhip_group.cpp", "internal.h"):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spp", type=int, default=256,
                    help="samples per pixel per step (one wavefront batch; config 3: >= 64 spp; 256 = four sub-batches of 64, so a "
                         "wave is one pixel x 64 samples, and the calls of an 8-GPU strip split stay large: path state = 140 GB of "
                         "the 288 GB per GPU at N = 1)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grid", type=int, default=708, help="terrain cells per side (708 -> 1 002 528 triangles)")
    ap.add_argument("--workload", default="terrain", choices=["terrain", "atrium"],
                    help="terrain = BASELINE config 3 (the contract workload); atrium = config 4 (263 k instanced, textured "
                         "triangles) under the same protocol, e.g. for its 8-GPU strip split")
    ap.add_argument("--integrator", default="pt", choices=["pt", "parity"])
    ap.add_argument("--max-depth", type=int, default=2)
    ap.add_argument("--refill", type=int, default=15, help="persistent-lane traversal: bit 0 bounce waves, bit 1 shadow waves, bit 2 primary wave, "
                                                             "bit 3 the primary wave in packet form (wave-uniform traversal)")
    ap.add_argument("--streams", type=int, default=4, help="concurrent sub-batches (HIP streams) per render call")
    ap.add_argument("--overlap", type=int, default=-1, help="connection waves on a second stream per sub-batch: 0 / 1 / -1 = by launch size")
    ap.add_argument("--lds-nodes", type=int, default=-1,
                    help="top-of-tree 4-wide nodes kept in LDS by the traversal kernels (-1: kernel capacity, 0: off)")
    ap.add_argument("--gather", default="comm", choices=["comm", "torch"],
                    help="N > 1: comm = rfwhip_comm_* (host C++ -> RCCL send / recv below the C ABI, the default — a failure to set it "
                         "up is an ERROR, never a silent change of path); torch = torch.distributed.gather of the local strips + "
                         "rfwhip_deinterleave_stream, only when asked for (the round-2 path)")
    ap.add_argument("--mode", default="ranks", choices=["ranks", "group"],
                    help="N > 1: ranks = one process per GPU under torch.distributed.run (the driver's launch); group = ONE process, one "
                         "host thread, rfwhip_group_* over --gpus devices — the plugin's host model (RFW/system/src/rfw/app.cpp:3-26); "
                         "run it as plain `python bench.py --gpus N --mode group`")
    ap.add_argument("--transport", default="auto", choices=["auto", "rccl", "peer"], help="--mode group: transport of the gather")
    ap.add_argument("--pipeline", type=int, default=1,
                    help="N > 1, --gather torch: 1 = stream-ordered present/gather/de-interleave overlapping the next step's "
                         "kernels; 0 = host-synchronous gather per step (reports gather_ms_per_step)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check what the headline does not need: the counter passes (--pmc), "
                         "the roofline and its per-stage table, the blue-noise sampler, the CPU baselines and the GPU image against "
                         "the CPU oracle's, and for N > 1 the gather of a finished frame alone.  Off: the run sets up, warms up, "
                         "times the steps, writes --dump-outputs and prints the result line with those fields null")
    ap.add_argument("--stage-rates", action="store_true",
                    help="--full: also report Mrays/s per stage of the serialised frame, the way the reference's stats window shows them")
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VALUE",
                    help="extra rendercore setting(s) for A/B runs, e.g. --set sample_group=1 (recorded in config.settings)")
    ap.add_argument("--pmc", default="auto", choices=["auto", "on", "off"],
                    help="hardware counters of THIS run for the roofline: separate `rocprofv3 --pmc` passes (FETCH_SIZE; WRITE_SIZE; VALU "
                         "instructions / lanes; VALU instruction classes) of a short child run of this script.  auto: when rocprofv3 is on the "
                         "PATH (--full, N = 1, pt integrator, roofline on; RFWHIP_BENCH_PMC=0 switches it off); otherwise — and when a pass fails — the "
                         "committed profiles/stage_counters.json is used if it belongs to the running sources")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="target CPU time of the cpu_baseline sample")
    ap.add_argument("--stage-json", default=os.path.join(ROOT, "profiles", "stage_counters.json"),
                    help="PMC-derived per-kernel counters (tools/evidence.sh; see profiles/README.md)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step — the presented image a "
                         "caller reads back (height x width x 4 float32) — as DIR/framebuffer.npy; the inputs are seeded, so two "
                         "builds run with the same arguments can be compared output for output")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:
        # (asked for explicitly, they would otherwise be dropped without a word)
        if args.stage_rates:
            ap.error("--stage-rates is part of the roofline: add --full")
        if args.pmc == "on":
            ap.error("--pmc on takes counters for the roofline: add --full")
    return args


DUMP_BYTES_MAX = 64 * 10 ** 6


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as <out_dir>/<name>.npy.  The files stay under DUMP_BYTES_MAX in all: an array above its
    share is written as a fixed sample of its rows along the last axis (e.g. the pixels of an image), chosen by seed 0 and
    kept in their original order — the same rows for the same shape on every run — and <name>_rows.npy beside it holds the
    index of every sampled row in a.reshape(-1, a.shape[-1]) (float64, exact)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BYTES_MAX // len(arrays) - 2 * 4096  # (room for two .npy headers)
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        if a.nbytes > share:
            rows = a.reshape(-1, a.shape[-1])
            pick = np.sort(np.random.default_rng(0).choice(len(rows), share // (rows[0].nbytes + 8), replace=False))
            a = rows[pick]
            np.save(os.path.join(out_dir, name + "_rows.npy"), pick.astype(np.float64))
        np.save(os.path.join(out_dir, name + ".npy"), a)


def load_stage_counters(path, scene_name, spp, streams):
    """profiles/stage_counters.json if it belongs to this workload; `fresh` tells whether it was taken on the sources that
    are running now."""
    try:
        pm = json.load(open(path))
    except Exception:
        return None, False
    if pm.get("workload") != scene_name or pm.get("spp") != spp or pm.get("streams") != streams:
        return None, False
    return pm, pm.get("csrc_hash") == csrc_hash()


PMC_PASSES = (("fetch", ["FETCH_SIZE"]), ("write", ["WRITE_SIZE"]),
              ("lanes", ["SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_THREAD_CYCLES_VALU", "GRBM_GUI_ACTIVE"]),
              ("mix", ["SQ_INSTS_VALU_TRANS_F32", "SQ_INSTS_VALU_FMA_F32", "SQ_INSTS_VALU_MUL_F32", "SQ_INSTS_VALU_ADD_F32", "SQ_INSTS_SALU"]))


def collect_stage_counters(args, scene_name, timeout_s=240):
    """The counters behind roofline.stages / .traffic, taken BY THIS RUN (round 5's verdict: the line's counters were constants from
    a committed file): one `rocprofv3 --pmc` pass per counter group — FETCH_SIZE and WRITE_SIZE each on their own, as
    MI355X_MICROARCH.md prescribes; no trace flags — of a short child run of this script (2 steps, fuse=0 so that every stage is a
    kernel of its own), summarised per kernel by profiles/summarize.py into <out>/stage_counters.json.  Returns (dict, path) or
    (None, reason)."""
    import shutil
    rocprof = shutil.which("rocprofv3")
    if not rocprof:
        return None, "rocprofv3 not on the PATH"
    if any("rocprof" in os.environ.get(k, "").lower() for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB")):
        return None, "this process is itself being profiled (no counter passes nested under a profiler)"
    out_dir = os.path.join(ROOT, "gpurun_out", "bench_pmc")
    try:
        shutil.rmtree(out_dir, ignore_errors=True)
        os.makedirs(out_dir, exist_ok=True)
    except OSError as e:
        return None, "cannot write %s: %s" % (out_dir, e)
    child = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-roofline",
             "--pmc", "off", "--spp", str(args.spp), "--width", str(args.width), "--height", str(args.height), "--grid", str(args.grid),
             "--workload", args.workload, "--max-depth", str(args.max_depth), "--refill", str(args.refill), "--streams", str(args.streams),
             "--set", "fuse=0"]
    for kv in args.set:
        if not kv.startswith("fuse="):
            child += ["--set", kv]
    env = dict(os.environ, TMPDIR="/tmp", RFWHIP_BENCH_PMC="0")
    dbs = []
    for name, counters in PMC_PASSES:
        d = os.path.join(out_dir, name)
        cmd = [rocprof, "--pmc"] + counters + ["-d", d, "--"] + child
        try:
            # (its own process group: a pass that hangs is killed with everything it started)
            pr = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=open(d + ".log", "w"), stderr=subprocess.STDOUT, start_new_session=True)
            try:
                rc = pr.wait(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                import signal
                os.killpg(pr.pid, signal.SIGKILL)
                pr.wait()
                return None, "pass %s timed out after %d s" % (name, timeout_s)
        except OSError as e:
            return None, "pass %s: %s" % (name, e)
        found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith(".db")]
        if rc != 0 or not found:
            return None, "pass %s failed (rc %s, %d result files; %s.log)" % (name, rc, len(found), os.path.relpath(d, ROOT))
        dbs.append(found[0])
    try:
        import contextlib
        import importlib.util
        import io
        spec = importlib.util.spec_from_file_location("rfw_summarize", os.path.join(ROOT, "profiles", "summarize.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            mod.stages(args.spp, args.streams, scene_name, "bench.py --pmc (this run)", csrc_hash(), *dbs)
        pm = json.loads(buf.getvalue())
        path = os.path.join(out_dir, "stage_counters.json")
        json.dump(pm, open(path, "w"), indent=1)
        return pm, path
    except Exception as e:
        return None, "summarising the passes failed: %s" % str(e)[:200]


def main_group(args):
    """--mode group: one process, one host thread, rfwhip_group_* over args.gpus devices (render on every device, ONE gather per
    step issued by the library, nothing blocks the host in between) — the plugin's host model, measured under the bench protocol."""
    import torch
    from __graft_entry__ import load_package
    if int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--mode group is ONE process: run `python bench.py --gpus N --mode group` without torch.distributed.run")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the rendercore has no CPU path")
    one_device = os.environ.get("RFWHIP_BENCH_ONE_DEVICE") == "1"  # development aid: n contexts on GPU 0, peer transport
    n = args.gpus
    if not one_device and torch.cuda.device_count() < n:
        raise SystemExit("--gpus %d --mode group: only %d device(s) visible" % (n, torch.cuda.device_count()))
    pkg = load_package()
    scene = (pkg.scenes.atrium(args.width, args.height) if args.workload == "atrium" else
             pkg.scenes.terrain(n=args.grid, width=args.width, height_px=args.height))
    g = pkg.render_group([0] * n if one_device else list(range(n)), "peer" if one_device else args.transport)
    g.init(args.width, args.height)
    scene.upload(g)
    for k, v in (("integrator", args.integrator), ("spp", args.spp), ("max_depth", args.max_depth), ("refill", args.refill),
                 ("streams", args.streams), ("lds_nodes", args.lds_nodes), ("overlap", args.overlap)):
        g.set_setting(k, v)
    extra = {}
    for kv in args.set:
        k, _, v = kv.partition("=")
        g.set_setting(k, v)
        extra[k] = v
    if args.set:
        g.update()

    def step(first):
        g.render_async(scene.camera, pkg.RESET if first else pkg.CONVERGE)
        g.gather()
    for k in range(args.warmup):
        step(k == 0)
    g.wait()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k == 0)
    g.wait()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    img = g.framebuffer()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"framebuffer": img})
    out = {"metric": "Msamples/sec at 1920x1080, 1M-tri scene; 1/2/4/8-GPU tile scaling", "value": round(float(args.width) * args.height * args.spp * args.steps / elapsed / 1e6, 3),
           "unit": "Msamples/s", "n_gpus": n, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "full": bool(args.full),
           "config": {"workload": "%s: %d triangles, %dx%d, %s integrator depth %d, %d spp per step" % (scene.name, scene.triangle_count(), args.width, args.height, args.integrator, args.max_depth, args.spp),
                      "parallelism": "ONE process / one host thread drives %d contexts (rfwhip_group_*): image strips of 8 rows interleaved over the ranks, one gather per step into rank 0's HBM" % n,
                      "gather": "group:%s%s" % (g.transport, " (all contexts on device 0: development aid, the number means nothing)" if one_device else ""),
                      "spp_per_step": args.spp, "streams": args.streams, "settings": extra or None, "csrc_hash": csrc_hash()},
           "roofline": None, "cpu_baseline": None, "image_mean": float(img[..., :3].mean())}
    print(json.dumps(out))
    g.destroy()


def main():
    args = parse()
    if args.mode == "group":
        return main_group(args)
    import numpy as np
    import torch
    from __graft_entry__ import load_package

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    one_device = os.environ.get("RFWHIP_BENCH_ONE_DEVICE") == "1"
    if one_device:
        # development aid for a 1-GPU box: all ranks on GPU 0 and — RCCL refuses two ranks on one device — gloo with host
        # staging for the gather.  Walks through the N > 1 control flow only; its numbers mean nothing.
        local_rank = 0
        if os.environ.get("RFWHIP_BENCH_TRY_COMM") != "1":  # (RCCL refuses the duplicate device: exercises the loud fall-back)
            args.gather = "torch"
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus %d needs one process per GPU: launch with python -m torch.distributed.run "
                             "--nnodes=1 --nproc-per-node %d ... bench.py --gpus %d" % (args.gpus, args.gpus, args.gpus))
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the rendercore has no CPU path (the CPU oracle is only the baseline)")
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        if one_device:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    pkg = load_package()
    t0 = time.time()
    if args.workload == "atrium":
        scene = pkg.scenes.atrium(args.width, args.height)
    else:
        scene = pkg.scenes.terrain(n=args.grid, width=args.width, height_px=args.height)
    t_scene = time.time() - t0
    # ---- the run's own hardware counters, BEFORE this process takes the device's memory (a 256-spp step holds 140 GB of path state,
    # and every counter pass is a child process that renders the same workload)
    own_pm, own_source, own_note = None, None, "--pmc off"
    want_pmc = (args.full and not args.no_roofline and rank == 0 and args.integrator == "pt" and
                (args.pmc == "on" or (args.pmc == "auto" and world == 1 and os.environ.get("RFWHIP_BENCH_PMC", "1") != "0")))
    if want_pmc:
        t_pmc = time.time()
        own_pm, where = collect_stage_counters(args, scene.name)
        if own_pm:
            own_source = {"file": os.path.relpath(where, ROOT), "taken_by": "this run: one `rocprofv3 --pmc` pass per counter group of a 2-step child run (fuse=0), before the timed region",
                          "passes": [" ".join(c) for _, c in PMC_PASSES], "seconds": round(time.time() - t_pmc, 1),
                          "tag": own_pm.get("tag"), "csrc_hash": own_pm.get("csrc_hash"), "matches_running_sources": True,
                          "valu_busy_validation": own_pm.get("valu_busy_validation")}
        else:
            own_note = where
    ctx = pkg.RenderContext(device=local_rank, rank=rank, world=world)
    ctx.init(args.width, args.height)
    t0 = time.time()
    scene.upload(ctx)
    t_upload = time.time() - t0
    ctx.set_setting("integrator", args.integrator)
    ctx.set_setting("spp", args.spp)
    ctx.set_setting("max_depth", args.max_depth)
    ctx.set_setting("stage_timing", 1)
    ctx.set_setting("count_traversal", 0)
    ctx.set_setting("refill", args.refill)
    ctx.set_setting("streams", args.streams)
    ctx.set_setting("lds_nodes", args.lds_nodes)
    ctx.set_setting("overlap", args.overlap)
    extra = {}
    for kv in args.set:
        k, _, v = kv.partition("=")
        ctx.set_setting(k, v)
        extra[k] = v
    if args.set:
        ctx.update()  # a setting may be one the acceleration structure depends on (flat_instances)

    W, H = args.width, args.height
    local_rows = ctx.local_rows()
    full_fb = torch.empty((H, W, 4), dtype=torch.float32, device=dev) if rank == 0 else None
    gather_ms = []
    gather_mode = "none" if world == 1 else args.gather

    # ---- N > 1, --gather comm: the library's own RCCL gather (rfwhip_comm_*); torch only ships the communicator id -------
    comm = None
    rccl_library = None
    if world > 1 and args.gather == "comm":
        # ONE RCCL in the process: torch.distributed has loaded the librccl.so its wheel bundles; the library's gather opens the
        # same file (RFWHIP_RCCL_LIBRARY) instead of the system's librccl.so.1 — two RCCL builds side by side in one process, one
        # of them with its symbols in the global scope, is a combination nobody tests.  (A host without torch — the plugin — uses
        # the system's.)  An explicit RFWHIP_RCCL_LIBRARY in the environment wins.
        bundled = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if "RFWHIP_RCCL_LIBRARY" not in os.environ and os.path.exists(bundled) and not one_device:
            os.environ["RFWHIP_RCCL_LIBRARY"] = bundled
        rccl_library = os.environ.get("RFWHIP_RCCL_LIBRARY", "librccl.so.1 (system)")
        try:
            idbuf = torch.zeros(128, dtype=torch.uint8, device="cpu" if one_device else dev)
            if rank == 0:
                idbuf.copy_(torch.from_numpy(np.frombuffer(pkg.comm_unique_id(), dtype=np.uint8).copy()))
            dist.broadcast(idbuf, src=0)
            comm = pkg.RenderComm(ctx, idbuf.cpu().numpy().tobytes())
        except Exception as e:
            # a SCALE number must come from host C++ -> RCCL; another path is taken only when asked for (--gather torch)
            raise SystemExit("bench.py: rfwhip_comm_create failed on rank %d (%s) — the library's RCCL gather is the N > 1 path; "
                             "run with --gather torch to measure the torch.distributed gather instead, or --mode group --transport peer "
                             "to take RCCL out of the picture" % (rank, str(e)[:300]))
    local_fb = gathered_flat = gathered = chain_stream = None
    if world > 1 and comm is None:
        local_fb = torch.empty((local_rows, W, 4), dtype=torch.float32, device=dev)
        # the gather lands directly in the [world][local_rows][W] staging image the de-interleave kernel reads
        gathered_flat = torch.empty((world, local_rows, W, 4), dtype=torch.float32, device=dev) if rank == 0 else None
        gathered = list(gathered_flat.unbind(0)) if gathered_flat is not None else None
        # The per-step present -> gather -> de-interleave chain runs on a stream of its own: on torch's default (legacy null)
        # stream the same three small operations cost an 8-GPU rank 0.75 ms of its 14 ms step, although the core's streams
        # are non-blocking.
        chain_stream = torch.cuda.Stream(device=dev)
        torch.cuda.set_stream(chain_stream)

    def step(k, first):
        # render_frame(camera, status): RESET on the first step of a series, CONVERGE afterwards (context.h:19-23)
        ctx.render_async(scene.camera, pkg.RESET if first else pkg.CONVERGE)
        if world == 1:
            return
        if comm is not None:
            # enqueue only: present on the library's gather stream behind the frame, ncclSend / ncclRecv, de-interleave on the
            # root; the next step's kernels overlap the transfer
            comm.gather(full_fb.data_ptr() if rank == 0 else 0)
        elif one_device:
            ctx.wait()
            ctx.read_local_framebuffer_device(local_fb.data_ptr())
            host = local_fb.cpu()
            parts = [torch.empty_like(host) for _ in range(world)] if rank == 0 else None
            dist.gather(host, parts, dst=0)
            if rank == 0:
                gathered_flat.copy_(torch.stack(parts))
                torch.cuda.synchronize()
                ctx.deinterleave_device(gathered_flat.data_ptr(), full_fb.data_ptr())
        elif args.pipeline:
            ts = torch.cuda.current_stream().cuda_stream
            ctx.read_local_framebuffer_stream(local_fb.data_ptr(), ts)
            dist.gather(local_fb, gathered, dst=0)
            if rank == 0:
                ctx.deinterleave_stream(gathered_flat.data_ptr(), full_fb.data_ptr(), ts)
        else:
            ctx.wait()
            t = time.perf_counter()
            ctx.read_local_framebuffer_device(local_fb.data_ptr())
            dist.gather(local_fb, gathered, dst=0)
            if rank == 0:
                torch.cuda.synchronize()
                ctx.deinterleave_device(gathered_flat.data_ptr(), full_fb.data_ptr())
            gather_ms.append((time.perf_counter() - t) * 1e3)

    local_done = [0.0]  # when THIS rank's own work of the region was done (before it waits for the others at the barrier)

    def fence():
        ctx.wait()
        if comm is not None:
            comm.wait()
        torch.cuda.synchronize()
        local_done[0] = time.perf_counter()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for k in range(args.warmup):
        step(k, k == 0)
    fence()
    for name in ctx.KERNELS:
        ctx.get_kernel_time(name, reset=True)
    ctx.get_counters(reset=True)  # also re-arms the device-side clock of the extend stage
    del gather_ms[:]
    t_start = time.perf_counter()
    for k in range(args.steps):
        step(k, k == 0)
    fence()
    elapsed = time.perf_counter() - t_start
    # the image of the last timed step, before anything below renders or gathers into full_fb again (N > 1: the gather probe)
    if world == 1:
        ctx.read_framebuffer_device(full_fb.data_ptr())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"framebuffer": full_fb.cpu().numpy()})
    ranks_info = None
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if one_device else dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        # so that a bad first scaling curve explains itself in one run: every rank's OWN time per step (its renders, its send,
        # on the root the receives and the de-interleave — up to where it starts waiting for the others), and the gather alone
        own = torch.zeros(world, dtype=torch.float64, device="cpu" if one_device else dev)
        own[rank] = (local_done[0] - t_start) / args.steps * 1e3
        dist.all_reduce(own, op=dist.ReduceOp.SUM)
        own = [round(float(x), 4) for x in own.tolist()]
        probe = None
        if comm is not None and args.full:
            # the gather of a finished frame, enqueue to done, with nothing else in flight: present + send on every rank,
            # world - 1 receives + the de-interleave on the root (xGMI: 33 MB / world per peer link)
            times = []
            for _ in range(3):
                ctx.render_async(scene.camera, pkg.CONVERGE)
                ctx.wait()
                torch.cuda.synchronize()
                dist.barrier()
                t0 = time.perf_counter()
                comm.gather(full_fb.data_ptr() if rank == 0 else 0)
                comm.wait()
                times.append((time.perf_counter() - t0) * 1e3)
            pg = torch.zeros(world, dtype=torch.float64, device="cpu" if one_device else dev)
            pg[rank] = sorted(times)[1]
            dist.all_reduce(pg, op=dist.ReduceOp.SUM)
            probe = [round(float(x), 4) for x in pg.tolist()]
        ranks_info = {"ms_per_step_own": own, "ms_per_step_own_min": min(own), "ms_per_step_own_max": max(own),
                      "note": "a rank's own time per step up to its fence (before the barrier); ms_per_step is the max over ranks of the time to the barrier",
                      "gather_enqueue_to_done_ms": probe,
                      "gather_note": "median of 3: gather of a finished frame alone (present + ncclSend per rank; root: world - 1 ncclRecv + de-interleave), per rank" if probe else None}
    kernel_times = {name: ctx.get_kernel_time(name) for name in ctx.KERNELS}
    clock = ctx.get_counters(reset=False)  # extend stage on the device's own clock: first workgroup in .. last workgroup out
    stats = ctx.get_stats().as_dict()

    samples = float(W) * H * args.spp * args.steps
    value = samples / elapsed / 1e6

    # ---- roofline: the extend stage as it ran, and every stage alone on the chip ----------------------------------------
    roofline, stage_rates = None, None
    subs = max(1, min(args.streams, args.spp))
    sub_spp = max(1, args.spp // subs)
    if args.full and not args.no_roofline and rank == 0 and args.integrator == "pt":
        ext_ms, ext_launches = kernel_times["extend"]

        def instrumented(frames, depth):
            ctx.set_setting("count_traversal", 1)
            ctx.set_setting("stage_timing", 0)
            ctx.set_setting("max_depth", depth)
            ctx.get_counters(reset=True)
            for k in range(frames):  # same sample indices as the first timed steps => identical rays
                ctx.render_async(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
            ctx.wait()
            c = ctx.get_counters(reset=True)
            ctx.set_setting("count_traversal", 0)
            ctx.set_setting("max_depth", args.max_depth)
            return c

        replay = min(args.steps, 4)
        cnt = instrumented(replay, args.max_depth)
        cnt0 = instrumented(1, 0)  # the primary wave alone (max_depth 0: the same primary rays, nothing behind them)
        primaries = float(W) * H * args.spp / world  # per step
        prim_hits0 = float(cnt0["shaded"])
        per_step = {k: cnt[k] / replay for k in ("rays_extend", "inner_extend", "tris_extend", "rays_shadow", "inner_shadow",
                                                 "tris_shadow", "shaded", "lds_extend", "lds_shadow")}
        prim = {k: float(cnt0[k]) for k in ("rays_extend", "inner_extend", "tris_extend", "lds_extend")}
        bounce = {k: per_step[k] - prim[k] for k in prim}
        # ---- algorithmic bytes per step, stage by stage ---------------------------------------------------------
        # primary: 20 B hit record written per ray (+ 16 B radiance for a miss the kernel finishes itself; no ray record since round 6), traversal per RAY;
        # bounce: 32 B ray in + 20 B hit out; shadow: 32 B ray in (the contribution record and the 32 B read-modify-write of an
        # unoccluded ray's radiance at depths >= 1, the 16 B store of an occluded one at depth 0 are not counted: no count of them
        # is kept — a lower bound); traversal: 64 B per popped 4-wide node, 52 B per triangle test
        # (round 6, late: a hit's slot of radiance starts in the primary kernel too — 16 B more written here, 16 B less in the shade kernel)
        algo_primary = prim_hits0 * (20 + 16) + (prim["rays_extend"] - prim_hits0) * (16 + 20) + NODE_BYTES * prim["inner_extend"] + 52.0 * prim["tris_extend"]
        algo_bounce = bounce["rays_extend"] * (32 + 20) + NODE_BYTES * bounce["inner_extend"] + 52.0 * bounce["tris_extend"]
        algo_shadow = per_step["rays_shadow"] * 32 + NODE_BYTES * per_step["inner_shadow"] + 52.0 * per_step["tris_shadow"]
        # shade: depth-0 hits read their hit record + instance (20 B; round 6: the primary ray is regenerated from pixel and sample, no direction record) and write 16 B radiance (+ 16 B for the connection term of a
        # path that goes on without a shadow ray: at most the hits minus the shadow rays); deeper entries read origin, direction, throughput, hit record (68 B); a shaded hit gathers
        # its 64 B shading record (round 6; + the 32 B texture-coordinate record on a textured scene) and 48 B of material; 48 B per
        # emitted shadow ray, 48 B per emitted extension ray
        # (the packet form of the primary wave finishes its misses itself — sky term into the slot, no direction record: the shade
        # kernel's scan reads their hit record and instance, 20 B, and nothing else; a per-lane primary kernel leaves them to the shade kernel)
        prim_hits = float(cnt0["shaded"])
        prim_miss = max(0.0, prim["rays_extend"] - prim_hits)
        packet_primaries = (args.refill & 8) != 0 and args.integrator == "pt"
        shade_record = 64 + (32 if ctx.get_setting("textured") == "1" else 0)
        # Round 6, late: (a) the packet form flags the 64-slot groups it has finished and the scan passes them by — the misses' 20 B are
        # read only in groups that also hold a hit (no count of those is kept: counted as 0, a lower bound); (b) the radiance slot of
        # a hit is initialised by the primary kernel, the shade kernel writes it only for a path that adds light or ends at depth 0
        # (no count kept: 0, a lower bound)
        group_flags = packet_primaries and ctx.get_setting("group_flags") == "1"
        algo_shade = (prim_hits * 20 + prim_miss * (0 if group_flags else 20 if packet_primaries else 20 + 16) +
                      max(0.0, prim_hits - per_step["rays_shadow"]) * 16 +
                      bounce["rays_extend"] * 68 + per_step["shaded"] * (shade_record + 48) + per_step["rays_shadow"] * 48 + bounce["rays_extend"] * 48)

        # ---- every stage alone on the chip: one sub-batch's worth of samples on one stream, hipEvents around each launch.  The
        # extension and shadow queues of a depth normally share ONE launch (k_trace_fused); for this table they are launched apart
        ctx.set_setting("streams", 1)
        ctx.set_setting("spp", sub_spp)
        ctx.set_setting("stage_timing", 1)
        ctx.set_setting("overlap", 0)
        ctx.set_setting("fuse", 0)
        ctx.set_setting("shadow_side", 0)  # (the packet form of the depth-0 connection wave on the sub-batch's own stream: alone on the chip like the others)
        ctx.render_frame(scene.camera, pkg.RESET)
        ser_frames, acc = 3, {}
        for k in range(ser_frames):
            ctx.render_frame(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
            st1 = ctx.get_stats().as_dict()
            for key in ("primaryTime", "secondaryTime", "deepTime", "shadowTime", "shadeTime", "finalizeTime"):
                acc[key] = acc.get(key, 0.0) + st1[key] / ser_frames
        ctx.set_setting("streams", args.streams)
        ctx.set_setting("spp", args.spp)
        ctx.set_setting("overlap", args.overlap)
        ctx.set_setting("fuse", int(extra.get("fuse", 1)))
        if not (int(extra.get("fuse", 1)) and (args.refill & 3) == 3 and args.max_depth >= 1):
            ctx.set_setting("shadow_side", int(extra.get("shadow_side", 1)))
        ser = {"primary": acc["primaryTime"], "bounce": acc["secondaryTime"] + acc["deepTime"], "shadow": acc["shadowTime"],
               "shade": acc["shadeTime"], "resolve": acc["finalizeTime"]}
        # ... and once more as the product launches them: extension rays of depth d + 1 and shadow rays of depth d in ONE kernel per
        # depth (k_trace_fused; its time is billed to the extend stage of depth d + 1: secondaryTime + deepTime), still one
        # sub-batch alone on the chip — what the default command's kernel trace shows per kernel, without the other sub-batches
        fused_ms = None
        if int(extra.get("fuse", 1)) and (args.refill & 3) == 3 and args.max_depth >= 1:
            ctx.set_setting("streams", 1)
            ctx.set_setting("spp", sub_spp)
            ctx.set_setting("overlap", 0)
            ctx.set_setting("fuse", 1)
            ctx.render_frame(scene.camera, pkg.RESET)
            facc = {}
            for k in range(ser_frames):
                ctx.render_frame(scene.camera, pkg.RESET if k == 0 else pkg.CONVERGE)
                st1 = ctx.get_stats().as_dict()
                for key in ("primaryTime", "secondaryTime", "deepTime", "shadowTime", "shadeTime", "finalizeTime"):
                    facc[key] = facc.get(key, 0.0) + st1[key] / ser_frames
            ctx.set_setting("streams", args.streams)
            ctx.set_setting("spp", args.spp)
            ctx.set_setting("overlap", args.overlap)
            ctx.set_setting("shadow_side", int(extra.get("shadow_side", 1)))
            fused_ms = {"primary": facc["primaryTime"], "fused": facc["secondaryTime"] + facc["deepTime"] + facc["shadowTime"],
                        "shade": facc["shadeTime"], "resolve": facc["finalizeTime"]}
        frac_of_step = 1.0 / subs  # one sub-batch = 1 / subs of a step's samples
        algo = {"primary": algo_primary * frac_of_step, "bounce": algo_bounce * frac_of_step,
                "shadow": algo_shadow * frac_of_step, "shade": algo_shade * frac_of_step}
        launches = {"primary": 1, "bounce": args.max_depth, "shadow": args.max_depth, "shade": args.max_depth + 1}
        # what binds a stage: the traversal kernels issue VALU instructions nearly every cycle at half-full waves while the BVH is
        # served from LDS / L1 / L2 / the Infinity Cache (their algorithmic byte rate exceeds the HBM peak: "cache_served"); the
        # shade kernel streams the path state and is the one stage whose time is HBM bytes
        bound = {"primary": "valu", "bounce": "valu", "shadow": "valu", "shade": "hbm"}
        STAGE_KERNELS = stage_kernels(ctx, int(ctx.get_setting("sample_group")))
        pm, fresh, source, pmc_note = own_pm, bool(own_pm), own_source, own_note
        if not pm:
            pm, fresh = load_stage_counters(args.stage_json, scene.name, args.spp, args.streams)
            if pm and world > 1:
                # the committed counters describe the launches of ONE rank rendering the whole frame; a rank of a strip split launches
                # 1 / world of that, and no counters were taken for it: the line says so instead of setting them beside its own bytes
                pm, fresh = None, False
                source = {"file": None, "own_passes_not_taken_because": "world %d: the committed counters (%s) are a single rank's whole-frame launches" % (
                    world, os.path.relpath(args.stage_json, ROOT))}
            if pm:
                source = {"file": os.path.relpath(args.stage_json, ROOT), "taken_by": "an earlier run (tools/evidence.sh), committed",
                          "own_passes_not_taken_because": pmc_note or "--pmc off", "tag": pm.get("tag"), "csrc_hash": pm.get("csrc_hash"),
                          "matches_running_sources": fresh, "valu_busy_validation": pm.get("valu_busy_validation")}
            elif pmc_note and world == 1:
                source = {"file": None, "own_passes_not_taken_because": pmc_note}
        stages = []
        chip_hbm_bytes_per_step = 0.0 if (pm and fresh) else None
        chip_valu_ms = 0.0  # per sub-batch: sum over the stages of (VALU-occupied share of the SIMD time x the stage's duration)
        for name in ("primary", "bounce", "shadow", "shade"):
            s_ms = ser[name]
            a_gbs = algo[name] / (s_ms * 1e-3) / 1e9 if s_ms > 0 else None
            ent = {"stage": name, "kernel": STAGE_KERNELS[name], "bound": bound[name], "launches_per_sub_batch": launches[name],
                   "serialised_ms_per_sub_batch": round(s_ms, 4),
                   "algorithmic_bytes_per_sub_batch": algo[name],
                   "algorithmic_gbs": round(a_gbs, 1) if a_gbs else None,
                   "algorithmic_frac_of_hbm_peak": round(a_gbs / HBM_PEAK_GBS, 4) if a_gbs else None,
                   # above 1: the bytes the algorithm asks for are served by the caches, not by HBM (see counter_hbm_* for HBM)
                   "cache_served": bool(a_gbs and a_gbs > HBM_PEAK_GBS)}
            k = pm["kernels"].get(STAGE_KERNELS[name]) if (pm and fresh) else None
            if name == "shadow" and STAGE_KERNELS.get("shadow0") and pm and fresh:
                # the shadow stage as TWO kernels: the packet form for the connections of depth 0 (one launch per sub-batch) and the
                # per-lane kernel for the deeper ones — the stage's entry is their sum per sub-batch, rates weighted by instructions
                k0 = pm["kernels"].get(STAGE_KERNELS["shadow0"])
                if k0:
                    n1 = max(0, launches[name] - 1)
                    parts = [(k0, 1)] + ([(k, n1)] if (k and n1) else [])
                    def tot(key):
                        vals = [(q.get(key) or 0.0) * m for q, m in parts]
                        return sum(vals) if all(q.get(key) is not None for q, _ in parts) else None
                    insts_t = tot("sq_insts_valu_per_dispatch")
                    def wavg(key):
                        if not insts_t or any(q.get(key) is None for q, _ in parts):
                            return None
                        return round(sum(q[key] * (q.get("sq_insts_valu_per_dispatch") or 0.0) * m for q, m in parts) / insts_t, 4)
                    k = {"hbm_bytes_per_dispatch": tot("hbm_bytes_per_dispatch") / launches[name] if tot("hbm_bytes_per_dispatch") is not None else None,
                         "sq_insts_valu_per_dispatch": insts_t / launches[name] if insts_t else None,
                         "avg_dispatch_us": tot("avg_dispatch_us") / launches[name],
                         "valu_lanes_per_instruction": wavg("valu_lanes_per_instruction"), "valu_busy_frac": wavg("valu_busy_frac"),
                         "valu_2_cycle_share": wavg("valu_2_cycle_share"), "valu_slow_pipe_frac": wavg("valu_slow_pipe_frac"),
                         "valu_issue_frac": wavg("valu_issue_frac"), "valu_transcendental_share": wavg("valu_transcendental_share"),
                         "sq_insts_salu_per_dispatch": tot("sq_insts_salu_per_dispatch") / launches[name] if tot("sq_insts_salu_per_dispatch") else None,
                         "salu_busy_frac": wavg("salu_busy_frac")}
                    ent["kernel"] = "%s (depth 0) + %s" % (STAGE_KERNELS["shadow0"], STAGE_KERNELS["shadow"])
            if k:
                n = launches[name]
                hbm, insts = k.get("hbm_bytes_per_dispatch"), k.get("sq_insts_valu_per_dispatch")
                lanes = k.get("valu_lanes_per_instruction")
                pm_ms = k.get("avg_dispatch_us", 0.0) * 1e-3 * n  # the same dispatches under the (serialising) PMC passes
                if hbm and chip_hbm_bytes_per_step is not None:
                    chip_hbm_bytes_per_step += hbm * n * subs
                if k.get("valu_busy_frac") is not None:
                    chip_valu_ms += k["valu_busy_frac"] * pm_ms
                rate = insts * n / (pm_ms * 1e-3) if (insts and pm_ms > 0) else None
                ent.update({
                    "counter_hbm_bytes_per_sub_batch": hbm * n if hbm else None,
                    "counter_hbm_gbs": round(hbm * n / (pm_ms * 1e-3) / 1e9, 1) if (hbm and pm_ms > 0) else None,
                    "counter_hbm_frac_of_peak": round(hbm * n / (pm_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if (hbm and pm_ms > 0) else None,
                    "counter_over_algorithmic_bytes": round(hbm * n / algo[name], 3) if (hbm and algo[name] > 0) else None,
                    "counter_ms_per_sub_batch": round(pm_ms, 4),
                    "valu_wave_insts_per_sub_batch": insts * n if insts else None,
                    "valu_lanes_active_of_64": lanes,
                    # wave-instructions per second against BOTH ceilings: the guide's (a wave64 instruction every 2 cycles per SIMD:
                    # what v_fma / v_mul / v_add_f32 reach, profiles/micro/valu_calib.hip) and the 4-cycle rate at which this part issues
                    # compares, selects, conversions and min / max (profiles/micro/valu_micro.hip).  A mix of both can exceed 1.0 of the
                    # 4-cycle rate — it is a ceiling for a mix WITHOUT 2-cycle instructions; valu_busy_frac weights the classes
                    "valu_issue_frac_of_2_cycle_rate": round(rate / VALU_ISSUE_PEAK, 4) if rate else None,
                    "valu_issue_frac_of_4_cycle_rate": round(rate / (VALU_ISSUE_PEAK / 2), 4) if rate else None,
                    "valu_lane_weighted_frac_of_2_cycle_rate": round(rate / VALU_ISSUE_PEAK * lanes / 64.0, 4) if (rate and lanes) else None,
                    # share of SIMD cycles a VALU instruction occupied, by instruction class: (2 x (FMA + MUL + ADD_F32) + 8 x transcendentals
                    # + 4 x the rest) / SIMD cycles (profiles/summarize.py; validated on a pure v_fma_f32 kernel: traffic_source.valu_busy_validation)
                    "valu_busy_frac": k.get("valu_busy_frac"), "valu_2_cycle_share": k.get("valu_2_cycle_share"),
                    # round 5's non-additive model (tools/dev/micro/inst_rate3.hip): time ~ max(4.3 x 4-clock instructions + 8.6 x
                    # transcendentals, 2.5 x all VALU instructions) over the SIMD cycles
                    "valu_slow_pipe_frac": k.get("valu_slow_pipe_frac"), "valu_issue_frac": k.get("valu_issue_frac"),
                    "valu_transcendental_share": k.get("valu_transcendental_share"),
                    # the CU's scalar unit: 4.46 SIMD clocks per scalar instruction (tools/dev/micro/inst_rate5.hip) over the launch's SIMD
                    # cycles — the packet kernels are bound by it as much as by their VALUs (DESIGN.md §4 "Round 6")
                    "salu_insts_per_sub_batch": k.get("sq_insts_salu_per_dispatch") * n if k.get("sq_insts_salu_per_dispatch") else None,
                    "salu_busy_frac": k.get("salu_busy_frac"),
                })
            else:
                ent.update({"counter_hbm_bytes_per_sub_batch": None, "valu_wave_insts_per_sub_batch": None, "valu_lanes_active_of_64": None,
                            "valu_issue_frac_of_2_cycle_rate": None, "valu_busy_frac": None})
            stages.append(ent)
        kres = pm["kernels"].get("k_resolve") if (pm and fresh) else None
        if kres and kres.get("hbm_bytes_per_dispatch") and chip_hbm_bytes_per_step is not None:
            chip_hbm_bytes_per_step += kres["hbm_bytes_per_dispatch"]

        # ---- the headline: the kernel that DOMINATES the default command, by the time its launches take alone on the chip ------------
        # (round 4's verdict: the shade kernel was "largest" only because the measurement leg un-fused the kernel the product really
        # runs).  Candidates are the kernels as the product launches them — the packet primary wave, k_trace_fused (extension rays of
        # depth d + 1 and shadow rays of depth d: one launch per depth), the shade kernel, the resolve — timed one sub-batch at a time
        # with hipEvents on the launch's own stream (the fused serialised leg above; the same kernels under rocprofv3 --kernel-trace
        # of the default command: profiles/r05*_kernel_stats.md).  On the bench scene that is k_trace_fused: bound by VALU issue at
        # half-full waves, its bytes served by LDS / L1 / L2 / the Infinity Cache — `achieved` (algorithmic bytes per launch over the
        # launch's duration) EXCEEDS the HBM peak, `cache_served`, and says nothing about how good the kernel is; what does is in
        # `valu`: wave-instructions per second against the issue ceilings, lanes per instruction, and the counters' HBM bytes.
        # The one stage whose time IS bytes, the shade kernel, keeps round 4's figures under `hbm_kernel`.
        shade_ms_total, shade_launches = kernel_times["shade"]
        launches_per_step = shade_launches / max(1, args.steps)
        bytes_per_launch = algo_shade / max(1.0, launches_per_step)
        ms_in_region = shade_ms_total / max(1, shade_launches)
        ms_per_launch = ser["shade"] / (args.max_depth + 1)
        achieved = bytes_per_launch / (ms_per_launch * 1e-3) / 1e9 if ms_per_launch > 0 else 0.0
        kshade = pm["kernels"].get(STAGE_KERNELS["shade"]) if (pm and fresh) else None
        traffic = int(kshade["hbm_bytes_per_dispatch"]) if (kshade and kshade.get("hbm_bytes_per_dispatch")) else None
        busy_ms = sum(kernel_times[name][0] for name in ctx.KERNELS)
        step_ms = elapsed / args.steps * 1e3
        kernel_share = {k: round(v / max(1e-9, sum(ser.values())), 4) for k, v in ser.items()}
        hbm_kernel = {
            "bound": "hbm", "kernel": STAGE_KERNELS["shade"],
            "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
            "traffic": traffic,
            "traffic_frac_of_peak": round(traffic / (ms_per_launch * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if (traffic and ms_per_launch > 0) else None,
            "traffic_over_algorithmic": round(traffic / bytes_per_launch, 3) if traffic else None,
            "algorithmic_bytes_per_launch": bytes_per_launch, "ms_per_launch": round(ms_per_launch, 4),
            "launches_per_step": launches_per_step,
            "frac_of_measured_copy_peak_6290": round(achieved / 6290.0, 5),
            "in_timed_region": {"ms_per_launch": round(ms_in_region, 4), "launches_timed": shade_launches,
                                "achieved": round(bytes_per_launch / (ms_in_region * 1e-3) / 1e9, 2) if ms_in_region > 0 else None,
                                "frac": round(bytes_per_launch / (ms_in_region * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if ms_in_region > 0 else None},
            "cross_checks": {"kernel_ms_per_step": round(ms_per_launch * launches_per_step, 3),
                             "kernel_time_fits_step": bool(ms_per_launch * launches_per_step <= step_ms),
                             "algorithmic_gbs_over_the_step": round(algo_shade / (step_ms * 1e-3) / 1e9, 1),
                             "algorithmic_rate_below_peak": bool(algo_shade / (step_ms * 1e-3) / 1e9 <= HBM_PEAK_GBS)}}
        # the candidates' times per sub-batch, alone on the chip, as the product launches them
        # (round 6, connections of depth 0 in packet form: the bounce and shadow waves are no longer ONE kernel per depth — the extension
        # rays of depth 1 run in k_trace_stream<false>, the connections of depth 0 beside them in k_shadow_packet, only the deeper waves
        # share k_trace_fused — so they are candidates of their own: bounce = the extension rays' launches and halves, shadow = the
        # connections'; hipEvents and, inside k_trace_fused, the device's tick sums, as the product launches them)
        if fused_ms and STAGE_KERNELS.get("shadow0"):
            cand = {"primary": facc["primaryTime"], "bounce": facc["secondaryTime"] + facc["deepTime"], "shadow": facc["shadowTime"],
                    "shade": facc["shadeTime"], "resolve": facc["finalizeTime"]}
        elif fused_ms:
            cand = dict(fused_ms)
        else:
            cand = {"primary": ser["primary"], "bounce": ser["bounce"], "shadow": ser["shadow"], "shade": ser["shade"], "resolve": ser["resolve"]}
        dom = max(cand, key=lambda k: cand[k])
        dom_kernel = {"primary": STAGE_KERNELS["primary"], "fused": STAGE_KERNELS["fused"],
                      "bounce": STAGE_KERNELS["bounce"] + (" (+ the extension rays' half of %s at depth >= 2)" % STAGE_KERNELS["fused"] if fused_ms else ""),
                      "shadow": ("%s (depth 0) + the connections' half of %s" % (STAGE_KERNELS["shadow0"], STAGE_KERNELS["fused"])) if STAGE_KERNELS.get("shadow0") else STAGE_KERNELS["shadow"],
                      "shade": STAGE_KERNELS["shade"], "resolve": "k_resolve"}[dom]
        dom_launches = {"primary": 1, "fused": args.max_depth, "bounce": args.max_depth, "shadow": args.max_depth,
                        "shade": args.max_depth + 1, "resolve": 1}[dom]
        dom_parts = {"fused": ("bounce", "shadow")}.get(dom, (dom,))  # the stage entries whose bodies the kernel runs
        dom_algo = sum(algo.get(q, 0.0) for q in dom_parts)          # algorithmic bytes per sub-batch
        dom_ms = cand[dom]
        dom_bound = "hbm" if dom in ("shade", "resolve") else "valu"
        ent_of = {e["stage"]: e for e in stages}
        dom_hbm = sum((ent_of[q].get("counter_hbm_bytes_per_sub_batch") or 0.0) for q in dom_parts if q in ent_of) or None
        dom_insts = sum((ent_of[q].get("valu_wave_insts_per_sub_batch") or 0.0) for q in dom_parts if q in ent_of) or None
        dom_lane_insts = sum((ent_of[q].get("valu_wave_insts_per_sub_batch") or 0.0) * (ent_of[q].get("valu_lanes_active_of_64") or 0.0)
                             for q in dom_parts if q in ent_of) or None
        dom_ach = dom_algo / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
        dom_rate = dom_insts / (dom_ms * 1e-3) if (dom_insts and dom_ms > 0) else None
        # `achieved / peak / unit / frac` speak the language of what binds the kernel (round 5's verdict: an algorithmic byte rate of 1.8 x
        # the HBM peak is not a fraction of anything).  bound "valu": VALU wave-instructions per second of the launch against the
        # chip's issue peak (1024 SIMDs x 2.4 GHz / 2 cycles per wave64 instruction), `lane_weighted_frac` = the same weighted by the
        # lanes that did work; the bytes — algorithmic (cache-served) and HBM by the counters — sit under `bytes`.  bound "hbm":
        # algorithmic bytes per second against the HBM peak, as SURVEY §8(d) prescribes.  Without counters for the running sources a
        # VALU-bound kernel has no measured rate: the headline then falls back to the HBM-bound kernel (`hbm_kernel`, always measured).
        dom_bytes = {"algorithmic_bytes_per_launch": dom_algo / dom_launches,
                     "algorithmic_gbs": round(dom_ach, 2), "algorithmic_frac_of_hbm_peak": round(dom_ach / HBM_PEAK_GBS, 5),
                     # above the HBM peak: the bytes the algorithm asks for come out of LDS, L1, L2 and the Infinity Cache
                     "cache_served": bool(dom_ach > HBM_PEAK_GBS),
                     "counter_hbm_bytes_per_launch": int(dom_hbm / dom_launches) if dom_hbm else None,
                     "counter_hbm_gbs": round(dom_hbm / (dom_ms * 1e-3) / 1e9, 1) if (dom_hbm and dom_ms > 0) else None,
                     "counter_hbm_frac_of_peak": round(dom_hbm / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if (dom_hbm and dom_ms > 0) else None,
                     "counter_over_algorithmic": round(dom_hbm / dom_algo, 3) if (dom_hbm and dom_algo > 0) else None}
        dom_desc = "%s — the largest kernel of the default command by time: %.0f %% of a sub-batch's kernel time, every launch alone on the chip (%s)" % (
            dom_kernel, 100.0 * dom_ms / max(1e-9, sum(cand.values())),
            ", ".join("%s %.2f ms" % (k, v) for k, v in sorted(cand.items(), key=lambda kv: -kv[1])))
        if dom_bound == "valu" and dom_rate:
            lanes_avg = dom_lane_insts / dom_insts if (dom_insts and dom_lane_insts) else None
            head = {"bound": "valu", "kernel": dom_desc,
                    "achieved": round(dom_rate / 1e9, 2), "peak": round(VALU_ISSUE_PEAK / 1e9, 1), "unit": "G wave-instructions/s",
                    "frac": round(dom_rate / VALU_ISSUE_PEAK, 5),
                    "lane_weighted_frac": round(dom_rate / VALU_ISSUE_PEAK * lanes_avg / 64.0, 5) if lanes_avg else None,
                    "lanes_active_of_64": round(lanes_avg, 2) if lanes_avg else None,
                    "wave_insts_per_launch": dom_insts / dom_launches,
                    # the measured two-class model (tools/dev/micro/inst_rate3.hip): share of the SIMD time the 4-clock pipe / instruction
                    # issue is busy, per body of the kernel
                    "slow_pipe_frac_by_stage": {q: ent_of[q].get("valu_slow_pipe_frac") for q in dom_parts if q in ent_of},
                    "issue_frac_by_stage": {q: ent_of[q].get("valu_issue_frac") for q in dom_parts if q in ent_of},
                    "busy_frac_by_stage": {q: ent_of[q].get("valu_busy_frac") for q in dom_parts if q in ent_of},
                    "traffic": dom_bytes["counter_hbm_bytes_per_launch"], "bytes": dom_bytes}
        elif dom_bound == "hbm":
            head = {"bound": "hbm", "kernel": dom_desc, "achieved": round(dom_ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(dom_ach / HBM_PEAK_GBS, 5), "traffic": dom_bytes["counter_hbm_bytes_per_launch"], "bytes": dom_bytes}
        else:
            head = {"bound": "hbm", "kernel": "%s — the HBM-bound kernel; the largest kernel by time is VALU-bound (%s) and has no counters for the running sources (traffic_source)" % (
                        STAGE_KERNELS["shade"], dom_desc),
                    "achieved": hbm_kernel["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": hbm_kernel["frac"], "traffic": hbm_kernel["traffic"],
                    "dominant_kernel_bytes": dom_bytes}
        roofline = dict(head)
        roofline.update({
            "traffic_source": source,
            "ms_per_launch": round(dom_ms / dom_launches, 4),
            "ms_per_launch_clock": "hip events on the launch's stream; %d-spp sub-batch, every launch alone on the chip (streams=1, host waits per frame), this process" % sub_spp,
            "launches_per_step": dom_launches * subs,
            "candidates_ms_per_sub_batch": {k: round(v, 4) for k, v in cand.items()},
            "hbm_kernel": hbm_kernel,
            "in_timed_region": {"kernels_in_flight": round(busy_ms / (elapsed * 1e3), 3) if elapsed > 0 else None,
                                "note": "%d sub-batches in flight: a launch shares the chip and stretches with its company (what rocprofv3 --kernel-trace of the default command shows per launch)" % subs},
            # both must hold for the headline to be physical: the kernel's launches of a step fit into the step, and the bytes it
            # is billed for do not exceed what HBM can deliver in that time
            "cross_checks": {
                "kernel_ms_per_step": round(dom_ms * subs, 3), "ms_per_step": round(step_ms, 3),
                "kernel_time_fits_step": bool(dom_ms * subs <= step_ms),
                "counter_hbm_gbs_over_the_step": round(dom_hbm * subs / (step_ms * 1e-3) / 1e9, 1) if dom_hbm else None,
                "counter_hbm_rate_below_peak": bool(dom_hbm * subs / (step_ms * 1e-3) / 1e9 <= HBM_PEAK_GBS) if dom_hbm else None,
                "all_stages_ms_per_step": round(sum(ser.values()) * subs, 3),
                "all_stages_over_step": round(sum(ser.values()) * subs / step_ms, 3)},
            # the whole chip over the timed region: HBM bytes of every kernel of a step by the counters / the step time
            "chip": {"counter_hbm_bytes_per_step": chip_hbm_bytes_per_step,
                     "counter_hbm_gbs": round(chip_hbm_bytes_per_step / (step_ms * 1e-3) / 1e9, 1) if chip_hbm_bytes_per_step else None,
                     "counter_hbm_frac_of_peak": round(chip_hbm_bytes_per_step / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if chip_hbm_bytes_per_step else None,
                     # VALU-occupied SIMD time of every stage (its valu_busy_frac x its counter-pass duration: class-weighted instruction
                     # cycles, profiles/summarize.py) over the pipelined step: how busy the chip's 1024 VALUs are while the step runs
                     "valu_busy_ms_per_step": round(chip_valu_ms * subs, 2) if chip_valu_ms else None,
                     "valu_busy_frac_over_step": round(chip_valu_ms * subs / step_ms, 4) if chip_valu_ms else None,
                     "binding_ceiling": "VALU issue: a step is %.1f G wave-instructions of mostly 4-cycle operations on 1024 SIMDs" % (
                         sum((e.get("valu_wave_insts_per_sub_batch") or 0) for e in stages) * subs / 1e9) if (pm and fresh) else None},
            "per_ray": {"inner_nodes": per_step["inner_extend"] / max(1, per_step["rays_extend"]),
                        "triangle_tests": per_step["tris_extend"] / max(1, per_step["rays_extend"]),
                        "primary_inner_nodes": prim["inner_extend"] / max(1, prim["rays_extend"]),
                        "primary_triangle_tests": prim["tris_extend"] / max(1, prim["rays_extend"]),
                        "rays_per_sample": per_step["rays_extend"] / max(1.0, primaries),
                        "shadow_rays_per_sample": per_step["rays_shadow"] / max(1.0, primaries),
                        "shadow_inner_nodes": per_step["inner_shadow"] / max(1, per_step["rays_shadow"]),
                        "shadow_triangle_tests": per_step["tris_shadow"] / max(1, per_step["rays_shadow"]),
                        "shaded_hits_per_sample": per_step["shaded"] / max(1.0, primaries)},
            "serialised_kernel_share": kernel_share, "sub_batch_ms_total": round(sum(ser.values()), 4),
            "valu_issue_peak_g_per_s": VALU_ISSUE_PEAK / 1e9,
            "stages": stages,
        })
        if args.stage_rates:
            def rate(count, ms):
                return round(count / (ms * 1e-3) / 1e6, 1) if ms > 0 else None
            f = frac_of_step
            stage_rates = {"spp": sub_spp, "streams": 1,
                           "primary": rate(prim["rays_extend"] * f, ser["primary"]), "bounce": rate(bounce["rays_extend"] * f, ser["bounce"]),
                           "shadow": rate(per_step["rays_shadow"] * f, ser["shadow"]),
                           "stage_ms": {k: round(v, 3) for k, v in acc.items()}}

    # ---- the configuration the reference actually runs: BLUENOISE 1 (context/settings.h:12, Kernels.cu:391-394, :712-719) --------
    # the primary rays' jitter and the depth-0 light samples come from the blue-noise table instead of the hash RNG.  Timed with a
    # table of the reference's LAYOUT filled with our own numbers (scenes.synthetic_blue_noise: the published table belongs to
    # the reference tree and reaches the core through rfwhip_set_blue_noise) — same fetches, same arithmetic, other values.
    bluenoise = None
    if args.full and not args.no_roofline and rank == 0 and world == 1 and args.integrator == "pt":
        ctx.set_blue_noise(pkg.scenes.synthetic_blue_noise())
        ctx.set_setting("sampler", "bluenoise")
        ctx.set_setting("stage_timing", 0)
        bn_steps = max(2, min(args.steps, 4))
        ctx.render_async(scene.camera, pkg.RESET)
        ctx.wait()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(bn_steps):
            ctx.render_async(scene.camera, pkg.CONVERGE)
        ctx.wait()
        torch.cuda.synchronize()
        bn_ms = (time.perf_counter() - t0) / bn_steps * 1e3
        ctx.set_setting("sampler", "hash")
        ctx.set_setting("stage_timing", 1)
        bluenoise = {"value": round(float(W) * H * args.spp / (bn_ms * 1e-3) / 1e6, 3), "unit": "Msamples/s", "ms_per_step": round(bn_ms, 4), "steps": bn_steps,
                     "over_hash_sampler": round((float(W) * H * args.spp / (bn_ms * 1e-3) / 1e6) / value, 4),
                     "note": "sampler=bluenoise (the reference's BLUENOISE 1 branch) with a synthetic table of the reference's layout; "
                             "the headline runs the reference's own hash-RNG branch (`#else`)"}

    # ---- CPU baselines: the oracle (a port, not the reference build) on this box's host cores ---------------------------
    cpu_baseline, parity, cpu_parity = None, None, None
    if args.full and not args.no_cpu_baseline and rank == 0 and world == 1:
        from __graft_entry__ import load_oracle
        orc = load_oracle()
        cores = usable_cores()
        ref = orc.OracleContext(pkg)
        ref.init(W, H)
        t0 = time.time()
        scene.upload(ref)  # includes the oracle's own (reference-style) BVH build; not timed
        t_build = time.time() - t0
        ref.set_setting("threads", cores)

        def oracle_rate(integrator, seconds, max_frames):
            ref.set_setting("integrator", integrator)
            ref.set_setting("max_depth", args.max_depth)
            ref.set_setting("spp", 1)
            done, spent = 0, 0.0
            while spent < seconds and done < max_frames:
                t0 = time.perf_counter()
                ref.render_frame(scene.camera, pkg.RESET if done == 0 else pkg.CONVERGE)
                spent += time.perf_counter() - t0
                done += 1
            return done, spent

        embree = probe_embree()
        embree_note = embree if embree else "not found (ldconfig, /usr, /usr/local, /opt searched)"
        # (1) the Embree rendercore's algorithm (the parity integrator) — oracle on the CPU, HIP on the GPU, same scene
        pdone, pspent = oracle_rate("parity", max(4.0, args.cpu_seconds * 0.4), 32)
        ctx.set_setting("integrator", "parity")
        ctx.set_setting("stage_timing", 0)
        ctx.set_setting("spp", 16)
        ctx.render_frame(scene.camera, pkg.RESET)
        t0 = time.perf_counter()
        psteps = 6
        for k in range(psteps):
            ctx.render_async(scene.camera, pkg.CONVERGE)
        ctx.wait()
        gpu_parity = float(W) * H * 16 * psteps / (time.perf_counter() - t0) / 1e6
        ctx.set_setting("integrator", args.integrator)
        cpu_parity_value = float(W) * H * pdone / pspent / 1e6
        cpu_parity = {"value": round(cpu_parity_value, 4), "unit": "Msamples/s", "cores": cores, "kind": "port",
                      "cpu_model": cpu_model(), "flags": oracle_flags(), "embree": embree_note, "gpu_value": round(gpu_parity, 2), "gpu_over_cpu": round(gpu_parity / cpu_parity_value, 1),
                      "sample": "%d full %dx%d frame(s) at 1 spp, parity integrator (EmbreeRT/src/Context.cpp:104-300 restated: 1 primary "
                                "ray + one shadow ray per light per sample), oracle/rfw_oracle.c with OpenMP, %.1f s; GPU: %d steps of 16 spp, "
                                "same scene and camera" % (pdone, W, H, pspent, psteps)}
        # (2) the metric's own integrator
        done, spent = oracle_rate(args.integrator, args.cpu_seconds, 64)
        cpu_value = float(W) * H * done / spent / 1e6
        cpu_baseline = {"value": round(cpu_value, 4), "unit": "Msamples/s", "cores": cores, "kind": "port",
                        # CPU model string, compiler + flags beside the number (no -march=native: the prebuilt
                        # library travels to the GPU box; the reference itself builds with -ffast-math -mavx2)
                        "cpu_model": cpu_model(), "flags": oracle_flags(),
                        # an Embree harness would be the first choice; none is installed on the box, so the
                        # oracle port is the only CPU line
                        "embree": embree_note,
                        "sample": "%d full %dx%d frame(s) at 1 spp of the same scene/camera/integrator (%s, depth %d), "
                                  "oracle/rfw_oracle.c with OpenMP, %.1f s; oracle BVH build %.1f s not timed"
                                  % (done, W, H, args.integrator, args.max_depth, spent, t_build)}
        # cross-check while both are here (outside every timed region; the oracle is the checker, not the thing measured):
        # the oracle has just accumulated sample indices 0..done-1 of this very scene — render the same indices on the GPU
        ref_img = ref.framebuffer()[..., :3]
        ref.destroy()
        ctx.set_setting("spp", done)
        ctx.set_setting("stage_timing", 0)
        ctx.render_frame(scene.camera, pkg.RESET)
        hip_img = ctx.framebuffer()[..., :3]
        ctx.set_setting("spp", args.spp)
        d = np.sqrt(((hip_img.astype(np.float64) - ref_img) ** 2).sum(-1))
        frac, rmse = float((d > 3e-2).mean()), float(np.sqrt((d ** 2).mean()))
        mean_rel = float(abs(hip_img.mean() - ref_img.mean()) / ref_img.mean())
        # 8x8 block means: per-pixel differences of a path tracer are decision flips (a 1-ulp sin / rcp difference sends one
        # sample of one pixel another way), which average out; a bias would not
        hb = hip_img[:H // 8 * 8, :W // 8 * 8].reshape(H // 8, 8, W // 8, 8, 3).mean((1, 3))
        rb = ref_img[:H // 8 * 8, :W // 8 * 8].reshape(H // 8, 8, W // 8, 8, 3).mean((1, 3))
        block_rel = float(np.abs(hb - rb).mean() / rb.mean())
        crit = {"mean_rel_max": 2e-3, "block8_mean_abs_rel_max": 2e-2, "frac_gt_3e-2_max": 4e-2}
        parity = {"samples_per_pixel": done, "tolerance": 3e-2, "frac_gt_3e-2": round(frac, 6), "rmse": round(rmse, 6),
                  "mean_rel": round(mean_rel, 7), "block8_mean_abs_rel": round(block_rel, 6),
                  "hip_mean": float(hip_img.mean()), "oracle_mean": float(ref_img.mean()),
                  "criterion": crit,
                  "criterion_note": "statistical agreement of two float32 path tracers after %d spp (discrete decisions amplify 1-ulp "
                                    "differences; the bit-level parity tests are tests/test_parity_gpu.py, tests/test_pt_golden.py): image "
                                    "means, 8x8 block means and the share of pixels beyond the tolerance" % done,
                  "pass": bool(mean_rel <= crit["mean_rel_max"] and block_rel <= crit["block8_mean_abs_rel_max"] and frac <= crit["frac_gt_3e-2_max"])}

    if rank == 0:
        out = {
            "metric": ("Msamples/sec at 1920x1080, 1M-tri scene; 1/2/4/8-GPU tile scaling" if args.workload == "terrain" else
                       "Msamples/sec at 1920x1080, Sponza-scale instanced textured scene (BASELINE config 4); tile scaling"),
            "value": round(value, 3), "unit": "Msamples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic", "full": bool(args.full),
            "config": {"workload": "%s: %d triangles, %dx%d, %s integrator depth %d, %d spp per step, %d area-light "
                                   "triangles + %d point lights, synthetic 2048x1024 HDR sky"
                                   % (scene.name, scene.triangle_count(), W, H, args.integrator, args.max_depth, args.spp,
                                      len(scene.area_lights), len(scene.point_lights)),
                       "parallelism": ("single GPU, no collective" if world == 1 else
                                       "image strips of 8 rows interleaved over %d ranks, one gather per step into rank 0's HBM" % world),
                       "gather": gather_mode if world > 1 else None, "rccl_library": rccl_library,
                       "gather_note": (None if world == 1 else
                                       "comm = rfwhip_comm_gather: ncclSend on every rank / ncclRecv x (world - 1) on the root issued by "
                                       "librfwhip.so, stream-ordered, overlapping the next step; torch = torch.distributed.gather"),
                       "pipeline": int(args.pipeline) if (world > 1 and comm is None) else None,
                       "spp_per_step": args.spp, "streams": args.streams, "settings": extra or None,
                       "sample_group": int(ctx.get_setting("sample_group")), "csrc_hash": csrc_hash()},
            "roofline": roofline, "sampler_bluenoise": bluenoise, "cpu_baseline": cpu_baseline, "cpu_baseline_parity": cpu_parity,
            # per-pixel RGB L2 between the GPU image and the oracle image of the same sample indices (None when the CPU leg is off)
            "parity_vs_cpu_baseline": parity,
            "stage_ms_per_step": {k: round(v[0] / args.steps, 4) for k, v in kernel_times.items()},
            "last_frame_counts": {k: stats[k] for k in ("primaryCount", "secondaryCount", "deepCount", "shadowCount")},
            # rays of one step (this rank's strips) over the step time: closest-hit (primary + extension) and any-hit
            "grays_per_s": {"closest_hit": round((stats["primaryCount"] + stats["secondaryCount"] + stats["deepCount"])
                                                 / (elapsed / args.steps) / 1e9, 3),
                            "shadow": round(stats["shadowCount"] / (elapsed / args.steps) / 1e9, 3)},
            "mrays_per_s_per_stage_serialised": stage_rates,
            "gather_ms_per_step": (round(sum(gather_ms) / len(gather_ms), 4) if gather_ms else
                                   (None if world > 1 else 0.0)),
            "setup_s": {"scene": round(t_scene, 2), "upload_and_bvh": round(t_upload, 2)},
            "image_mean": float(full_fb[..., :3].mean().item()),
            "ranks": ranks_info,
        }
        print(json.dumps(out))
    if comm is not None:
        comm.destroy()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
