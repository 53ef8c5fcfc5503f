"""bench.py's two kinds of run: a plain run is the headline alone (set-up, warm-up, the timed steps, --dump-outputs, the
line); --full adds what the headline does not need — roofline and counters, the blue-noise sampler, the CPU baselines and
the GPU image against the oracle's — after the timed region, so that the timed steps and their image are the same."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SMALL = ["--steps", "2", "--warmup", "1", "--spp", "8", "--width", "480", "--height", "270", "--grid", "64"]
EXTRAS = ("roofline", "sampler_bluenoise", "cpu_baseline", "cpu_baseline_parity", "parity_vs_cpu_baseline")


def test_plain_is_the_default_and_what_belongs_to_full_asks_for_it():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and (a.steps, a.warmup) == (3, 1)
    assert bench.parse(["--full", "--stage-rates", "--pmc", "on"]).full
    # the roofline's options without --full are refused, not dropped without a word
    for extra in (["--stage-rates"], ["--pmc", "on"]):
        with pytest.raises(SystemExit):
            bench.parse(extra)
    # what the counter passes' child runs and the scripts' plain runs pass is still accepted
    assert not bench.parse(["--no-roofline", "--no-cpu-baseline", "--pmc", "off"]).full


def _bench(args, out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args + ["--dump-outputs", out_dir],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench([], str(tmp_path / "plain"))
    assert plain["full"] is False and all(plain[k] is None for k in EXTRAS), {k: plain[k] is None for k in EXTRAS}
    full = _bench(["--full", "--pmc", "off", "--cpu-seconds", "1"], str(tmp_path / "full"))
    assert full["full"] is True and all(full[k] is not None for k in EXTRAS), {k: full[k] is None for k in EXTRAS}
    for d in (plain, full):
        assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["value"] > 0 and d["ms_per_step"] > 0 and (d["steps"], d["warmup"]) == (2, 1)
    # everything --full adds runs after the timed steps: the image of the last timed step is the same
    a = np.load(str(tmp_path / "plain" / "framebuffer.npy"))
    b = np.load(str(tmp_path / "full" / "framebuffer.npy"))
    assert a.shape == (270, 480, 4) and np.array_equal(a, b)
    assert plain["image_mean"] == full["image_mean"]
