"""bench.py end to end on the device at a small size: a plain run prints the headline line only
(--steps is the number of timed steps, ms_per_step their mean, none of the --full figures), and
--dump-outputs writes what the last timed step left as float32 / float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "env_roofline", "learn_us", "actenv_us", "act_full_roofline", "env_step_roofline",
             "scalar_dropin", "cpu_baseline", "cpu_config0")


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_outputs(tmp_path):
    n, cap, steps, warm = 2048, 8192, 6, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warm), "--arenas", str(n), "--memory", str(cap), "--dump-outputs", str(tmp_path / "out")],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] and d["metric"]
    assert d["steps"] == steps and d["warmup"] == warm and d["ms_per_step"] > 0
    assert d["learner"]["train_steps"] == steps + warm and d["config"]["updates_in_timed_region"] == steps
    assert abs(d["value"] - n * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]  # both from the same timed region
    assert not [k for k in FULL_ONLY if k in d]
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == sorted(k + ".npy" for k in d["dumped"]["arrays"]) and "paramsB.npy" in files
    total = 0
    for f in files:
        a = np.load(tmp_path / "out" / f)
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    assert total <= 64 * 1000 * 1000
    load = lambda k: np.load(tmp_path / "out" / (k + ".npy"))  # noqa: E731
    assert load("obsB").shape == (n, 7) and load("env_f64").shape == (n, 7) and load("aB").shape == (n,)
    assert set(np.unique(load("aB"))) <= {0.0, 1.0, 2.0}
    c = dict(zip(("step", "pos", "size", "train_steps"), load("counters")[:4]))
    assert c["step"] == steps + warm and c["train_steps"] == steps + warm and c["size"] == cap
    assert np.abs(load("paramsB") - load("paramsT")).max() > 0  # the updates moved the learner off its target
