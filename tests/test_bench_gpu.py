"""bench.py's contract (the driver parses its one JSON line): a short run of the default workload at a small
resolution must print a well-formed line with the roofline and timing fields."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--res", "256",
                        "--batch", "1", "--full", "--no-cpu-baseline", "--no-vae"], capture_output=True, text=True,
                       timeout=280, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["n_gpus"] == 1 and d["steps"] == 2
    rf = d["roofline"]
    assert rf["achieved"] > 0 and 0 < rf["frac"] < 1 and rf["peak"] > 0 and rf["isolated_frac"] > 0
    assert d["config"]["parallelism"] == "dp1"


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps and runs none of the side measurements; --dump-outputs
    writes what the last timed step returned and left behind as float32 .npy files, and two runs with the same
    arguments write the same arrays (same seeded inputs; the tiny step is bit-deterministic,
    tests/test_train_step_gpu.py).  The tiny SDXL-shaped UNet: the leg under test is the bench's."""
    import numpy as np
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dirs = [tmp_path / "a", tmp_path / "b"]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup",
                               "1", "--res", "128", "--batch", "2", "--tiny", "--dump-outputs", str(d)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=env) for d in dirs]
    outs = [p.communicate(timeout=170) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    lines = [ln for ln in outs[0][0].splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, outs[0][0][-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and len(d["step_ms_each"]) == 3 and len(d["losses_exact"]) == 3 and d["ms_per_step"] > 0
    assert d["value"] > 0 and d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["cpu_baseline"] is None and d["vae_encode"] is None
    rf = d["roofline"]
    assert "achieved" not in rf and "isolated_achieved" not in rf and rf["step_achieved"] > 0
    a, b = ({f.name: np.load(f) for f in sorted(x.iterdir())} for x in dirs)
    assert {"loss.npy", "losses.npy", "params.npy"} <= set(a) and set(a) == set(b)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    assert a["losses.npy"].tolist() == d["losses_exact"] and a["loss.npy"].tolist() == d["losses_exact"][-1:]
    assert a["params.npy"].size > 0 and a["params.npy"].std() > 0


def test_bench_two_ranks_json_line():
    """bench.py's multi-rank leg (launch_ranks + the world > 1 paths: barrier, max-over-ranks time, loss mean)
    run before the driver's multi-GPU node does: two child ranks on the test box's one GPU over gloo (RCCL
    cannot put two ranks on one device; the RCCL reducer itself is covered by test_rccl_reducer_world1).  The
    tiny SDXL-shaped UNet (--tiny): the leg under test is the bench's, not the network's, and the full SDXL
    pushes 5.1 GB of gradients per step through host memory over gloo."""
    env = dict(os.environ, OTAMD_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--res", "128", "--batch", "2", "--tiny"], capture_output=True, text=True, timeout=170, cwd=ROOT,
                       env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]       # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 4 and d["config"]["parallelism"] == "dp2"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 3
    assert "tiny" in d["config"]["model"]
    import math
    assert math.isfinite(d["loss"]) and d["loss"] > 0
    assert d["cpu_baseline"] is None                 # N > 1: no CPU leg
