"""bench.py's result line and `--dump-outputs`: two runs with the same arguments write the same arrays, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(dump_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--global-batch", "64", "--no-dense-compare", "--no-cpu-baseline", "--dump-outputs", str(dump_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-len(".npy")]: np.load(os.path.join(dump_dir, f)) for f in os.listdir(dump_dir)}


@pytest.mark.gpu
def test_bench_dump_outputs_repeat(tmp_path):
    (res, a), (res2, b) = _bench(tmp_path / "a", 3), _bench(tmp_path / "b", 3)
    for r in (res, res2):
        assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert sorted(a) == sorted(b)
    assert {"loss", "image_features", "text_features", "logit_scale"} <= set(a)
    assert a["image_features"].shape == a["text_features"].shape == (64, 512)
    params = [k for k in a if k.startswith("param.")]
    assert params and all("grad." + k[len("param."):] in a for k in params)
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert abs(float(a["loss"]) - res["final_loss"]) < 1e-4
    # no float atomics on the train step: the same arguments give the same bits
    differ = [k for k in a if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]
    assert all(np.isfinite(x).all() for x in a.values())
    assert not differ, differ[:10]


def _result_line(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--global-batch", "64", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_full_adds_its_own_runs():
    """A plain run stops after the timed steps; --full adds the dense-text measurement, the instrumented step behind `roofline`
    and the CPU baseline."""
    full_only = {"dense_text_rows", "roofline", "cpu_baseline"}
    plain = _result_line()
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(plain) and plain["value"] > 0
    assert not full_only & set(plain), sorted(full_only & set(plain))
    full = _result_line("--full", "--cpu-steps", "1")
    assert full_only <= set(full), sorted(full_only - set(full))
    assert full["dense_text_rows"]["steps"] == 2 and full["dense_text_rows"]["ms_per_step"] > 0
    assert full["roofline"]["launches_per_step"] > 0 and full["roofline"]["achieved"] > 0
    assert full["cpu_baseline"]["value"] > 0
