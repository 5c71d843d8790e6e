"""bench.py's command line: a plain run times --steps steps and prints only the headline line, --dump-outputs writes what the
last timed step computed, --full adds the other measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("sustained", "roofline", "cpu_baseline", "text2embedding", "bulk_assign", "gru_resident", "shipped_config", "train_iter")


def _bench(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    return r


def _line(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_steps_below_one_are_refused():
    r = _bench("--gpus", "1", "--steps", "0", "--warmup", "1", timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    outs = []
    for k in range(2):
        d = str(tmp_path / f"out{k}")
        line = _line(_bench("--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", d))
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == 3 and line["warmup"] == 2 and line["unit"] == "chunks/s" and line["dtype"] == "f32"
        assert abs(line["value"] - 4096 * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
        assert not [key for key in FULL_ONLY if key in line], "a plain run measures only the headline figure"
        assert line["config"]["dp_diag"] is None
        a = _load(d)
        assert sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
        assert all(v.dtype in (np.float32, np.float64) for v in a.values())
        assert abs(float(a["loss"][0]) - line["config"]["final_loss"]) <= 1e-6 * abs(line["config"]["final_loss"]) + 1e-6
        idx = a["code_indices"]
        assert idx.shape == (4096,) and np.array_equal(idx, np.round(idx)) and idx.min() >= 0 and idx.max() < 512
        rows = a["reconstruction_rows"]
        assert rows.shape == (1024,) and np.all(np.diff(rows) > 0) and rows[-1] < 4096
        assert a["reconstruction"].shape == (1024, 34, 135) and np.isfinite(a["reconstruction"]).all()
        assert a["state.vq_layer._embedding.weight"].shape == (512, 128)
        assert a["custom_loss_terms"].shape == (5,) and a["perplexity"].shape == (1,)
        outs.append(a)
    # same arguments, same inputs: the two runs compute the same step
    assert sorted(outs[0]) == sorted(outs[1])
    assert np.array_equal(outs[0]["reconstruction_rows"], outs[1]["reconstruction_rows"])
    assert np.mean(outs[0]["code_indices"] == outs[1]["code_indices"]) >= 0.99
    for name in outs[0]:
        if name != "code_indices":
            np.testing.assert_allclose(outs[0][name], outs[1][name], rtol=1e-4, atol=1e-6, err_msg=name)


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements():
    line = _line(_bench("--gpus", "1", "--steps", "3", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-part-d",
                        "--sustained", "5"))
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["sustained"]["steps"] == 5
    assert line["roofline"]["avg_us"] > 0 and "whole_step" in line["roofline"]
    assert "cpu_baseline" not in line and "text2embedding" not in line
