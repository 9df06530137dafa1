"""`bench.py` without `--full` runs only what the headline needs (set-up, warm-up, one timed region, the JSON line), and
what `--dump-outputs` writes does not depend on `--full`: both write the state after `--repeats` regions of `--steps`
steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--size", "128"]
DUMPED = ("loss", "seg_loss", "attn_loss", "grads", "params")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only_and_dumps_what_a_full_run_dumps(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert d["metric"].startswith("images/sec") and d["unit"] == "images/sec" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] and d["steps"] == 2 and d["warmup"] == 1
    assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    for k in ("repeat_ms_per_step", "host_work_ms_per_step_idle_queue", "dp_check", "roofline", "cpu_baseline",
              "seg_trans_branch", "exact_precision", "fast_gemm_fp32_par", "with_comer", "encoder_only_b32"):
        assert k not in d, k

    f = _bench("--full", "--no-extras", "--no-cpu-baseline", "--roof-steps", "0", "--timer-stride", "0",
               "--dump-outputs", str(tmp_path / "full"))
    assert len(f["repeat_ms_per_step"]) == 5 and f["repeat_ms_per_step"][0] == f["ms_per_step"]
    assert f["host_work_ms_per_step_idle_queue"] > 0 and "roofline" in f
    for name in DUMPED:
        a = np.load(tmp_path / "plain" / (name + ".npy"))
        b = np.load(tmp_path / "full" / (name + ".npy"))
        np.testing.assert_array_equal(a, b, err_msg=name)
