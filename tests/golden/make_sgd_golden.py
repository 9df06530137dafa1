"""Writes tests/golden/sgd_schedule.npz: the reference's own `PolyWarmupSGD` (utils/optimizer.py:35-65), unmodified, run on CPU.

    python tests/golden/make_sgd_golden.py

Build-container only (needs the reference checkout that oracle/refharness.py points at).  Cases and inputs are those of
tests/sgd_ref.py:
  lr_w<warmup>_p<power> (max_iter + 3, 2) f64: the lr of both groups after the schedule of steps s = 0 .. max_iter + 2, for
      warmup_iter in {0, 3}, max_iter = 40, power in {1.0, 0.9};
  traj_p<group>, traj_buf<group> (6, n) f32: parameters and momentum buffers after each of six steps across the warm-up
      boundary, from the seeded start values and gradients of sgd_ref.traj_inputs().
Recorded numbers only: nothing of the reference's code is stored."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refharness  # noqa: E402
from tests import sgd_ref as S  # noqa: E402


def reference_class():
    """The reference's class from its own file (the file imports torch only; loaded under a private name, so that neither
    `utils` package is touched)."""
    if not refharness.available():
        raise SystemExit("the reference checkout is not present")
    spec = importlib.util.spec_from_file_location("_ref_optimizer", os.path.join(refharness.REF, "utils", "optimizer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PolyWarmupSGD


def main():
    cls = reference_class()
    out = {}
    for w in S.SCHED_WARMUP:
        for power in S.SCHED_POWER:
            out[S.sched_key(w, power)] = np.asarray(S.run_schedule(cls, w, power), dtype=np.float64)
    traj = S.run_trajectory(cls)
    for gi in range(2):
        out[f"traj_p{gi}"] = torch.stack([t[gi] for t in traj]).numpy()
        out[f"traj_buf{gi}"] = torch.stack([t[2 + gi] for t in traj]).numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sgd_schedule.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
