"""tests/mmd_ref.py (the fp64 closed form the GPU tests compare against) reproduces the reference's own fp64 run, recorded in
tests/golden/mmd_rbf.npz by tests/golden/make_mmd_golden.py, and its bandwidth identity holds against the brute-force sum."""
import numpy as np
import pytest
import torch

import mmd_ref


@pytest.fixture(scope="module")
def gold(golden):
    return golden("mmd_rbf.npz")


def _names(gold):
    return [str(n) for n in gold["names"]]


def test_golden_has_every_case(gold):
    assert len(_names(gold)) == 8
    assert {n.rsplit("_", 1)[0] for n in _names(gold)} == {"B1_d1", "B2_d3", "B5_d7", "B33_d40"}


def test_restatement_reproduces_the_reference(gold):
    for name in _names(gold):
        src, tgt = torch.from_numpy(gold[f"{name}_source"]), torch.from_numpy(gold[f"{name}_target"])
        fix = float(gold[f"{name}_fix"])
        r = mmd_ref.mmd(src, tgt, 2.0, 5, fix or None, want_K=True)
        for key, got in (("loss", r["loss"]), ("K", r["K"]), ("grad_source", r["grad_source"]), ("grad_target", r["grad_target"])):
            want = torch.from_numpy(np.asarray(gold[f"{name}_{key}"]))
            err = (got - want).abs().max().item()
            assert err <= 1e-12, (name, key, err)


def test_scales_bound_the_values(gold):
    for name in _names(gold):
        src, tgt = torch.from_numpy(gold[f"{name}_source"]), torch.from_numpy(gold[f"{name}_target"])
        r = mmd_ref.mmd(src, tgt, 2.0, 5, float(gold[f"{name}_fix"]) or None)
        assert abs(r["loss"]) <= r["A"]
        assert (r["grad_source"].abs() <= r["G_source"] * (1 + 1e-12)).all() and (r["grad_target"].abs() <= r["G_target"] * (1 + 1e-12)).all()


@pytest.mark.parametrize("N,d,shift", [(2, 1, 0.0), (7, 3, 0.0), (66, 40, 100.0), (130, 9, -3.0)])
def test_bandwidth_identity(N, d, shift):
    X = torch.randn(N, d, dtype=torch.float64, generator=torch.Generator().manual_seed(N + d)) * 1.7 + shift
    a, b = mmd_ref.bandwidth_bruteforce(X).item(), mmd_ref.bandwidth_centred(X).item()
    assert abs(a - b) <= 1e-12 * abs(a)


def test_chunked_rows_equal_one_pass():
    g = torch.Generator().manual_seed(5)
    src, tgt = torch.randn(37, 11, generator=g, dtype=torch.float64), torch.randn(37, 11, generator=g, dtype=torch.float64) + 0.3
    a, b = mmd_ref.mmd(src, tgt, 1.5, 3, None, want_K=True, chunk=1024), mmd_ref.mmd(src, tgt, 1.5, 3, None, want_K=True, chunk=16)
    for k in ("loss", "A", "K", "grad_source", "grad_target", "G_source", "G_target"):
        assert (a[k] - b[k]).abs().max().item() <= 1e-13, k
