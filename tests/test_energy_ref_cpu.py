"""The fp64 restatement of the dense energy loss (tests/energy_ref.py) against the reference's own classes, as recorded in
tests/golden/energy_loss.npz (tests/golden/make_energy_golden.py: the reference's get_energy_loss / DenseEnergyLoss /
DenseEnergyLossFunction on the CPU with an exact filter assigned to the name its missing extension would provide).

Tolerance 1e-5 on the loss (relative) and on the logit gradient (of its largest entry), as the issue sets it: eight times the
worst residue of its three cases (1.3e-6 on the logit gradient) and four times the worst of the four recorded here (2.5e-6, the
ramp case).  The residue is the reference's own f32 arithmetic; the rest is room for another BLAS."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_ref as E  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "energy_loss.npz")
TOL = 1e-5
N_CASES = 4


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("i", range(N_CASES))
def test_restatement_matches_the_reference(gold, i):
    t = lambda k: torch.from_numpy(gold[f"c{i}_{k}"])
    weight, srgb, sxy, s = gold[f"c{i}_cfg"].tolist()
    r = E.energy_loss(t("img"), t("logit"), t("label"), gold[f"c{i}_box"].tolist(), weight, srgb, sxy, s)
    loss, grad, gate, A = t("loss").double(), t("grad").double(), t("gate").double(), t("A").double()
    e_loss = ((r["loss"] - loss).abs() / loss.abs()).item()
    e_grad = ((r["grad_logit"] - grad).abs().max() / grad.abs().max()).item()
    e_gate = (r["gate"] - gate).abs().max().item()
    e_A = ((r["A"] - A).abs().max() / A.abs().max()).item()
    print(f"case {i}: loss rel {e_loss:.1e}, logit gradient {e_grad:.1e} of its largest entry, gate abs {e_gate:.1e}, A {e_A:.1e}")
    assert loss.item() < 0 and grad.abs().max().item() > 0
    assert e_loss <= TOL and e_grad <= TOL
    # the Gate is in [0, 1] and the recorded one is the reference's f32 arithmetic on f32 probabilities: a few 2^-24
    assert e_gate <= 1e-6 and e_A <= TOL


def test_fixture_covers_what_it_should(gold):
    """A 255 patch that survives the scaling, a box strictly inside the image, a case at scale 1, and a smooth image."""
    for i in range(N_CASES):
        assert (gold[f"c{i}_label"] == 255).any() and (gold[f"c{i}_gate"] == 1).any()
        assert (gold[f"c{i}_gate"] == 0).any()                      # outside the box: ROI - max P < 0
    assert gold["c2_cfg"][3] == 1.0 and gold["c0_cfg"][3] == 0.5
    img = gold["c3_img"]
    assert np.abs(np.diff(img, axis=3)).max() < 0.2                  # the ramp: neighbours differ by a few grey levels


def test_function_gradient_is_the_reference_formula():
    """Documents the remark of DESIGN.md section 15 on tests/energy_ref.py alone (it runs no package code and pins nothing in
    it; the device gradient is compared with this restatement in tests/test_energy_gpu.py): grad = -2 A ROI / N with the
    Gate held constant is not the derivative of the loss, even with the Gate frozen, wherever the Gate is not flat."""
    g = torch.Generator().manual_seed(0)
    img = torch.rand(2, 3, 6, 7, generator=g) * 255
    P = torch.softmax(torch.randn(2, 4, 6, 7, generator=g, dtype=torch.float64), 1)
    roi = (torch.rand(2, 6, 7, generator=g) > 0.3).double()
    unl = torch.rand(2, 6, 7, generator=g) > 0.8
    r = E.energy_function(img, P, 15.0, 3.0, roi, unl)
    # with the Gate frozen the true derivative of -(1/N) sum S G AS is -(1/N) ROI (G AS + AS(G S)); the reference writes 2 G AS
    Pv = P.clone().requires_grad_(True)
    S = Pv * roi[:, None]
    AS = E.bilateral_filter_batch(img, S, 15.0, 3.0)
    (-(S * r["gate"][:, None] * AS).sum() / 2).backward()
    sym = -(roi[:, None] * (r["A"] + E.bilateral_filter_batch(img, r["gate"][:, None] * r["S"], 15.0, 3.0))) / 2
    assert torch.allclose(Pv.grad, sym, rtol=1e-10, atol=1e-12)
    assert torch.equal(r["grad"], -2.0 * r["A"] * roi[:, None] / 2)
    assert not torch.allclose(r["grad"], Pv.grad, rtol=1e-3)         # they differ wherever the Gate is not flat
