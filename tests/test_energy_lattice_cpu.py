"""The lattice form of the dense energy loss without a GPU: the composed fp64 restatement tests/energy_lattice_ref.py, and the
host side of the feature (header, library, keywords, parser, a-priori key bound).  DESIGN.md section 15.3."""
import argparse
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import weclip_vit_comer_amd  # noqa: F401
from weclip_vit_comer_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_lattice_ref as LE  # noqa: E402
import energy_ref as E  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "energy_loss.npz")
TOL = 1e-5                              # tests/test_energy_ref_cpu.py's tolerance against the recorded reference
WC_ERR_ARG = 1
SYMBOLS = ("wc_energy_lattice_workspace_bytes", "wc_bilateral_filter_batch_lattice", "wc_dense_energy_fwd_lattice")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _case(gold, i):
    t = lambda k: torch.from_numpy(gold[f"c{i}_{k}"])
    return (t("img"), t("logit"), t("label"), gold[f"c{i}_box"].tolist()) + tuple(gold[f"c{i}_cfg"].tolist())


@pytest.mark.parametrize("i", range(4))
def test_composition_with_the_exact_filter_reproduces_the_fixture(gold, i):
    """The composed restatement with the exact fp64 filter in the lattice's place is the reference's recorded loss, Gate, A and
    logit gradient: the composition itself adds nothing."""
    r = LE.energy_loss(*_case(gold, i), filt=E.bilateral_filter_batch)
    t = lambda k: torch.from_numpy(gold[f"c{i}_{k}"]).double()
    e_loss = ((r["loss"] - t("loss")).abs() / t("loss").abs()).item()
    e_grad = ((r["grad_logit"] - t("grad")).abs().max() / t("grad").abs().max()).item()
    e_A = ((r["A"] - t("A")).abs().max() / t("A").abs().max()).item()
    print(f"case {i}: loss rel {e_loss:.1e}, logit gradient {e_grad:.1e}, A {e_A:.1e}")
    assert e_loss <= TOL and e_grad <= TOL and e_A <= TOL and (r["gate"] - t("gate")).abs().max().item() <= 1e-6


@pytest.mark.parametrize("i", range(4))
def test_lattice_loss_is_finite_negative_and_another_number(gold, i):
    """Pins nothing numerically: the switch switches.  (The lattice AS is about half the exact one)"""
    lat = LE.energy_loss(*_case(gold, i))
    exact = LE.energy_loss(*_case(gold, i), filt=E.bilateral_filter_batch)
    ratio = (lat["loss"] / exact["loss"]).item()
    print(f"case {i}: lattice loss / exact loss = {ratio:.3f}")
    assert torch.isfinite(lat["loss"]).all().item() and lat["loss"].item() < 0
    assert torch.isfinite(lat["grad_logit"]).all().item() and lat["grad_logit"].abs().max().item() > 0
    assert abs(ratio - 1.0) > 1e-3


def test_lattice_restatement_zero_roi():
    g = torch.Generator().manual_seed(0)
    img = torch.rand(2, 3, 9, 7, generator=g) * 255
    P = torch.softmax(torch.randn(2, 4, 9, 7, generator=g, dtype=torch.float64), 1)
    r = LE.energy_function(img, P, 15.0, 20.0, torch.zeros(2, 9, 7), torch.rand(2, 9, 7, generator=g) > 0.8)
    assert r["loss"].item() == 0 and r["grad"].abs().max().item() == 0


def test_restatement_filter_is_the_per_image_lattice():
    """lattice_filter_batch is dcrf_lattice_ref's build + filter of every image on its own, and counts its vertices."""
    import dcrf_lattice_ref as LR
    g = torch.Generator().manual_seed(1)
    img = torch.rand(2, 3, 6, 5, generator=g) * 255
    seg = torch.randn(2, 3, 6, 5, generator=g)
    counts = []
    AS, scale = LE.lattice_filter_batch(img, seg, 15.0, 4.0, want_abs=True, counts=counts)
    for n in range(2):
        lat = LR.build(img[n].permute(1, 2, 0).contiguous(), 6, 5, 4.0, 15.0)
        assert counts[n] == lat.M
        assert np.array_equal(AS[n].numpy(), LR.filter_planes(lat, seg[n]))
    assert (scale >= AS.abs() - 1e-12).all().item()
    over = img.clone()
    over[0, 1] += 300.0                                          # colours outside [0, 256] are clamped, as the kernels clamp them
    assert torch.equal(LE.lattice_filter_batch(over, seg, 15.0, 4.0), LE.lattice_filter_batch(over.clamp(0, 256), seg, 15.0, 4.0))


# ---------------------------------------------------------------------------------------------- host side of the feature
def test_header_declares_the_entries_and_the_library_has_them():
    names = {n for n, _, _ in _lib.parse_header()}
    assert set(SYMBOLS) <= names
    lib = _lib.lib()
    for s in SYMBOLS:
        assert callable(getattr(lib, s))


def test_bilateral_keyword_and_value_errors():
    from weclip_vit_comer_amd.utils import losses as LS
    assert inspect.signature(LS.bilateral_filter_batch).parameters["bilateral"].default == "exact"
    assert inspect.signature(LS.DenseEnergyLoss.__init__).parameters["bilateral"].default == "exact"
    assert LS.DenseEnergyLoss(1e-7, 15, 100, 0.5).bilateral == "exact"
    assert LS.DenseEnergyLoss(1e-7, 15, 100, 0.5, bilateral="lattice").bilateral == "lattice"
    img, seg = torch.zeros(1, 3, 4, 5), torch.zeros(1, 2, 4, 5)
    roi, unl = torch.ones(1, 4, 5), torch.zeros(1, 4, 5, dtype=torch.bool)
    layer = LS.DenseEnergyLoss(1e-7, 15, 100, 0.5)
    layer.bilateral = "nope"
    for call in (lambda: LS.DenseEnergyLoss(1e-7, 15, 100, 0.5, bilateral="nope"),
                 lambda: LS.bilateral_filter_batch(img, seg, 15, 100, bilateral="nope"),
                 lambda: LS.DenseEnergyLossFunction.apply(img, seg, 15, 100, roi, unl, "nope"),
                 lambda: LS.dense_energy_forward(img, seg, 15, 100, roi, unl, bilateral="nope"),
                 lambda: LS.get_energy_loss_fused(img, seg, torch.zeros(1, 4, 5, dtype=torch.long), None, layer),
                 lambda: LS.energy_term(img, seg, torch.zeros(1, 4, 5, dtype=torch.long), None, 1e-7, 15, 100, 0.5, [0.0] * 3, [1.0] * 3,
                                        bilateral="Lattice")):
        with pytest.raises(ValueError, match="bilateral"):
            call()


def test_extra_repr():
    from weclip_vit_comer_amd.utils.losses import DenseEnergyLoss
    assert DenseEnergyLoss(1e-7, 15, 100, 0.5).extra_repr() == "sigma_rgb=15, sigma_xy=100, weight=1e-07, scale_factor=0.5"
    assert repr(DenseEnergyLoss(1e-7, 15, 100, 0.5, "exact")) == repr(DenseEnergyLoss(1e-7, 15, 100, 0.5))
    assert DenseEnergyLoss(1e-7, 15, 100, 0.5, "lattice").extra_repr() == ("sigma_rgb=15, sigma_xy=100, weight=1e-07, scale_factor=0.5, "
                                                                           "bilateral=lattice")


def test_reg_settings_and_parser():
    from weclip_vit_comer_amd import train as T
    cfg = argparse.Namespace(train=argparse.Namespace(cam_iters=2000))
    p = T.build_parser()
    assert p.parse_args(["--config", "c.yaml"]).reg_bilateral == "exact"
    assert T.reg_settings(cfg, p.parse_args(["--config", "c.yaml"])) is None
    plain = T.reg_settings(cfg, p.parse_args(["--config", "c.yaml", "--reg_loss"]))
    assert plain == {"coef": 0.01, "scale_factor": 0.5, "start_iter": 2000}                      # what it was before the flag existed
    assert T.reg_settings(cfg, p.parse_args(["--config", "c.yaml", "--reg_loss", "--reg_bilateral", "exact"])) == plain
    assert T.reg_settings(cfg, p.parse_args(["--config", "c.yaml", "--reg_loss", "--reg_bilateral", "lattice"])) == dict(plain, bilateral="lattice")
    with pytest.raises(SystemExit):
        p.parse_args(["--config", "c.yaml", "--reg_bilateral", "nope"])


def test_reg_term_carries_the_filter():
    from weclip_vit_comer_amd.train_step import RegTerm
    assert RegTerm({}).bilateral == "exact" and RegTerm({}).layer.bilateral == "exact" and RegTerm({}).layer.workspace_cache is None
    r = RegTerm({"bilateral": "lattice", "coef": 0.5})
    assert r.bilateral == "lattice" and r.layer.bilateral == "lattice" and r.layer.workspace_cache == {}
    with pytest.raises(ValueError):
        RegTerm({"bilateral": "nope"})


def test_torch_ops_are_listed():
    from weclip_vit_comer_amd import torch_ops
    assert {"dense_energy_lattice", "energy_term_lattice"} <= set(torch_ops.OPS)
    same = lambda a, b: [(x.name, str(x.type)) for x in a._schema.arguments] == [(x.name, str(x.type)) for x in b._schema.arguments]
    assert same(torch.ops.weclip.dense_energy_lattice.default, torch.ops.weclip.dense_energy.default)
    assert same(torch.ops.weclip.energy_term_lattice.default, torch.ops.weclip.energy_term.default)


def test_key_bound_admits_the_lineage_parameters_at_every_scale():
    """(sigma_xy * s, sigma_rgb) = (100 s, 15), s in {1, 1/2, 1/4}, up to 640 x 640 scaled pixels: computed, not assumed."""
    so = ctypes.CDLL(_lib.LIB_PATH)
    fn = so.wc_dcrf_lattice_key_bound
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_double)]
    b = ctypes.c_double(-1.0)
    for s in (1.0, 0.5, 0.25):
        for H, W in ((640, 640), (512, 512), (320, 320), (256, 256), (37, 53)):
            assert fn(H, W, 100.0 * s, 15.0, ctypes.byref(b)) == 0, (s, H, W, b.value)
            print(f"s={s} {H}x{W}: key bound {b.value:.1f}")
            assert 20 < b.value <= 2047
    assert fn(640, 640, 0.25, 15.0, ctypes.byref(b)) == WC_ERR_ARG and b.value > 2047
