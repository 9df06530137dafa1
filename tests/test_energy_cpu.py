"""Dense energy loss without a GPU: the three names of the reference's utils/losses.py import (directly and through the
drop-in), the module prints as the reference's does, calls fail loudly, and every C-ABI limit is rejected before a launch."""
import ctypes
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import weclip_vit_comer_amd  # noqa: F401
from weclip_vit_comer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WC_ERR_ARG = 1


def test_names_import_from_the_package():
    from weclip_vit_comer_amd.utils.losses import DenseEnergyLoss, DenseEnergyLossFunction, get_energy_loss
    assert issubclass(DenseEnergyLoss, torch.nn.Module) and issubclass(DenseEnergyLossFunction, torch.autograd.Function)
    assert callable(get_energy_loss)


def test_the_training_scripts_import_line_resolves_through_the_dropin(tmp_path):
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import weclip_vit_comer_amd
        weclip_vit_comer_amd.install_dropin()
        from utils.losses import DenseEnergyLoss, get_aff_loss, get_energy_loss
        from utils.losses import DenseEnergyLossFunction
        assert DenseEnergyLoss.__module__ == "weclip_vit_comer_amd.utils.losses", DenseEnergyLoss.__module__
        print("ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr


def test_repr_has_the_reference_format():
    from weclip_vit_comer_amd.utils.losses import DenseEnergyLoss
    assert repr(DenseEnergyLoss(1e-7, 15, 100, 0.5)) == "DenseEnergyLoss(sigma_rgb=15, sigma_xy=100, weight=1e-07, scale_factor=0.5)"


def test_calls_without_a_gpu_raise():
    from weclip_vit_comer_amd.utils import losses
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    img, P = torch.zeros(1, 3, 4, 6), torch.full((1, 2, 4, 6), 0.5)
    roi, unl = torch.ones(1, 4, 6), torch.zeros(1, 4, 6, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.DenseEnergyLossFunction.apply(img, P, 15.0, 100.0, roi, unl)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.bilateral_filter_batch(img, P, 15.0, 100.0)
    layer = losses.DenseEnergyLoss(1e-7, 15, 100, 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        layer(img, P, roi, torch.zeros(1, 1, 4, 6, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        losses.get_energy_loss(img, torch.zeros(1, 2, 4, 6), torch.zeros(1, 4, 6, dtype=torch.long), [[0, 4, 0, 6]], layer)
    weclip_vit_comer_amd.register_torch_ops()
    with pytest.raises(NotImplementedError):          # no CPU backend: the dispatcher refuses, nothing falls back
        torch.ops.weclip.dense_energy(img, P, roi, unl, 15.0, 100.0)
    with pytest.raises(NotImplementedError):
        torch.ops.weclip.bilateral_filter_batch(img, P, 15.0, 100.0)


def test_fake_kernels_propagate_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    weclip_vit_comer_amd.register_torch_ops()
    with FakeTensorMode():
        img, P = torch.empty(2, 3, 8, 6, device="cuda"), torch.empty(2, 5, 8, 6, device="cuda")
        roi, unl = torch.empty(2, 8, 6, device="cuda"), torch.empty(2, 8, 6, device="cuda", dtype=torch.bool)
        loss, A = torch.ops.weclip.dense_energy(img, P, roi, unl, 15.0, 50.0)
        assert tuple(loss.shape) == (1,) and tuple(A.shape) == (2, 5, 8, 6) and loss.dtype == A.dtype == torch.float32
        assert tuple(torch.ops.weclip.dense_energy_bwd(loss, A, roi).shape) == (2, 5, 8, 6)
        assert tuple(torch.ops.weclip.bilateral_filter_batch(img, P, 15.0, 50.0).shape) == (2, 5, 8, 6)


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, _, args in _lib.parse_header():
        if "energy" in name or "bilateral" in name:
            getattr(so, name).argtypes = [t for t, _ in args]
    return so


P = ctypes.c_void_p(256)           # never dereferenced: every call below is rejected before any launch

BAD_DIMS = [dict(N=0), dict(N=-1), dict(N=65536), dict(K=0), dict(K=129), dict(H=0), dict(W=0), dict(H=641, W=640), dict(H=409601, W=1)]
BAD_SIGMAS = [dict(srgb=0.0), dict(sxy=-1.0), dict(srgb=float("nan")), dict(sxy=float("inf"))]


def _args(**kw):
    a = dict(N=2, K=21, H=8, W=8, srgb=15.0, sxy=50.0)
    a.update(kw)
    return a


@pytest.mark.parametrize("kw", BAD_DIMS + BAD_SIGMAS + [dict(null=i) for i in range(8)])
def test_forward_limits(so, kw):
    a = _args(**{k: v for k, v in kw.items() if k != "null"})
    p = [P] * 8
    if "null" in kw:
        p[kw["null"]] = None
    assert so.wc_dense_energy_fwd(*p, a["N"], a["K"], a["H"], a["W"], a["srgb"], a["sxy"], None) == WC_ERR_ARG


@pytest.mark.parametrize("kw", BAD_DIMS + BAD_SIGMAS + [dict(null=i) for i in range(4)])
def test_filter_limits(so, kw):
    a = _args(**{k: v for k, v in kw.items() if k != "null"})
    p = [P] * 4
    if "null" in kw:
        p[kw["null"]] = None
    assert so.wc_bilateral_filter_batch(*p, a["N"], a["K"], a["H"], a["W"], a["srgb"], a["sxy"], None) == WC_ERR_ARG


@pytest.mark.parametrize("kw", BAD_DIMS + [dict(null=i) for i in range(4)])
def test_backward_limits(so, kw):
    a = _args(**{k: v for k, v in kw.items() if k != "null"})
    p = [P] * 4
    if "null" in kw:
        p[kw["null"]] = None
    assert so.wc_dense_energy_bwd(*p, a["N"], a["K"], a["H"], a["W"], None) == WC_ERR_ARG


def test_workspace_size_and_error_text(so):
    n = ctypes.c_long(-7)
    assert so.wc_energy_workspace_floats(2, 200, 8, 8, ctypes.byref(n)) == WC_ERR_ARG and n.value == -7
    assert so.wc_energy_workspace_floats(2, 21, 8, 8, None) == WC_ERR_ARG
    assert so.wc_energy_workspace_floats(2, 21, 8, 8, ctypes.byref(n)) == 0 and n.value == 2 * (64 * (8 + 32) + 1)
    assert so.wc_energy_workspace_floats(3, 33, 13, 11, ctypes.byref(n)) == 0 and n.value == 3 * (143 * (8 + 64) + 2)
    lib = _lib.lib()
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.wc_dense_energy_fwd(P, P, P, P, P, P, P, P, 2, 0, 8, 8, 15.0, 50.0, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.wc_bilateral_filter_batch(P, P, P, P, 2, 21, 8, 8, 0.0, 50.0, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.wc_dense_energy_bwd(P, None, P, P, 2, 21, 8, 8, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.wc_energy_workspace_floats(0, 21, 8, 8, ctypes.byref(n))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_energy_kernels_issue_their_loads_together(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_scan
    rows = isa_scan.report([os.path.join(ROOT, "weclip-vit-comer_amd", "csrc", "energy.hip")], threshold=4, out_dir=str(tmp_path))
    bad = [(alone, loads, name) for alone, loads, _, name, _ in rows]
    assert not bad, "loads waited for one at a time (see tools/isa_scan.py): %s" % bad
