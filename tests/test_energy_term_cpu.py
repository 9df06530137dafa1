"""The dense energy loss as a step term, without a GPU: every host-side check of get_energy_loss_fused fires before the library is
touched, the C ABI rejects its limits before a launch, the stock f32 torch chain itself meets the P_s bound that
tests/test_energy_term_gpu.py holds the kernel to, the training entry point's new arguments parse and leave the record alone
without --reg_loss, and csrc/energy_prep.hip passes the serialised-load scan."""
import argparse
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import weclip_vit_comer_amd  # noqa: F401
from weclip_vit_comer_amd import _lib
from weclip_vit_comer_amd import train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_term_ref as R  # noqa: E402

WC_ERR_ARG = 1


def _ok():
    from weclip_vit_comer_amd.utils.losses import DenseEnergyLoss
    return dict(img=torch.zeros(2, 3, 8, 12), seg=torch.zeros(2, 5, 2, 3), label=torch.zeros(2, 8, 12, dtype=torch.long),
                box=[[0, 8, 0, 12], [1, 2, 3, 4]], layer=DenseEnergyLoss(1e-7, 15, 100, 0.5))


class _NoFields:
    pass


BAD = [
    ("img", lambda a: a.update(img=[1, 2]), TypeError),
    ("img", lambda a: a.update(img=torch.zeros(2, 1, 8, 12)), ValueError),
    ("img", lambda a: a.update(img=torch.zeros(2, 3, 8, 12, dtype=torch.uint8)), TypeError),
    ("seg_lowres", lambda a: a.update(seg=torch.zeros(2, 5, 6)), ValueError),
    ("seg_lowres", lambda a: a.update(seg=torch.zeros(2, 5, 2, 3, dtype=torch.long)), TypeError),
    ("label", lambda a: a.update(label=torch.zeros(2, 1, 8, 12, dtype=torch.long)), ValueError),
    ("label", lambda a: a.update(label=torch.zeros(2, 8, 12)), TypeError),
    ("label", lambda a: a.update(label=torch.zeros(2, 8, 12, dtype=torch.bool)), TypeError),
    ("batch", lambda a: a.update(seg=torch.zeros(3, 5, 2, 3)), ValueError),
    ("differ in size", lambda a: a.update(label=torch.zeros(2, 8, 11, dtype=torch.long)), ValueError),
    ("K", lambda a: a.update(seg=torch.zeros(2, 129, 2, 3)), ValueError),
    ("empty", lambda a: a.update(seg=torch.zeros(2, 5, 0, 3)), ValueError),
    ("scale_factor", lambda a: setattr(a["layer"], "scale_factor", 0.3), ValueError),
    ("scale_factor", lambda a: setattr(a["layer"], "scale_factor", 2.0), ValueError),
    ("scaled size", lambda a: (a.update(img=torch.zeros(2, 3, 1, 12), label=torch.zeros(2, 1, 12, dtype=torch.long))), ValueError),
    ("W <= 8192", lambda a: (a.update(img=torch.zeros(2, 3, 2, 8194), label=torch.zeros(2, 2, 8194, dtype=torch.long))), ValueError),
    ("sigmas", lambda a: setattr(a["layer"], "sigma_rgb", 0), ValueError),
    ("weight", lambda a: setattr(a["layer"], "weight", "1e-7"), TypeError),
    ("loss_layer", lambda a: a.update(layer=_NoFields()), TypeError),
    ("img_box", lambda a: a.update(box=[[0, 8, 0, 12]]), ValueError),
    ("img_box", lambda a: a.update(box=[[0, 8, 0], [1, 2, 3]]), ValueError),
    ("img_box", lambda a: a.update(box=torch.zeros(2, 4)), TypeError),
    ("img_box", lambda a: a.update(box=torch.zeros(2, 5, dtype=torch.int32)), ValueError),
    ("img_box", lambda a: a.update(box=7), TypeError),
    ("mean", lambda a: a.update(mean=[1.0, 2.0]), ValueError),
]


@pytest.mark.parametrize("what,edit,exc", BAD, ids=[f"{i}-{b[0].replace(' ', '_')}" for i, b in enumerate(BAD)])
def test_host_checks_fire_before_the_library_is_touched(monkeypatch, what, edit, exc):
    from weclip_vit_comer_amd.utils import losses

    def touched(*a, **k):
        raise AssertionError("the library was touched before the host-side check")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "require_gpu", touched)
    a = _ok()
    edit(a)
    kw = {"mean": a["mean"]} if "mean" in a else {}
    with pytest.raises(exc, match=what):
        losses.get_energy_loss_fused(a["img"], a["seg"], a["label"], a["box"], a["layer"], **kw)


def test_valid_cpu_inputs_reach_the_gpu_requirement():
    from weclip_vit_comer_amd.utils import losses
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    a = _ok()
    for box in (a["box"], None, torch.tensor(a["box"], dtype=torch.int16)):
        with pytest.raises(RuntimeError, match="GPU"):
            losses.get_energy_loss_fused(a["img"], a["seg"], a["label"], box, a["layer"])
    weclip_vit_comer_amd.register_torch_ops()
    with pytest.raises(NotImplementedError):          # no CPU backend: the dispatcher refuses, nothing falls back
        torch.ops.weclip.energy_term(a["img"], a["seg"], a["label"], None, 1e-7, 15.0, 100.0, 0.5, list(R.MEAN), list(R.STD))


def test_fake_kernel_propagates_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    weclip_vit_comer_amd.register_torch_ops()
    assert "energy_term" in weclip_vit_comer_amd.torch_ops.OPS
    with FakeTensorMode():
        img, seg = torch.empty(2, 3, 8, 12, device="cuda"), torch.empty(2, 5, 2, 3, device="cuda")
        lab, box = torch.empty(2, 8, 12, device="cuda", dtype=torch.long), torch.empty(2, 4, device="cuda", dtype=torch.int32)
        loss, grad = torch.ops.weclip.energy_term(img, seg, lab, box, 1e-7, 15.0, 100.0, 0.5, list(R.MEAN), list(R.STD))
        assert tuple(loss.shape) == (1,) and tuple(grad.shape) == (2, 5, 2, 3) and loss.dtype == grad.dtype == torch.float32


def test_reg_term_settings():
    from weclip_vit_comer_amd.train_step import RegTerm
    assert RegTerm.of(None) is None
    r = RegTerm.of({})
    assert (r.coef, r.weight, r.sigma_rgb, r.sigma_xy, r.scale_factor, r.start_iter) == (0.01, 1e-7, 15, 100, 0.5, 0)
    assert repr(r.layer) == "DenseEnergyLoss(sigma_rgb=15, sigma_xy=100, weight=1e-07, scale_factor=0.5)"
    r = RegTerm.of(argparse.Namespace(coef=0.5, start_iter=2))
    assert r.coef == 0.5 and [r.begin_step() for _ in range(4)] == [False, False, True, True]
    with pytest.raises(ValueError, match="scale_factor"):
        RegTerm.of({"scale_factor": 0.3})
    with pytest.raises(ValueError, match="unknown"):
        RegTerm.of({"coeff": 1.0})


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, _, args in _lib.parse_header():
        if "energy_prep" in name:
            getattr(so, name).argtypes = [t for t, _ in args]
    return so


def test_symbols_are_in_the_header_and_in_the_library(so):
    declared = {name for name, _, _ in _lib.parse_header()}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in ("wc_energy_prep_fwd", "wc_energy_prep_bwd", "wc_energy_prep_workspace_floats"):
        assert name in declared and name in exported, name


P = ctypes.c_void_p(256)           # never dereferenced: every call below is rejected before any launch
HOST3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
# N, K, h, w, H, W, e
BAD_DIMS = [dict(K=0), dict(K=129), dict(e=-1), dict(e=3), dict(H=1, e=1), dict(W=3, e=2), dict(H=0), dict(h=0), dict(w=0), dict(N=0),
            dict(N=65536), dict(N=16384, K=128), dict(H=641, W=640, e=0), dict(H=1282, W=1280, e=1), dict(H=2564, W=2560, e=2), dict(H=4, W=8193, e=0)]


def _dims(kw):
    a = dict(N=2, K=21, h=2, w=3, H=8, W=12, e=1)
    a.update({k: v for k, v in kw.items() if k != "null"})
    return [a[k] for k in ("N", "K", "h", "w", "H", "W", "e")]


@pytest.mark.parametrize("kw", BAD_DIMS + [dict(null=i) for i in (0, 1, 2, 4, 5, 6, 7, 8, 9)])
def test_prep_forward_limits(so, kw):
    p = [P, P, P, P, HOST3, HOST3, P, P, P, P]
    if "null" in kw:
        p[kw["null"]] = None
    assert so.wc_energy_prep_fwd(*p, *_dims(kw), None) == WC_ERR_ARG


def test_prep_forward_refuses_a_misaligned_box(so):
    assert so.wc_energy_prep_fwd(P, P, P, ctypes.c_void_p(260), HOST3, HOST3, P, P, P, P, *_dims({}), None) == WC_ERR_ARG


@pytest.mark.parametrize("kw", BAD_DIMS + [dict(null=i) for i in range(5)] + [dict(coef=float("nan")), dict(coef=float("inf"))])
def test_prep_backward_limits(so, kw):
    p = [P] * 5
    if "null" in kw:
        p[kw["null"]] = None
    coef = kw.get("coef", -1e-7)
    assert so.wc_energy_prep_bwd(*p, coef, *_dims({k: v for k, v in kw.items() if k != "coef"}), None) == WC_ERR_ARG


def test_workspace_size_and_error_text(so):
    n = ctypes.c_long(-7)
    assert so.wc_energy_prep_workspace_floats(2, 200, 4, 96, ctypes.byref(n)) == WC_ERR_ARG and n.value == -7
    assert so.wc_energy_prep_workspace_floats(2, 21, 4, 96, None) == WC_ERR_ARG
    assert so.wc_energy_prep_workspace_floats(2, 21, 4, 96, ctypes.byref(n)) == 0 and n.value == 2 * 2 * 21 * 4 * 96
    lib = _lib.lib()
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.wc_energy_prep_fwd(P, P, P, None, HOST3, HOST3, P, P, P, P, 2, 21, 2, 3, 8, 12, 3, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.wc_energy_prep_bwd(P, P, P, P, None, -1e-7, 2, 21, 2, 3, 8, 12, 1, None)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_prep_kernels_issue_their_loads_together(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_scan
    rows = isa_scan.report([os.path.join(ROOT, "weclip-vit-comer_amd", "csrc", "energy_prep.hip")], threshold=4, out_dir=str(tmp_path))
    bad = [(alone, loads, name) for alone, loads, _, name, _ in rows]
    assert not bad, "loads waited for one at a time (see tools/isa_scan.py): %s" % bad


# ------------------------------------------------------------------------------------------------ the bound of the GPU test
@pytest.mark.parametrize("e", R.ES)
@pytest.mark.parametrize("si", range(len(R.SHAPES)))
def test_the_stock_f32_chain_meets_the_P_bound(si, e):
    """|P - P64| <= (16 M + K + 16) 2^-24 is derived from the roundings of the chain, not from the kernel: the stock f32 torch
    ops, which take the same route, stay inside it on the inputs of the GPU test (and on the magnitude-30 case)."""
    hw, HW = R.SHAPES[si]
    s = 2.0 ** -e
    worst = 0.0
    for K, N, mag in [(K, 3, 3.0) for K in R.KS] + [(21, 1, 30.0)]:
        img, seg, lab, box = R.make_case(hw, HW, K, N, R.case_seed(si, e, K, N), mag)
        P64 = R.prep_forward(img, seg, lab, box, s, R.F64)[1]
        P32 = R.prep_forward(img, seg, lab, box, s, torch.float32)[1]
        ratio = R.worst_p_ratio(P32, P64, seg, HW, K)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (hw, HW, e, K, mag, ratio)
    print(f"{hw}->{HW} e={e}: stock f32 chain, worst |P - P64| / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ the training entry point
def test_new_arguments_parse_and_default_off():
    d = T.build_parser().parse_args(["--config", "c.yaml"])
    assert d.reg_loss is False and d.reg_coef == 0.01 and d.reg_scale == 0.5 and d.reg_start is None
    cfg = T.Config(train=T.Config(cam_iters=2000))
    assert T.reg_settings(cfg, d) is None
    a = T.build_parser().parse_args(["--config", "c.yaml", "--reg_loss"])
    assert T.reg_settings(cfg, a) == {"coef": 0.01, "scale_factor": 0.5, "start_iter": 2000}
    b = T.build_parser().parse_args(["--config", "c.yaml", "--reg_loss", "--reg_coef", "0.1", "--reg_scale", "0.25", "--reg_start", "0"])
    assert T.reg_settings(cfg, b) == {"coef": 0.1, "scale_factor": 0.25, "start_iter": 0}
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--config", "c.yaml", "--reg_scale", "0.3"])


def test_record_and_log_line_gain_reg_loss_only_with_the_flag():
    rec = T.log_record(200, 2e-4, [3.0, 2.0, 1.0, 30.0, 40.0], 2)
    assert list(rec) == ["iter", "lr", "seg_loss", "attn_loss", "pseudo_seg_mAcc"]
    assert rec == {"iter": 200, "lr": 2e-4, "seg_loss": 1.0, "attn_loss": 0.5, "pseudo_seg_mAcc": 0.75}
    reg = T.log_record(200, 2e-4, [3.0, 2.0, 1.0, 4e-6, 30.0, 40.0], 2)
    assert list(reg) == list(rec) + ["reg_loss"] and reg["reg_loss"] == 2e-6 and reg["pseudo_seg_mAcc"] == 0.75
    plain = T.format_log_line(200, "0:02:11", "5:25:19", 1.9867e-4, 0.123449, 0.98765, 0.87654)
    assert T.format_log_line(200, "0:02:11", "5:25:19", 1.9867e-4, 0.123449, 0.98765, 0.87654, None) == plain
    assert T.format_log_line(200, "0:02:11", "5:25:19", 1.9867e-4, 0.123449, 0.98765, 0.87654, 2e-6) == plain + ", reg_loss: 2.0000e-06"
