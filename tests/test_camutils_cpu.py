"""utils.camutils without a GPU: the lineage's import line resolves through the drop-in, every new function fails loudly on CPU
inputs, the registered op has no CPU backend, and every C-ABI limit is rejected before a launch."""
import ctypes
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import weclip_vit_comer_amd
from weclip_vit_comer_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camutils_cases as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WC_ERR_ARG = 1


def test_the_training_scripts_import_line_resolves_through_the_dropin(tmp_path):
    """scripts/.ipynb_checkpoints/dist_train_voc-checkpoint.py, the line after `from utils.losses import ...`."""
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import weclip_vit_comer_amd
        weclip_vit_comer_amd.install_dropin()
        from utils.camutils import (cam_to_label, cams_to_affinity_label, ignore_img_box,
                                    multi_scale_cam, multi_scale_cam_with_aff_mat,
                                    propagte_aff_cam_with_bkg, refine_cams_with_bkg_v2,
                                    refine_cams_with_cls_label)
        from utils.camutils import propagte_aff_cam
        import utils.camutils
        assert cam_to_label.__module__ == "weclip_vit_comer_amd.utils.camutils", cam_to_label.__module__
        assert not hasattr(utils.camutils, "cam_to_fg_bg_label")
        print("ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr


def test_cpu_inputs_raise():
    from weclip_vit_comer_amd.utils import camutils as M
    cfg = K.make_cfg()
    cam, cls, box = torch.rand(2, 3, 8, 12), torch.ones(2, 3), [[0, 8, 0, 12], [1, 7, 2, 9]]
    img, aff = torch.rand(2, 3, 8, 12), torch.rand(2, 6, 6)
    ref_mod = lambda i, m: m
    model = lambda x, cam_only=True: (x[:, :2], x[:, 0, :2, :2])
    calls = [lambda: M.cam_to_label(cam, cls, cfg=cfg),
             lambda: M.cam_to_label(cam, cls, img_box=box, ignore_mid=True, cfg=cfg),
             lambda: M.ignore_img_box(torch.zeros(2, 8, 12, dtype=torch.long), box, 255),
             lambda: M.propagte_aff_cam(torch.rand(2, 3, 2, 3), aff=aff),
             lambda: M.propagte_aff_cam_with_bkg(torch.rand(2, 3, 2, 3), aff=aff, cls_labels=cls, bkg_score=0.35),
             lambda: M.refine_cams_with_bkg_v2(ref_mod, img, cam, cls, cfg, box),
             lambda: M.refine_cams_with_bkg_v2(ref_mod, img, cam, cls, cfg, box, keys=[[0], [1, 2]]),
             lambda: M.refine_cams_with_cls_label(ref_mod, img, cls, cam, box),
             lambda: M.multi_scale_cam(model, img, (1.0, 0.5)),
             lambda: M.multi_scale_cam_with_aff_mat(model, img, (1.0, 0.5))]
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    # the functions kept on stock ops still run on CPU tensors
    lab = torch.zeros(1, 32, 32, dtype=torch.long)
    assert tuple(M.cams_to_affinity_label(lab, mask=M.get_mask_by_radius(2, 2, 1)).shape) == (1, 4, 4)
    weclip_vit_comer_amd.register_torch_ops()
    with pytest.raises(NotImplementedError):          # no CPU backend: the dispatcher refuses, nothing falls back
        torch.ops.weclip.aff_propagate(aff, torch.rand(2, 3, 6), None, cls, 0.35, True)


def test_fake_kernel_propagates_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    weclip_vit_comer_amd.register_torch_ops()
    with FakeTensorMode():
        aff, cams = torch.empty(2, 63, 63, device="cuda"), torch.empty(2, 5, 63, device="cuda")
        cls, mask = torch.empty(2, 5, device="cuda"), torch.empty(63, 63, device="cuda")
        o = torch.ops.weclip.aff_propagate(aff, cams, mask, cls, 0.35, True)
        assert tuple(o.shape) == (2, 6, 63) and o.dtype == torch.float32
        assert tuple(torch.ops.weclip.aff_propagate(aff, cams, None, None, 0.0, False).shape) == (2, 5, 63)


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    names = ("wc_aff_propagate", "wc_cam_to_label", "wc_box_ignore", "wc_bkg_refine", "wc_box_gather", "wc_box_scatter")
    for name, _, args in _lib.parse_header():
        if name.startswith(names):
            getattr(so, name).argtypes = [t for t, _ in args]
    return so


P = ctypes.c_void_p(256)           # never dereferenced: every call below is rejected before any launch


def _walk(so, p=None, B=2, n=63, C=5, bkg=0.35, with_bkg=1):
    p = p or [P] * 6
    return so.wc_aff_propagate(*p, B, n, C, bkg, with_bkg, None)


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=65536), dict(n=0), dict(n=4097), dict(C=128), dict(C=129, with_bkg=0), dict(C=0, with_bkg=0),
                                dict(C=-1), dict(bkg=float("nan")), dict(bkg=float("inf")), dict(with_bkg=2)])
def test_walk_limits(so, kw):
    assert _walk(so, **kw) == WC_ERR_ARG


@pytest.mark.parametrize("null", [0, 2, 3, 4, 5])
def test_walk_null_pointers(so, null):
    p = [P] * 6
    p[null] = None
    assert _walk(so, p) == WC_ERR_ARG              # (index 1, the mask, may be NULL; index 3, the labels, not with_bkg = 1)


def test_walk_workspace_size_and_error_text(so):
    n = ctypes.c_long(-7)
    assert so.wc_aff_propagate_workspace_floats(2, 63, 200, 1, ctypes.byref(n)) == WC_ERR_ARG and n.value == -7
    assert so.wc_aff_propagate_workspace_floats(2, 63, 5, 1, None) == WC_ERR_ARG
    assert so.wc_aff_propagate_workspace_floats(2, 63, 5, 1, ctypes.byref(n)) == 0 and n.value == 2 * 63 * 32
    assert so.wc_aff_propagate_workspace_floats(3, 400, 80, 1, ctypes.byref(n)) == 0 and n.value == 3 * 400 * 96
    assert so.wc_aff_propagate_workspace_floats(3, 400, 64, 0, ctypes.byref(n)) == 0 and n.value == 3 * 400 * 64
    with pytest.raises(RuntimeError, match="bad argument"):
        _lib.lib().wc_aff_propagate(P, None, P, P, P, P, 2, 5000, 5, 0.35, 1, None)


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=65536), dict(C=0), dict(H=0), dict(W=0), dict(H=4097, W=4096), dict(null=0), dict(null=1),
                                dict(null=3)])
def test_label_limits(so, kw):
    a = dict(B=2, C=3, H=8, W=12)
    a.update({k: v for k, v in kw.items() if k != "null"})
    p = [P] * 5
    if "null" in kw:
        p[kw["null"]] = None
    assert so.wc_cam_to_label(*p, a["B"], a["C"], a["H"], a["W"], 0.45, 0.55, 0.35, 1, 255, None) == WC_ERR_ARG
    if kw.get("null", 0) != 3 and "C" not in kw:
        q = [P] * 3
        if "null" in kw:
            q[kw["null"]] = None
        assert so.wc_box_ignore(*q, a["B"], a["H"], a["W"], 0, 255, None) == WC_ERR_ARG


@pytest.mark.parametrize("kw", [dict(B=0), dict(C=0), dict(H=0), dict(h2=0), dict(h2=9), dict(w2=13), dict(Kmax=0), dict(Kmax=5), dict(null=0),
                                dict(null=1), dict(null=2)])
def test_bkg_refine_limits(so, kw):
    a = dict(B=2, C=3, H=8, W=12, h2=4, w2=6, Kmax=3)
    a.update({k: v for k, v in kw.items() if k != "null"})
    p = [P] * 3
    if "null" in kw:
        p[kw["null"]] = None
    assert so.wc_bkg_refine_prep(*p, a["B"], a["C"], a["H"], a["W"], a["h2"], a["w2"], a["Kmax"], 4.4, 2.8, None) == WC_ERR_ARG
    if "C" not in kw and kw.get("Kmax") != 5:
        q = [P] * 4
        if "null" in kw:
            q[kw["null"]] = None
        assert so.wc_bkg_refine_finish(*q, a["B"], a["H"], a["W"], a["h2"], a["w2"], a["Kmax"], 255.0, None) == WC_ERR_ARG


@pytest.mark.parametrize("kw", [dict(G=0), dict(B=0), dict(C=0), dict(hb=1), dict(hb=9), dict(wb=13), dict(wb=1), dict(Kg=0), dict(Kg=4),
                                dict(null=0), dict(null=1), dict(null=2)])
def test_box_gather_scatter_limits(so, kw):
    a = dict(G=2, B=2, C=3, H=8, W=12, hb=6, wb=7, Kg=2)
    a.update({k: v for k, v in kw.items() if k != "null"})
    p, q = [P] * 5, [P] * 3
    if "null" in kw:
        p[kw["null"]] = q[kw["null"]] = None
    dims = (a["G"], a["B"], a["C"], a["H"], a["W"], a["hb"], a["wb"], a["Kg"])
    assert so.wc_box_gather(*p, *dims, None) == WC_ERR_ARG
    assert so.wc_box_scatter(*q, *dims, None) == WC_ERR_ARG
