"""Dense CRF without a GPU: the drop-in resolves `utils.dcrf` to this package, calls fail loudly, every C-ABI limit is
rejected before a launch, and the compiler issues the loads of csrc/dcrf.hip together."""
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


def test_dropin_resolves_utils_dcrf_to_the_package(tmp_path):
    (tmp_path / "utils").mkdir()
    (tmp_path / "utils" / "__init__.py").write_text("")
    (tmp_path / "utils" / "dcrf.py").write_text("raise ImportError('decoy: pydensecrf is not installed')\n")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import weclip_vit_comer_amd
        weclip_vit_comer_amd.install_dropin(reference_root={str(tmp_path)!r})
        from utils.dcrf import DenseCRF, crf_inference, crf_inference_label
        import utils.dcrf
        assert DenseCRF.__module__ == "weclip_vit_comer_amd.utils.dcrf", DenseCRF.__module__
        assert utils.dcrf.__file__.startswith({ROOT!r}), utils.dcrf.__file__
        print("ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr


def test_calls_without_a_gpu_raise():
    import numpy as np
    from weclip_vit_comer_amd.utils import dcrf
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    img = np.zeros((4, 5, 3), np.uint8)
    P = np.full((2, 4, 5), 0.5, np.float32)
    with pytest.raises(RuntimeError, match="GPU"):
        dcrf.DenseCRF(10, 3, 3, 4, 64, 5)(img, P)
    with pytest.raises(RuntimeError, match="GPU"):
        dcrf.crf_inference(img, P, labels=2)
    with pytest.raises(RuntimeError, match="GPU"):
        dcrf.crf_inference_label(img, np.zeros((4, 5), np.int64), n_labels=2)


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, _, args in _lib.parse_header():
        if name.startswith("wc_dcrf"):
            getattr(so, name).argtypes = [t for t, _ in args]
    return so


P = ctypes.c_void_p(256)           # never dereferenced: every call below is rejected before any launch


def _inf(so, **kw):
    a = dict(img=P, u8=1, unary=P, Q=P, ws=P, C=21, H=8, W=8, iters=10, pos_w=3.0, pos_std=3.0, bi_w=4.0, bi_xy=64.0,
             bi_rgb=5.0)
    a.update(kw)
    return so.wc_dcrf_inference(a["img"], a["u8"], a["unary"], a["Q"], a["ws"], a["C"], a["H"], a["W"], a["iters"], a["pos_w"],
                                a["pos_std"], a["bi_w"], a["bi_xy"], a["bi_rgb"], None)


@pytest.mark.parametrize("kw", [dict(C=0), dict(C=129), dict(H=0), dict(W=0), dict(H=641, W=640), dict(H=409601, W=1),
                                dict(pos_std=0.0), dict(bi_xy=-1.0), dict(bi_rgb=0.0), dict(bi_rgb=float("nan")),
                                dict(pos_std=float("inf")), dict(iters=-1), dict(img=None), dict(unary=None), dict(Q=None),
                                dict(ws=None)])
def test_inference_limits(so, kw):
    assert _inf(so, **kw) == WC_ERR_ARG


def test_other_entries_limits(so):
    assert so.wc_dcrf_message(P, 1, P, P, P, P, P, 0, 8, 8, 3.0, 64.0, 5.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_message(P, 1, P, P, P, P, P, 21, 8, 8, 3.0, 0.0, 5.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_message(P, 1, P, None, P, P, P, 21, 8, 8, 3.0, 64.0, 5.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_message(P, 1, P, P, P, P, P, 21, 700, 700, 3.0, 64.0, 5.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_unary_prob(P, P, 129, 8, 8, None) == WC_ERR_ARG
    assert so.wc_dcrf_unary_prob(None, P, 21, 8, 8, None) == WC_ERR_ARG
    assert so.wc_dcrf_unary_label(P, P, 21, 8, 8, 1.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_unary_label(P, P, 1, 8, 8, 0.7, None) == WC_ERR_ARG
    assert so.wc_dcrf_unary_logits(P, P, 21, 0, 8, 8, 8, None) == WC_ERR_ARG
    assert so.wc_dcrf_unary_logits(P, P, 21, 8, 8, 641, 641, None) == WC_ERR_ARG
    n = ctypes.c_long(-7)
    assert so.wc_dcrf_workspace_floats(200, 8, 8, ctypes.byref(n)) == WC_ERR_ARG and n.value == -7
    assert so.wc_dcrf_workspace_floats(21, 8, 8, ctypes.byref(n)) == 0 and n.value == 64 * (12 + 2 * 32 + 3 * 21)
    with pytest.raises(RuntimeError, match="bad argument"):
        _lib.lib().wc_dcrf_inference(P, 1, P, P, P, 21, 8, 8, -1, 3.0, 3.0, 4.0, 64.0, 5.0, None)


# kernels of csrc/dcrf.hip that may wait for a load alone, and why
ALLOWED = {
    "dcrf_feat_kernel": "uint8 / f32 image branch, one pixel per thread, once per call",
    "dcrf_scale_kernel": "two independent loads; the wait is for the last of them (nothing to overlap with)",
}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_dcrf_kernels_issue_their_loads_together(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_scan
    rows = isa_scan.report([os.path.join(ROOT, "weclip-vit-comer_amd", "csrc", "dcrf.hip")], threshold=1, out_dir=str(tmp_path))
    bad = [(alone, loads, name) for alone, loads, _, name, _ in rows if not any(a in name for a in ALLOWED)]
    assert not bad, "loads waited for one at a time (see tools/isa_scan.py): %s" % bad
