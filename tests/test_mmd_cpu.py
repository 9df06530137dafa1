"""utils.mmdloss without a GPU: the drop-in import, the reference's signatures, host-side argument errors, no CPU fallback."""
import inspect
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import weclip_vit_comer_amd  # noqa: F401
from weclip_vit_comer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dropin_import_resolves_without_a_reference_root(tmp_path):
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import weclip_vit_comer_amd
        weclip_vit_comer_amd.install_dropin()
        from utils.mmdloss import mmd_rbf, rbf_kernel
        import inspect, utils.mmdloss
        assert utils.mmdloss is weclip_vit_comer_amd.utils.mmdloss
        for f in (mmd_rbf, rbf_kernel):
            p = inspect.signature(f).parameters
            assert list(p) == ["source", "target", "kernel_mul", "kernel_num", "fix_sigma"], list(p)
            assert p["kernel_mul"].default == 2.0 and p["kernel_num"].default == 5 and p["fix_sigma"].default is None
        print("ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_signatures_carry_the_reference_defaults():
    from weclip_vit_comer_amd.utils import mmdloss
    for f in (mmdloss.mmd_rbf, mmdloss.rbf_kernel):
        p = inspect.signature(f).parameters
        assert [(k, v.default) for k, v in p.items()][2:] == [("kernel_mul", 2.0), ("kernel_num", 5), ("fix_sigma", None)]


@pytest.mark.parametrize("fn", ["mmd_rbf", "rbf_kernel"])
def test_argument_errors_are_raised_on_the_host(fn):
    from weclip_vit_comer_amd.utils import mmdloss
    f = getattr(mmdloss, fn)
    with pytest.raises(ValueError, match="rows"):
        f(torch.zeros(3, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="rows"):
        f(torch.zeros(1, 4), torch.zeros(5, 4))
    with pytest.raises(ValueError, match="widths"):
        f(torch.zeros(3, 4), torch.zeros(3, 5))
    with pytest.raises(ValueError, match="2-D"):
        f(torch.zeros(4), torch.zeros(4))
    with pytest.raises(ValueError, match="2-D"):
        f(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="float32 or both float16"):
        f(torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.float16))
    with pytest.raises(ValueError, match="float32 or both float16"):
        f(torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="kernel_num"):
        f(torch.zeros(3, 4), torch.zeros(3, 4), kernel_num=9)
    with pytest.raises(ValueError, match="kernel_num"):
        f(torch.zeros(3, 4), torch.zeros(3, 4), kernel_num=0)
    with pytest.raises(ValueError, match="kernel_mul"):
        f(torch.zeros(3, 4), torch.zeros(3, 4), kernel_mul=0.0)
    with pytest.raises(ValueError, match="bad argument"):
        f(torch.zeros(2, 8193), torch.zeros(2, 8193))


@pytest.mark.parametrize("fn", ["mmd_rbf", "rbf_kernel"])
def test_cpu_tensors_raise_the_gpu_error(fn):
    from weclip_vit_comer_amd.utils import mmdloss
    with pytest.raises(RuntimeError, match="GPU"):
        getattr(mmdloss, fn)(torch.zeros(3, 4), torch.ones(3, 4))


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    names = weclip_vit_comer_amd.register_torch_ops()
    assert {"mmd_rbf", "rbf_kernel"} <= set(names)
    with FakeTensorMode():
        s, t = torch.empty(5, 7, device="cuda", dtype=torch.float16), torch.empty(5, 7, device="cuda", dtype=torch.float16)
        loss, grad = torch.ops.weclip.mmd_rbf(s, t, 2.0, 5, 0.0, True)
        assert loss.shape == () and loss.dtype == torch.float32 and tuple(grad.shape) == (10, 7) and grad.dtype == torch.float32
        assert tuple(torch.ops.weclip.mmd_rbf(s, t, 2.0, 5, 0.0, False)[1].shape) == (0, 7)
        K = torch.ops.weclip.rbf_kernel(s, t, 2.0, 5, 0.0)
        assert tuple(K.shape) == (10, 10) and K.dtype == torch.float32
    with pytest.raises(NotImplementedError):
        torch.ops.weclip.mmd_rbf(torch.zeros(3, 4), torch.zeros(3, 4), 2.0, 5, 0.0, False)


def test_c_entries_refuse_bad_arguments():
    import ctypes
    lib = _lib.lib()
    n = ctypes.c_long()
    lib.wc_mmd_workspace_bytes(2048, 768, ctypes.byref(n))
    N, dp, nt = 4096, 768, 64
    up = lambda b: (b + 255) // 256 * 256                                             # noqa: E731
    assert n.value == up(8 * 64 * dp) + up(8 * nt * 16) + up(8 * dp) + 2 * up(4 * N) + 256 + up(4 * N * dp)
    p = ctypes.c_void_p(256)
    for kw in (dict(B=0), dict(d=0), dict(d=8193), dict(num=0), dict(num=9), dict(mul=0.0), dict(mul=-2.0), dict(fix=float("nan"))):
        a = dict(B=4, d=4, num=5, mul=2.0, fix=0.0)
        a.update(kw)
        with pytest.raises(RuntimeError, match="bad argument"):
            lib.wc_mmd_rbf(p, p, 0, p, None, p, a["B"], a["d"], a["num"], a["mul"], a["fix"], None)
        with pytest.raises(RuntimeError, match="bad argument"):
            lib.wc_mmd_rbf_kernel(p, p, 0, p, p, a["B"], a["d"], a["num"], a["mul"], a["fix"], None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.wc_mmd_rbf(None, p, 0, p, None, p, 4, 4, 5, 2.0, 0.0, None)
    with pytest.raises(RuntimeError, match="aligned"):
        lib.wc_mmd_rbf(p, p, 0, p, None, ctypes.c_void_p(260), 4, 4, 5, 2.0, 0.0, None)
