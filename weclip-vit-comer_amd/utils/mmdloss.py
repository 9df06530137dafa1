"""Multi-bandwidth RBF maximum mean discrepancy on the GPU: the reference's utils/mmdloss.py (`rbf_kernel` :4-35, `mmd_rbf`
:38-59) with its signatures and defaults, served by csrc/mmd.hip.

What differs from the reference, on purpose:
  * source and target need the same number of rows (ValueError otherwise): the reference's four blocks add only then; it raises
    on unequal counts, or broadcasts a one-row side into something that is not an MMD.
  * neither the (N, N, d) expansion nor -- for `mmd_rbf` -- the (N, N) matrix is ever formed; `rbf_kernel` returns the matrix
    and is meant for small N.  `rbf_kernel` carries no autograd; `mmd_rbf` is differentiable in both inputs, with the bandwidth
    a constant as in the reference (`.data`, :28).
  * inputs are float32 or float16, computed in float32; the loss is a 0-dim float32 tensor, gradients come back in the inputs'
    dtype.  `fix_sigma` is a Python number (or None / 0: bandwidth from the data, which stays on the device).
  * all rows identical gives bandwidth 0 and a NaN loss, as in the reference.
There is no CPU path: without a GPU, or on CPU tensors, both functions raise RuntimeError."""
import torch

from .. import ops


def rbf_kernel(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """K (n + m, n + m) = sum over kernel_num bandwidths of exp(-|x_i - x_j|^2 / bw_b) for x = cat(source, target)."""
    _, _, fix = ops.mmd_check(source, target, kernel_mul, kernel_num, fix_sigma, "rbf_kernel")
    ops.mmd_device(source, "rbf_kernel")
    from .. import torch_ops  # noqa: F401  (registers torch.ops.weclip.*)
    return torch.ops.weclip.rbf_kernel(source, target, float(kernel_mul), int(kernel_num), fix)


def mmd_rbf(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """mean(XX + YY - XY - YX) over the four blocks of `rbf_kernel`: a 0-dim tensor, differentiable in source and target."""
    _, _, fix = ops.mmd_check(source, target, kernel_mul, kernel_num, fix_sigma, "mmd_rbf")
    ops.mmd_device(source, "mmd_rbf")
    from .. import torch_ops  # noqa: F401
    need_grad = torch.is_grad_enabled() and (source.requires_grad or target.requires_grad)
    return torch.ops.weclip.mmd_rbf(source, target, float(kernel_mul), int(kernel_num), fix, need_grad)[0]
