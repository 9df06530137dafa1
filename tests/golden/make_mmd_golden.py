"""Writes tests/golden/mmd_rbf.npz: the reference's own `mmd_rbf` and `rbf_kernel` (utils/mmdloss.py) run in fp64 with autograd.

    python tests/golden/make_mmd_golden.py --reference_root /path/to/reference

Per case `c` (B, d) in {(1,1), (2,3), (5,7), (33,40)} x fix_sigma in {None, a value near the data's mean squared distance}:
c_source, c_target (B, d) f64 inputs; c_fix (0.0 = None); c_loss; c_K (2B, 2B); c_grad_source, c_grad_target.
Recorded results only: nothing of the reference's code is stored."""
import argparse
import importlib.util
import os

import numpy as np
import torch

SHAPES = [(1, 1), (2, 3), (5, 7), (33, 40)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference_root", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "mmd_rbf.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("_ref_mmdloss", os.path.join(args.reference_root, "utils", "mmdloss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    out = {}
    names = []
    for B, d in SHAPES:
        g = torch.Generator().manual_seed(1000 * B + d)
        src = torch.randn(B, d, generator=g, dtype=torch.float64)
        tgt = 1.3 * torch.randn(B, d, generator=g, dtype=torch.float64) + 0.5
        X = torch.cat([src, tgt])
        mean_l2 = float(torch.cdist(X, X).square().sum() / (4 * B * B - 2 * B))
        for fix in (None, round(0.8 * mean_l2, 3)):
            name = f"B{B}_d{d}_{'data' if fix is None else 'fix'}"
            s, t = src.clone().requires_grad_(True), tgt.clone().requires_grad_(True)
            loss = ref.mmd_rbf(s, t, kernel_mul=2.0, kernel_num=5, fix_sigma=fix)
            gs, gt = torch.autograd.grad(loss, (s, t))
            K = ref.rbf_kernel(src, tgt, kernel_mul=2.0, kernel_num=5, fix_sigma=fix)
            names.append(name)
            out.update({f"{name}_source": src.numpy(), f"{name}_target": tgt.numpy(), f"{name}_fix": np.float64(fix or 0.0),
                        f"{name}_loss": loss.detach().numpy(), f"{name}_K": K.numpy(), f"{name}_grad_source": gs.numpy(),
                        f"{name}_grad_target": gt.numpy()})
    out["names"] = np.array(names)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {len(names)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
