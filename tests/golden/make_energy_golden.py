"""Generate tests/golden/energy_loss.npz by RUNNING THE UNMODIFIED REFERENCE's dense energy loss on the CPU.

Build-container only (needs the reference checkout; oracle/refharness.py imports it without its missing packages).
    python tests/golden/make_energy_golden.py
The reference's utils/losses.py calls `bilateralfilter_batch(images, segmentations, AS, N, K, H, W, sigma_rgb, sigma_xy)` from an
extension it does not ship (the import is commented out).  This script assigns that name in the reference module's namespace:
an exact fp64 all-pairs filter written here (tests/energy_ref.py), rounded to the f32 array the reference hands over.  The
reference's `get_energy_loss`, `DenseEnergyLoss` and `DenseEnergyLossFunction` then run as they stand.  A second run with a
filter that writes ones leaves the reference's own Gate in `ctx.AS`.

Recorded per case i (data only, nothing of the reference's text): the inputs c{i}_img (normalised), c{i}_logit, c{i}_label,
c{i}_box, c{i}_cfg = (weight, sigma_rgb, sigma_xy, scale_factor), and the reference's c{i}_loss (1,), c{i}_grad (the
gradient on the logits), c{i}_gate (N,h,w) and c{i}_A (N,K,h,w) = Gate * AS at the scaled size, all f32."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import energy_ref as E  # noqa: E402

CFG = (1e-7, 15.0, 100.0)                     # weight, sigma_rgb, sigma_xy of the lineage's training scripts
CASES = [(2, 3, 12, 20, 0.5, "noise"), (3, 21, 26, 22, 0.5, "noise"), (1, 5, 16, 16, 1.0, "noise"), (2, 4, 16, 24, 0.5, "ramp")]
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def make_inputs(i, N, K, H, W, kind):
    """Random logits x 3, a 255 patch in the label, a box inside the image; the image is uniform noise or a colour ramp."""
    g = torch.Generator().manual_seed(100 + i)
    if kind == "noise":
        rgb = torch.rand(N, 3, H, W, generator=g) * 255
    else:
        ys, xs = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        rgb = torch.stack([torch.stack([40 + 60 * xs + 20 * n, 90 + 50 * ys, 140 + 30 * (xs + ys)]) for n in range(N)])
        rgb = rgb + torch.rand(N, 3, H, W, generator=g)
    img = torch.stack([(rgb[:, c] - MEAN[c]) / STD[c] for c in range(3)], 1)
    logit = 3 * torch.randn(N, K, H, W, generator=g)
    label = torch.randint(0, K, (N, H, W), generator=g)
    label[:, H // 4:H // 2, W // 3:W // 3 + 5] = 255
    box = torch.tensor([[1 + n % 2, H - 2, 2, W - 1 - n % 3] for n in range(N)])
    return img.float(), logit.float(), label, box


def exact_filter(images, segmentations, AS, N, K, H, W, sigma_rgb, sigma_xy):
    img = torch.from_numpy(np.asarray(images)).reshape(N, 3, H, W)
    seg = torch.from_numpy(np.asarray(segmentations)).reshape(N, K, H, W)
    AS[:] = E.bilateral_filter_batch(img, seg, sigma_rgb, sigma_xy).reshape(-1).to(torch.float32).numpy()


def ones_filter(images, segmentations, AS, N, K, H, W, sigma_rgb, sigma_xy):
    AS[:] = 1.0


def _ctx_AS(loss):
    """The `AS` attribute the reference's Function leaves on its autograd node."""
    todo = [loss.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None:
            continue
        if hasattr(fn, "AS"):
            return np.asarray(fn.AS)
        todo += [f for f, _ in fn.next_functions]
    raise RuntimeError("no autograd node with an AS attribute")


def main():
    from oracle import refharness
    refharness.install()
    import utils.losses as RL
    out = {}
    for i, (N, K, H, W, s, kind) in enumerate(CASES):
        img, logit, label, box = make_inputs(i, N, K, H, W, kind)
        layer = RL.DenseEnergyLoss(weight=CFG[0], sigma_rgb=CFG[1], sigma_xy=CFG[2], scale_factor=s)
        RL.bilateralfilter_batch = exact_filter
        lg = logit.clone().requires_grad_(True)
        loss = RL.get_energy_loss(img, lg, label, box.tolist(), layer)
        A = _ctx_AS(loss)
        loss.backward()
        RL.bilateralfilter_batch = ones_filter
        gate = _ctx_AS(RL.get_energy_loss(img, logit.clone().requires_grad_(True), label, box.tolist(), layer))[:, 0]
        r = E.energy_loss(img, logit, label, box.tolist(), CFG[0], CFG[1], CFG[2], s)
        e_loss = abs(r["loss"].item() - loss.item()) / abs(loss.item())
        e_grad = ((r["grad_logit"] - lg.grad.double()).abs().max() / lg.grad.abs().max()).item()
        print(f"case {i} {(N, K, H, W, s)} {kind}: loss {loss.item():.6e}; restatement vs reference: loss rel {e_loss:.1e}, "
              f"logit gradient / largest entry {e_grad:.1e}")
        out.update({f"c{i}_img": img.numpy(), f"c{i}_logit": logit.numpy(), f"c{i}_label": label.numpy().astype(np.uint8),
                    f"c{i}_box": box.numpy().astype(np.int32), f"c{i}_cfg": np.array(CFG + (s,), np.float64),
                    f"c{i}_loss": loss.detach().numpy().astype(np.float32).reshape(1), f"c{i}_grad": lg.grad.numpy(),
                    f"c{i}_gate": gate.astype(np.float32), f"c{i}_A": A.astype(np.float32)})
    np.savez_compressed(os.path.join(HERE, "energy_loss.npz"), **out)


if __name__ == "__main__":
    main()
