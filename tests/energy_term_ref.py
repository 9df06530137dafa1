"""The dense energy loss as a term of the training step (include/weclip_hip.h wc_energy_prep_*): the
composition get_energy_loss(img, F.interpolate(seg_lowres, (H, W), bilinear), label, img_box, DenseEnergyLoss(..., s)) restated
with the stock torch ops at a chosen dtype (float64: the reference of the tests; float32: the stock chain whose own error the
bounds are compared with), on tests/energy_ref.py.  Also the inputs of the prep-kernel tests, shared by the CPU and GPU files."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_ref as E  # noqa: E402

F64 = torch.float64
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
ULP = 2.0 ** -24


def upsample(seg, size):
    return F.interpolate(seg, size=tuple(size), mode="bilinear", align_corners=False)


def prep_forward(img, seg, label, img_box, s, dtype=F64, mean=MEAN, std=STD):
    """(images_s, P_s, rois_s, unlabel (bool)) at scale factor s: what DenseEnergyLoss.forward hands to its Function when
    get_energy_loss is given the up-sampled `seg`.  img_box None = the whole image.  P_s carries the autograd graph of `seg`."""
    H, W = label.shape[1:]
    prob = F.softmax(upsample(seg.to(dtype), (H, W)), dim=1)
    _img = E.denormalise(img.to(dtype), mean, std)
    box = [[0, H, 0, W]] * img.shape[0] if img_box is None else img_box
    rois = E.crop_mask(prob[:, 0].detach(), box)
    return E.scaled_inputs(_img, prob, rois, label.to(torch.uint8).unsqueeze(1), s)


def prep_backward(seg, size, s, A, rois_s, coef, dtype=F64):
    """d/d seg of sum(P_s * G_s) with G_s = (coef * A) * rois_s held constant: what wc_energy_prep_bwd computes."""
    sg = seg.detach().to(dtype).clone().requires_grad_(True)
    P = F.interpolate(F.softmax(upsample(sg, size), dim=1), scale_factor=s, mode="bilinear", align_corners=False)
    G = (coef * A.to(dtype)) * rois_s.to(dtype)[:, None]
    (g,) = torch.autograd.grad(P, sg, grad_outputs=G)
    return g


def energy_term(img, seg, label, img_box, weight, sigma_rgb, sigma_xy, s, mean=MEAN, std=STD):
    """get_energy_loss_fused in fp64: dict(loss (1,) = weight * energy, grad = d loss / d seg (N,K,h,w), the Gate constant)."""
    sg = torch.as_tensor(seg).to(F64).clone().requires_grad_(True)
    si, ss, sr, unl = prep_forward(torch.as_tensor(img), sg, torch.as_tensor(label), img_box, s, F64, mean, std)
    r = E.energy_function(si, ss.detach(), sigma_rgb, sigma_xy * s, sr, unl)
    (g,) = torch.autograd.grad(ss, sg, grad_outputs=weight * r["grad"])
    return dict(loss=weight * r["loss"], grad=g)


def p_bound(K, M):
    """|P_s - P64| per element, M = max |up-sampled logit|: three roundings per interpolation on the way up, entering the exponent
    twice (the logit and the maximum), the maximum's subtraction, v_exp_f32 at ~2^-22, a K-term sum, the down-sample."""
    return (16 * M + K + 16) * ULP


# (h, w) -> (H, W): one low-resolution pixel; odd sizes with a last row and column that nothing taps at e > 0; the tiny model;
# the identity up-sample
SHAPES = [((1, 1), (4, 4)), ((2, 3), (37, 50)), ((4, 6), (64, 96)), ((16, 16), (16, 16))]
ES = [0, 1, 2]
KS = [1, 21, 33, 81, 128]
NS = [1, 3]


def boxes(kind, N, H, W):
    """img_box rows (y0, y1, x0, x1), different per image.  whole: None; rows: the whole image / one pixel / empty (y0 == y1);
    border: boxes that touch each border and leave the opposite one out."""
    if kind == "whole":
        return None
    if kind == "rows":
        rows = [[0, H, 0, W], [H // 3, H // 3 + 1, W // 2, W // 2 + 1], [2, 2, 0, W]]
    else:
        rows = [[0, H - 1, 1, W], [1, H, 0, W - 1], [0, H, 0, 1]]
    return [rows[n % 3] for n in range(N)]


def labels(kind, N, H, W, K, dtype, gen):
    """none: no pixel unlabelled; patch: a different patch of 255 per image (int64: also 511 and -1, whose low byte is 255, and
    256, whose low byte is not); all: every pixel 255."""
    lab = torch.randint(0, K, (N, H, W), generator=gen)
    if kind == "all":
        lab[:] = 255
    elif kind == "patch":
        for n in range(N):
            lab[n, n % H:n % H + max(H // 2, 1), (2 * n) % W:(2 * n) % W + max(W // 3, 1)] = 255
        if dtype == torch.int64:
            lab[:, H - 1, 0::3] = 511
            lab[:, 0, 1::3] = -1
            lab[:, H // 2, 0::2] = 256
    return lab.to(dtype)


def make_case(hw, HW, K, N, seed, magnitude=3.0):
    """Inputs of one prep case; the box kind, the label kind and the label dtype rotate with the seed."""
    g = torch.Generator().manual_seed(seed)
    (h, w), (H, W) = hw, HW
    img = torch.randn(N, 3, H, W, generator=g)
    seg = magnitude * torch.randn(N, K, h, w, generator=g)
    dtype = (torch.int64, torch.uint8)[seed % 2]
    lab = labels(("none", "patch", "all")[(seed // 2) % 3], N, H, W, K, dtype, g)
    return img, seg, lab, boxes(("whole", "rows", "border")[seed % 3], N, H, W)


def case_seed(si, e, K, N):
    return 1000 * si + 100 * e + K + 7 * N


def worst_p_ratio(P, P64, seg, size, K):
    M = upsample(seg.to(F64), size).abs().max().item()
    return ((P.double() - P64).abs().max() / p_bound(K, M)).item()
