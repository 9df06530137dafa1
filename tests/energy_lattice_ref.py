"""Float64 restatement of the dense energy loss with the permutohedral lattice as its bilateral filter (DESIGN.md section 15.3;
include/weclip_hip.h wc_bilateral_filter_batch_lattice, wc_dense_energy_fwd_lattice).  No new algorithm: the loss, Gate and
gradient are tests/energy_ref.py's, the filter is tests/dcrf_lattice_ref.py's build + filter per image (un-normalised, forward
blur order, alpha = 1 / (1 + 2^-d)); this file only composes them.  `filt` is the batched filter: `lattice_filter_batch` here,
or energy_ref.bilateral_filter_batch, with which every function below is energy_ref's / energy_term_ref's own."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcrf_lattice_ref as LR  # noqa: E402
import energy_ref as E  # noqa: E402
import energy_term_ref as T  # noqa: E402

F64 = torch.float64


def lattice_filter_batch(images, segs, sigma_rgb, sigma_xy, want_abs=False, counts=None):
    """AS (N, K, H, W) fp64: image n's lattice built from images[n] (3, H, W), clamped to [0, 256], at (sigma_xy, sigma_rgb), filter
    of segs[n].
    want_abs: also the filter of |segs| (the scale of the kernels' error bound).  counts: a list that receives every M."""
    images, segs = torch.as_tensor(images), torch.as_tensor(segs).to(F64)
    N, K, H, W = segs.shape
    out, out_abs = [], []
    for n in range(N):
        # colours outside [0, 256] are clamped before the build, as the header says of the kernels (they report it in a flag)
        lat = LR.build(images[n].to(F64).clamp(0.0, 256.0).permute(1, 2, 0).contiguous(), H, W, sigma_xy, sigma_rgb)
        if counts is not None:
            counts.append(lat.M)
        V = segs[n].reshape(K, H * W).T.numpy()
        out.append(torch.from_numpy(LR.filter(lat, V).T.reshape(K, H, W)))
        if want_abs:
            out_abs.append(torch.from_numpy(LR.filter(lat, np.abs(V)).T.reshape(K, H, W)))
    AS = torch.stack(out)
    return (AS, torch.stack(out_abs)) if want_abs else AS


def energy_function(images, segs, sigma_rgb, sigma_xy, rois, unlabel, filt=lattice_filter_batch):
    """energy_ref.energy_function with the filter `filt`: dict(loss, A, gate, AS, S, grad = -2 A ROI / N, the Gate constant)."""
    P = torch.as_tensor(segs).to(F64)
    roi = torch.as_tensor(rois).to(F64)
    N = P.shape[0]
    G = E.gate(P, roi, unlabel)
    S = P * roi[:, None]
    AS = filt(images, S, sigma_rgb, sigma_xy)
    A = G[:, None] * AS
    loss = -(S * A).sum().reshape(1) / N
    return dict(loss=loss, A=A, gate=G, AS=AS, S=S, grad=-2.0 * A * roi[:, None] / N)


def energy_loss(img, logit, label, img_box, weight, sigma_rgb, sigma_xy, s, filt=lattice_filter_batch, mean=T.MEAN, std=T.STD):
    """energy_ref.energy_loss (get_energy_loss on full-resolution logits) with the filter `filt`."""
    lg = torch.as_tensor(logit).to(F64).clone().requires_grad_(True)
    prob = torch.softmax(lg, dim=1)
    _img = E.denormalise(torch.as_tensor(img).to(F64), mean, std)
    rois = E.crop_mask(prob[:, 0].detach(), img_box)
    si, ss, sr, unl = E.scaled_inputs(_img, prob, rois, torch.as_tensor(label).to(torch.uint8).unsqueeze(1), s)
    r = energy_function(si, ss.detach(), sigma_rgb, sigma_xy * s, sr, unl, filt)
    (g,) = torch.autograd.grad(ss, lg, grad_outputs=weight * r["grad"])
    return dict(loss=weight * r["loss"], grad_logit=g, gate=r["gate"], A=r["A"])


def energy_term(img, seg, label, img_box, weight, sigma_rgb, sigma_xy, s, filt=lattice_filter_batch, mean=T.MEAN, std=T.STD):
    """energy_term_ref.energy_term (get_energy_loss_fused on low-resolution logits) with the filter `filt`."""
    sg = torch.as_tensor(seg).to(F64).clone().requires_grad_(True)
    si, ss, sr, unl = T.prep_forward(torch.as_tensor(img), sg, torch.as_tensor(label), img_box, s, F64, mean, std)
    r = energy_function(si, ss.detach(), sigma_rgb, sigma_xy * s, sr, unl, filt)
    (g,) = torch.autograd.grad(ss, sg, grad_outputs=weight * r["grad"])
    return dict(loss=weight * r["loss"], grad=g)
