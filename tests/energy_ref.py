"""Float64 CPU restatement of the dense energy loss (include/weclip_hip.h wc_dense_energy_*): the
whole chain of the reference's utils/losses.py:35-116, `get_energy_loss` down to the gradient on the logits, with the
bilateral filter as a brute-force all-pairs sum (no lattice).  images (N,3,H,W) on the 0..255 scale, segs (N,K,H,W)."""
import torch
import torch.nn.functional as F

F64 = torch.float64


def _features(img, sigma_rgb, sigma_xy):
    """(HW, 5) fp64 rows (x, y, R, G, B), each divided by its sigma, centred (differences stay exact far below 2^-40)."""
    _, H, W = img.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    f = torch.stack([xs.reshape(-1) / sigma_xy, ys.reshape(-1) / sigma_xy] + [img[c].to(F64).reshape(-1) / sigma_rgb for c in range(3)], 1)
    return f - f.mean(0)


def kernel_rows(img, sigma_rgb, sigma_xy, rows=None):
    """k(i, j) = exp(-|p_i - p_j|^2 / (2 sigma_xy^2) - |I_i - I_j|^2 / (2 sigma_rgb^2)) for i in rows (all by default): (R, HW)."""
    f = _features(torch.as_tensor(img), sigma_rgb, sigma_xy)
    q = f if rows is None else f[rows]
    return torch.exp(-0.5 * torch.cdist(q, f, compute_mode="donot_use_mm_for_euclid_dist").square_())


def bilateral_filter_batch(images, segs, sigma_rgb, sigma_xy, rows=None, want_abs=False):
    """AS (N, K, H, W) fp64 = sum_j k_n(i, j) segs(n, :, j); with rows (an index tensor of pixels): (N, K, len(rows)).
    want_abs: also sum_j k |segs_j| (the scale of the kernels' error bound), same shape."""
    images, segs = torch.as_tensor(images), torch.as_tensor(segs).to(F64)
    N, K, H, W = segs.shape
    HW = H * W
    chunk = max(1, (1 << 23) // HW)
    out, out_abs = [], []
    for n in range(N):
        S = segs[n].reshape(K, HW).T
        idx = torch.arange(HW) if rows is None else torch.as_tensor(rows)
        a = torch.empty(len(idx), K, dtype=F64)
        b = torch.empty(len(idx), K, dtype=F64)
        for s in range(0, len(idx), chunk):
            k = kernel_rows(images[n], sigma_rgb, sigma_xy, idx[s:s + chunk])
            a[s:s + chunk] = k @ S
            if want_abs:
                b[s:s + chunk] = k @ S.abs()
        out.append(a.T)
        out_abs.append(b.T)
    shape = (N, K, H, W) if rows is None else (N, K, len(rows))
    AS = torch.stack(out).reshape(shape)
    return (AS, torch.stack(out_abs).reshape(shape)) if want_abs else AS


def gate(segs, rois, unlabel):
    """Gate (N, H, W) = ROI - max_k P, then 1 where unlabelled, then 0 where negative, in the dtype of `segs`."""
    g = torch.as_tensor(rois).to(segs.dtype) - segs.max(1).values
    g = torch.where(torch.as_tensor(unlabel).bool(), torch.ones_like(g), g)
    return torch.where(g < 0, torch.zeros_like(g), g)


def energy_function(images, segs, sigma_rgb, sigma_xy, rois, unlabel):
    """DenseEnergyLossFunction in fp64: dict(loss (1,), A = Gate * AS, gate, AS, S = P * ROI, grad: d loss / d segs for an
    upstream gradient of 1 = -2 A ROI / N, the Gate held constant)."""
    P = torch.as_tensor(segs).to(F64)
    roi = torch.as_tensor(rois).to(F64)
    N = P.shape[0]
    G = gate(P, roi, unlabel)
    S = P * roi[:, None]
    AS = bilateral_filter_batch(images, S, sigma_rgb, sigma_xy)
    A = G[:, None] * AS
    loss = -(S * A).sum().reshape(1) / N
    return dict(loss=loss, A=A, gate=G, AS=AS, S=S, grad=-2.0 * A * roi[:, None] / N)


def scaled_inputs(images, segs, rois, seg_label, s):
    """DenseEnergyLoss.forward's set-up at scale factor s: (images, segs, ROIs, unlabel) at the scaled size."""
    si = F.interpolate(images, scale_factor=s)
    ss = F.interpolate(segs, scale_factor=s, mode="bilinear", align_corners=False)
    sr = F.interpolate(rois.unsqueeze(1), scale_factor=s).squeeze(1)
    sl = F.interpolate(seg_label.to(images.dtype), scale_factor=s, mode="nearest")
    return si, ss, sr, (sl.long() == 255).squeeze(1)


def denormalise(img, mean, std):
    return torch.stack([img[:, c] * std[c] + mean[c] for c in range(3)], 1)


def crop_mask(like, img_box):
    m = torch.zeros_like(like)
    for i, b in enumerate(img_box):
        m[i, int(b[0]):int(b[1]), int(b[2]):int(b[3])] = 1
    return m


def energy_loss(img, logit, label, img_box, weight, sigma_rgb, sigma_xy, s, mean=(123.675, 116.28, 103.53),
                std=(58.395, 57.12, 57.375)):
    """get_energy_loss(img, logit, label, img_box, DenseEnergyLoss(weight, sigma_rgb, sigma_xy, s)) in fp64:
    dict(loss (1,), grad_logit, gate, A, segs (the scaled soft-max), rois, unlabel, images: the Function's inputs)."""
    lg = torch.as_tensor(logit).to(F64).clone().requires_grad_(True)
    prob = F.softmax(lg, dim=1)
    _img = denormalise(torch.as_tensor(img).to(F64), mean, std)
    rois = crop_mask(prob[:, 0].detach(), img_box)
    si, ss, sr, unl = scaled_inputs(_img, prob, rois, torch.as_tensor(label).to(torch.uint8).unsqueeze(1), s)
    r = energy_function(si, ss.detach(), sigma_rgb, sigma_xy * s, sr, unl)
    (g,) = torch.autograd.grad(ss, lg, grad_outputs=weight * r["grad"])
    return dict(loss=weight * r["loss"], grad_logit=g, gate=r["gate"], A=r["A"], segs=ss.detach(), rois=sr, unlabel=unl, images=si)
