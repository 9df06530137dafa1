"""Restatement of the reference's utils/camutils.py pseudo-label chain in stock torch ops, written from its definitions
(DESIGN.md section 16), in the precision of its inputs: the tests feed it float64 (the yardstick of csrc/camlabel.hip), the
benchmark tool feeds it float32 on the device as the "stock ops" side.  It keeps the reference's structure: per-image loops,
`nonzero` per image, one refinement call per image and threshold.

    A[b,i,j] = (aff[b,i,j] [mask[i,j] != 0])^2;  out[b,k,j] = sum_i X[b,k,i] A[b,i,j] / (sum_i A[b,i,j] + eps)
"""
import numpy as np
import torch
import torch.nn.functional as F


def _box(row, H, W):
    return slice(int(row[0]), int(row[1])), slice(int(row[2]), int(row[3]))


def _resize(x, size, align_corners=False):
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=align_corners)


def ignore_img_box(label, img_box, ignore_index):
    out = torch.full_like(label, ignore_index)
    for b, row in enumerate(img_box):
        ys, xs = _box(row, *label.shape[1:])
        out[b, ys, xs] = label[b, ys, xs]
    return out


def cam_to_label(cam, cls_label, img_box=None, ignore_mid=False, cfg=None):
    valid = cls_label.to(cam.dtype)[:, :, None, None] * cam
    value, label = valid.max(dim=1)
    label = label + 1
    label[value <= cfg.cam.bkg_score] = 0
    if img_box is None:
        return label
    if ignore_mid:
        label[value <= cfg.cam.high_thre] = cfg.dataset.ignore_index
        label[value <= cfg.cam.low_thre] = 0
    return valid, ignore_img_box(label, img_box, cfg.dataset.ignore_index)


def _walk(X, aff, mask, eps):
    """X (K, n), aff (n, n) -> (K, n)."""
    A = aff if mask is None else aff * (mask != 0).to(aff.dtype)
    A = A * A
    return (X @ A) / (A.sum(dim=0, keepdim=True) + eps)


def propagte_aff_cam(cams, aff=None, mask=None):
    b, c, h, w = cams.shape
    return torch.stack([_walk(cams[i].reshape(c, -1), aff[i].to(cams.dtype), mask, 1e-4) for i in range(b)]).reshape(b, c, h, w)


def propagte_aff_cam_with_bkg(cams, aff=None, mask=None, cls_labels=None, bkg_score=None):
    b, c, h, w = cams.shape
    out = torch.zeros(b, c + 1, h, w, dtype=cams.dtype, device=cams.device)
    for i in range(b):
        keys = torch.nonzero(cls_labels[i])[:, 0]
        x = torch.cat([torch.full((1, h * w), bkg_score, dtype=cams.dtype, device=cams.device), cams[i, keys].reshape(len(keys), h * w)])
        rows = torch.cat([keys.new_zeros(1), keys + 1])
        out[i, rows] = _walk(torch.softmax(x, dim=0), aff[i].to(cams.dtype), mask, 1e-1).reshape(-1, h, w)
    return out


class Par:
    """Pixel-adaptive refinement (reference WeCLIP_model/PAR.py:64-92) in the precision of its inputs, any batch."""

    def __init__(self, dilations, num_iter, w1=0.3, w2=0.01):
        self.dilations, self.num_iter, self.w1, self.w2 = list(dilations), int(num_iter), w1, w2

    def _neighbours(self, x):
        H, W = x.shape[-2:]
        ys, xs = torch.arange(H, device=x.device), torch.arange(W, device=x.device)
        out = []
        for d in self.dilations:
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dy or dx:
                        out.append(x[..., (ys + dy * d).clamp(0, H - 1), :][..., (xs + dx * d).clamp(0, W - 1)])
        return torch.stack(out, dim=2)                        # (b, c, T, H, W)

    def __call__(self, imgs, masks):
        imgs = _resize(imgs.to(masks.dtype), masks.shape[-2:], align_corners=True)
        nb = self._neighbours(imgs)
        e = -(((nb - imgs[:, :, None]).abs() / (nb.std(dim=2, keepdim=True) + 1e-8) / self.w1) ** 2).mean(dim=1, keepdim=True)
        pos = torch.tensor([d * (2.0 ** 0.5 if dy and dx else 1.0) for d in self.dilations for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                            if dy or dx], dtype=masks.dtype, device=masks.device)
        pe = -((pos / (pos.std() + 1e-8) / self.w1) ** 2)
        aff = torch.softmax(e, dim=2) + self.w2 * torch.softmax(pe, dim=0)[None, None, :, None, None]
        for _ in range(self.num_iter):
            masks = (self._neighbours(masks) * aff).sum(dim=2)
        return masks


def bkg_refined_maps(ref_mod, images, cams, cls_labels, cfg, down_scale=2):
    """Per image (label values, refined high-threshold maps, refined low-threshold maps), both (K_b, H, W) after the
    up-sample: what refine_cams_with_bkg_v2 takes its arg-max of."""
    b, _, h, w = images.shape
    size = (h // down_scale, w // down_scale)
    _images = _resize(images.to(cams.dtype), size)
    out = []
    for i in range(b):
        keys = torch.nonzero(cls_labels[i])[:, 0]
        values = torch.cat([keys.new_zeros(1), keys + 1])
        maps = []
        for thre in (cfg.cam.high_thre, cfg.cam.low_thre):
            x = torch.cat([torch.full((1, 1, h, w), thre, dtype=cams.dtype, device=cams.device), cams[i:i + 1, keys]], dim=1)
            maps.append(_resize(ref_mod(_images[i:i + 1], torch.softmax(_resize(x, size), dim=1)), (h, w))[0])
        out.append((values, maps[0], maps[1]))
    return out


def refine_cams_with_bkg_v2(ref_mod, images, cams, cls_labels, cfg, img_box, down_scale=2):
    b, _, h, w = images.shape
    ign = cfg.dataset.ignore_index
    lab_h = torch.full((b, h, w), float(ign), dtype=cams.dtype, device=cams.device)
    lab_l = lab_h.clone()
    for i, (values, mh, ml) in enumerate(bkg_refined_maps(ref_mod, images, cams, cls_labels, cfg, down_scale)):
        ys, xs = _box(img_box[i], h, w)
        lab_h[i, ys, xs] = values[mh.argmax(dim=0)].to(cams.dtype)[ys, xs]
        lab_l[i, ys, xs] = values[ml.argmax(dim=0)].to(cams.dtype)[ys, xs]
    out = lab_h.clone()
    out[lab_h == 0] = ign
    out[(lab_h + lab_l) == 0] = 0
    return out


def refine_cams_with_cls_label(ref_mod, images, labels, cams, img_box):
    out = torch.zeros_like(cams)
    for i, row in enumerate(img_box):
        ys, xs = _box(row, *cams.shape[2:])
        crop = images[i:i + 1, :, ys, xs].to(cams.dtype)
        keys = torch.nonzero(labels[i])[:, 0]
        small = _resize(crop, (crop.shape[2] // 2, crop.shape[3] // 2))
        out[i, keys, ys, xs] = ref_mod(small, cams[i:i + 1, :, ys, xs][:, keys])[0]
    return out


def _multi_scale(model, inputs, scales):
    b, _, h, w = inputs.shape

    def one(x):
        cam, aff = model(torch.cat([x, x.flip(-1)]), cam_only=True)
        cam = _resize(cam.to(inputs.dtype), (h, w))
        return torch.relu(torch.max(cam[:b], cam[b:].flip(-1))), aff

    runs = [one(inputs)] + [one(_resize(inputs, (int(s * h), int(s * w)))) for s in scales if s != 1.0]
    cam = sum(c for c, _ in runs)
    cam = cam - cam.amin(dim=(2, 3), keepdim=True)
    return cam / (cam.amax(dim=(2, 3), keepdim=True) + 1e-5), [a for _, a in runs]


def multi_scale_cam(model, inputs, scales):
    return _multi_scale(model, inputs, scales)[0]


def multi_scale_cam_with_aff_mat(model, inputs, scales):
    cam, affs = _multi_scale(model, inputs, scales)
    return cam, affs[np.argmax(scales)]


def top2_margin(maps, dim=0):
    """Largest minus second largest along `dim` (infinite for a single channel)."""
    if maps.shape[dim] < 2:
        return torch.full_like(maps.select(dim, 0), float("inf"))
    t = maps.topk(2, dim=dim).values
    return t.select(dim, 0) - t.select(dim, 1)
