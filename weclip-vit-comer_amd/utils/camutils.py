"""The reference's utils/camutils.py on the MI355X: the AFA pseudo-label chain of the lineage's training script
(scripts/.ipynb_checkpoints/dist_train_voc-checkpoint.py:309-339) behind the reference's names, argument order, defaults, return
types and dtypes.

`cams_to_affinity_label` (reference utils/camutils.py:226-247) and `get_mask_by_radius` (scripts/dist_clip_voc.py:116-133) are
vectorised stock PyTorch ops and also run on CPU tensors.  Everything else runs in csrc/camlabel.hip and has no
CPU path: without a GPU every call raises RuntimeError.

Common arguments.  `cfg`: anything with `.cam.bkg_score`, `.cam.high_thre`, `.cam.low_thre` and `.dataset.ignore_index`
(train.Config, OmegaConf).  `img_box`: B rows (y0, y1, x0, x1), as a sequence, a CPU tensor or a CUDA tensor; a row is applied
as the Python slices [y0:y1, x0:x1] are.  `cam_to_label`, `ignore_img_box` and both `propagte_*` never read device memory on the
host.  The two `refine_*` functions size a compact channel stack: they make ONE device-to-host read per call (the class labels,
together with img_box when that is a CUDA tensor) and none when the caller names the present classes with `keys=[[class ids],
...]`, as `WeCLIP.forward(labels=...)` does.

`cam_to_fg_bg_label` is absent on purpose: no script of the reference imports it, and it is a loop over `crf_inference_label`,
whose parity with pydensecrf is unpinned."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F


def get_mask_by_radius(h=20, w=20, radius=8, device="cpu"):
    """(hw, hw) 0/1 mask of token pairs within a Chebyshev window of `radius`."""
    idx = torch.arange(h * w, device=device)
    yy, xx = idx // w, idx % w
    m = ((yy[:, None] - yy[None]).abs() <= radius) & ((xx[:, None] - xx[None]).abs() <= radius)
    return m.to(torch.float32)


def cams_to_affinity_label(cam_label, mask=None, ignore_index=255):
    b, h, w = cam_label.shape
    r = F.interpolate(cam_label.unsqueeze(1).float(), size=[h // 16, w // 16], mode="nearest")
    lab = r.reshape(b, 1, -1)
    aff = (lab.transpose(1, 2) == lab).long()
    ign = lab == ignore_index
    bad = ign | ign.transpose(1, 2)
    if mask is not None:
        bad = bad | (torch.as_tensor(mask, device=cam_label.device)[None] == 0)
    aff[bad] = ignore_index
    return aff


# ---------------------------------------------------------------------------------------------------------------------
def _L():
    from .. import _lib
    _lib.require_gpu()
    return _lib


def _f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a CUDA tensor (this package needs the GPU; there is no CPU path)")
    return t.detach().float().contiguous()


def _upload_i32(rows, device):
    """A small host table -> int32 device tensor through pinned memory: no host synchronisation."""
    return torch.tensor(rows, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def _box_rows(img_box, B):
    """img_box as a device (B, 4) int32 tensor or, from the host, a list of B rows of 4 ints."""
    if isinstance(img_box, torch.Tensor):
        if tuple(img_box.shape) != (B, 4):
            raise RuntimeError(f"img_box must have shape ({B}, 4), got {tuple(img_box.shape)}")
        return img_box if img_box.is_cuda else [[int(v) for v in r] for r in img_box.tolist()]
    rows = list(img_box)
    if len(rows) != B:
        raise RuntimeError(f"img_box must have {B} rows, got {len(rows)}")
    if rows and all(isinstance(r, torch.Tensor) and r.is_cuda for r in rows):
        return _box_rows(torch.stack([r.reshape(-1) for r in rows]), B)
    out = [[int(v) for v in r] for r in rows]
    if any(len(r) != 4 for r in out):
        raise RuntimeError("img_box rows must be (y0, y1, x0, x1)")
    return out


def _box_device(img_box, B, device):
    rows = _box_rows(img_box, B)
    if isinstance(rows, torch.Tensor):
        return rows.to(torch.int32).contiguous()
    return _upload_i32(rows, device)


def _slice_bounds(row, H, W):
    y0, y1, _ = slice(row[0], row[1]).indices(H)
    x0, x1, _ = slice(row[2], row[3]).indices(W)
    return y0, max(y1, y0), x0, max(x1, x0)


def _cls(cls_label, B, C, name="cls_label"):
    c = _f32(cls_label, name)
    if tuple(c.shape) != (B, C):
        raise RuntimeError(f"{name} must have shape ({B}, {C}), got {tuple(c.shape)}")
    return c


def cam_to_label(cam, cls_label, img_box=None, ignore_mid=False, cfg=None):
    """reference utils/camutils.py:8-28.  Without `img_box`: the int64 label (B,H,W) = 1 + argmax_c cls_label * cam, 0 where the
    maximum is <= cfg.cam.bkg_score.  With `img_box`: (valid_cam f32 (B,C,H,W) = cls_label * cam, pseudo_label int64); first the
    bkg_score threshold, then, if `ignore_mid`, ignore_index where the maximum is <= high_thre and 0 where it is <= low_thre,
    then ignore_index outside the box.  On ties the lowest class index wins.  One kernel, no host synchronisation."""
    L = _L()
    cam = _f32(cam, "cam")
    if cam.dim() != 4:
        raise RuntimeError(f"cam must be (B, C, H, W), got {tuple(cam.shape)}")
    B, C, H, W = cam.shape
    cls = _cls(cls_label, B, C)
    label = torch.empty(B, H, W, device=cam.device, dtype=torch.int64)
    box = valid = None
    hi = lo = 0.0
    if img_box is not None:
        box = _box_device(img_box, B, cam.device)
        valid = torch.empty_like(cam)
        if ignore_mid:
            hi, lo = float(cfg.cam.high_thre), float(cfg.cam.low_thre)
    ignore = int(cfg.dataset.ignore_index) if img_box is not None else 255
    L.lib().wc_cam_to_label(L.ptr(cam, torch.float32, "cam"), L.ptr(cls), L.ptr(box), L.ptr(label), L.ptr(valid), B, C, H, W,
                            float(cfg.cam.bkg_score), hi, lo, 1 if ignore_mid else 0, ignore, L.stream())
    if img_box is None:
        return label
    return valid, label


def ignore_img_box(label, img_box, ignore_index):
    """reference utils/camutils.py:30-37: `label` (B,H,W), int64 or float32, with `ignore_index` outside each image's box; the
    dtype is kept.  Other dtypes raise.  One kernel, no host synchronisation."""
    L = _L()
    if not isinstance(label, torch.Tensor) or not label.is_cuda:
        raise RuntimeError("label: expected a CUDA tensor (this package needs the GPU; there is no CPU path)")
    if label.dtype not in (torch.int64, torch.float32):
        raise RuntimeError(f"ignore_img_box: label must be int64 or float32, got {label.dtype}")
    if label.dim() != 3:
        raise RuntimeError(f"label must be (B, H, W), got {tuple(label.shape)}")
    label = label.detach().contiguous()
    B, H, W = label.shape
    box = _box_device(img_box, B, label.device)
    out = torch.empty_like(label)
    L.lib().wc_box_ignore(L.ptr(label), L.ptr(box), L.ptr(out), B, H, W, 1 if label.dtype == torch.float32 else 0,
                          int(ignore_index), L.stream())
    return out


# ---------------------------------------------------------------------------------------------------------------------
def _aff_propagate(aff, cams, mask=None, cls=None, bkg_score=0.0, with_bkg=False):
    """The random walk behind both `propagte_*` functions (C ABI wc_aff_propagate, registered as
    torch.ops.weclip.aff_propagate): aff (B,n,n), cams (B,C,n), mask (n,n) or None, cls (B,C) or None -> (B,C+with_bkg,n) f32."""
    L = _L()
    aff, cams = _f32(aff, "aff"), _f32(cams, "cams")
    if aff.dim() != 3 or aff.shape[1] != aff.shape[2] or cams.dim() != 3 or cams.shape[0] != aff.shape[0] or cams.shape[2] != aff.shape[1]:
        raise RuntimeError(f"aff_propagate: aff {tuple(aff.shape)} must be (B, n, n) and cams {tuple(cams.shape)} (B, C, n)")
    B, C, n = cams.shape
    if mask is not None:
        mask = _f32(torch.as_tensor(mask), "mask")
        if tuple(mask.shape) != (n, n):
            raise RuntimeError(f"aff_propagate: mask must be ({n}, {n}), got {tuple(mask.shape)}")
    if with_bkg:
        if cls is None:
            raise RuntimeError("aff_propagate: with_bkg needs the class labels")
        cls = _cls(cls, B, C, "cls_labels")
    else:
        cls = None
    nf = ctypes.c_long()
    L.lib().wc_aff_propagate_workspace_floats(B, n, C, 1 if with_bkg else 0, ctypes.byref(nf))
    ws = torch.empty(nf.value, device=aff.device, dtype=torch.float32)
    out = torch.empty(B, C + (1 if with_bkg else 0), n, device=aff.device, dtype=torch.float32)
    L.lib().wc_aff_propagate(L.ptr(aff, torch.float32, "aff"), L.ptr(mask), L.ptr(cams), L.ptr(cls), L.ptr(out), L.ptr(ws), B, n, C,
                             float(bkg_score), 1 if with_bkg else 0, L.stream())
    return out


def _walk(cams, aff, mask, cls, bkg_score, with_bkg):
    if not isinstance(cams, torch.Tensor) or cams.dim() != 4:
        raise RuntimeError("cams must be a (B, C, h, w) tensor")
    if aff is None:
        raise RuntimeError("aff is required")
    b, c, h, w = cams.shape
    out = _aff_propagate(aff, _f32(cams, "cams").reshape(b, c, h * w), mask, cls, bkg_score, with_bkg)
    return out.reshape(b, out.shape[1], h, w)


def propagte_aff_cam(cams, aff=None, mask=None):
    """reference utils/camutils.py:249-275: out[b,k,j] = sum_i cams[b,k,i] A[b,i,j] / (sum_i A[b,i,j] + 1e-4) with
    A = (aff * [mask != 0])^2 -> f32 (B,C,h,w).  The caller's `aff` is left as it is (the reference zeroes it in place where the
    mask is 0, which is why its callers pass `aff.clone()`: here the clone is not needed).  No host synchronisation."""
    return _walk(cams, aff, mask, None, 0.0, False)


def propagte_aff_cam_with_bkg(cams, aff=None, mask=None, cls_labels=None, bkg_score=None):
    """reference utils/camutils.py:277-317: the same walk (eps = 1e-1) of the soft-max over [bkg_score, the present classes'
    CAMs] -> f32 (B,C+1,h,w); the rows of absent classes are 0.  `cls_labels` (B,C) is read inside the kernels as a mask: no
    `nonzero`, no host synchronisation.  The caller's `aff` is left as it is (see propagte_aff_cam)."""
    if cls_labels is None or bkg_score is None:
        raise RuntimeError("propagte_aff_cam_with_bkg needs cls_labels and bkg_score")
    return _walk(cams, aff, mask, cls_labels, float(bkg_score), True)


# ---------------------------------------------------------------------------------------------------------------------
def _present(labels, keys, B, C, extra=None):
    """Per image the ascending list of the channels whose label is non-zero.  From `keys` when given (no device read);
    otherwise ONE device-to-host read of the label matrix, with `extra` (a CUDA tensor) riding along; returns (keys, extra)."""
    if keys is not None:
        keys = [sorted({int(k) for k in row}) for row in keys]
        if len(keys) != B or any(k < 0 or k >= C for row in keys for k in row):
            raise RuntimeError(f"keys must be {B} lists of channel indices in [0, {C})")
        if extra is not None:
            extra = extra.cpu()
        return keys, extra
    if tuple(labels.shape) != (B, C):
        raise RuntimeError(f"the class labels must have shape ({B}, {C}), got {tuple(labels.shape)}")
    flat = (labels.detach() != 0).to(torch.int32).reshape(-1)
    if extra is not None:
        flat = torch.cat([flat, extra.to(torch.int32).reshape(-1)])
    host = flat.cpu()                                          # the one read
    present = host[:B * C].reshape(B, C).numpy()
    if extra is not None:
        extra = host[B * C:].reshape(extra.shape)
    return [np.nonzero(present[b])[0].tolist() for b in range(B)], extra


def _bkg_refined_stack(ref_mod, images, cams, keys, cfg, down_scale=2):
    """refine_cams_with_bkg_v2 up to and including the refinement (reference :152-179, :193): the compact soft-max stack
    (B, 2 Kmax, H//s, W//s) -- high-threshold half, then low-threshold half, each image's background + present classes,
    zero-padded -- after ONE `ref_mod(_images, stack)` call.  Returns (stack, meta, Kmax); meta (B, 1 + Kmax) int32 on the
    device: channel count, then label values."""
    from ..resize import bilinear_resize
    L = _L()
    images, cams = _f32(images, "images"), _f32(cams, "cams")
    B, C, H, W = cams.shape
    if images.shape[0] != B or tuple(images.shape[2:]) != (H, W):
        raise RuntimeError(f"images {tuple(images.shape)} and cams {tuple(cams.shape)} do not match")
    h2, w2 = H // down_scale, W // down_scale
    Kmax = 1 + max(len(k) for k in keys)
    meta = _upload_i32([[1 + len(k), 0] + [1 + c for c in k] + [0] * (Kmax - 1 - len(k)) for k in keys], cams.device)
    stack = torch.empty(B, 2 * Kmax, h2, w2, device=cams.device, dtype=torch.float32)
    L.lib().wc_bkg_refine_prep(L.ptr(cams, torch.float32, "cams"), L.ptr(meta), L.ptr(stack), B, C, H, W, h2, w2, Kmax,
                               float(cfg.cam.high_thre), float(cfg.cam.low_thre), L.stream())
    _images = bilinear_resize(images, (h2, w2), align_corners=False)
    return ref_mod(_images, stack), meta, Kmax


def refine_cams_with_bkg_v2(ref_mod=None, images=None, cams=None, cls_labels=None, cfg=None, img_box=None, down_scale=2, keys=None):
    """reference utils/camutils.py:149-198 -> the f32 (B,H,W) label: 1 + class where the high-threshold refinement says so,
    ignore_index where it says background, 0 where the low-threshold one says background too, ignore_index outside the box.

    The reference calls `ref_mod` 2 B times at batch 1; here the two soft-max stacks of all images go through ONE call
    `ref_mod(_images, stack)`, each image's present classes compacted and zero-padded to the batch's largest count.  `ref_mod`
    is called as given and must treat images and channels independently, as `PAR` does (linear per channel, affinities from the
    image alone).  The up-sampled maps are never written: the arg-max is taken while up-sampling.
    `keys=[[class ids], ...]` names each image's present classes and saves the one device-to-host read of `cls_labels`."""
    L = _L()
    if not isinstance(cams, torch.Tensor) or cams.dim() != 4:
        raise RuntimeError("cams must be a (B, C, H, W) tensor")
    B, C, H, W = cams.shape
    keys, _ = _present(cls_labels, keys, B, C)
    stack, meta, Kmax = _bkg_refined_stack(ref_mod, images, cams, keys, cfg, down_scale)
    stack = _f32(stack, "ref_mod output")
    h2, w2 = H // down_scale, W // down_scale
    if tuple(stack.shape) != (B, 2 * Kmax, h2, w2):
        raise RuntimeError(f"ref_mod returned {tuple(stack.shape)}, expected {(B, 2 * Kmax, h2, w2)}")
    box = _box_device(img_box, B, stack.device)
    out = torch.empty(B, H, W, device=stack.device, dtype=torch.float32)
    L.lib().wc_bkg_refine_finish(L.ptr(stack, torch.float32, "stack"), L.ptr(meta), L.ptr(box), L.ptr(out), B, H, W, h2, w2, Kmax,
                                 float(cfg.dataset.ignore_index), L.stream())
    return out


def refine_cams_with_cls_label(ref_mod=None, images=None, labels=None, cams=None, img_box=None, keys=None):
    """reference utils/camutils.py:200-223 -> f32 shaped like `cams` (B,C,H,W): inside each image's box the refinement of the
    channels whose `labels[b, c]` is non-zero, from the box crop of `cams` and the crop of `images` down-sampled to half its size
    (`ref_mod` brings it back to the crop's size); exactly 0 outside the boxes and on absent channels.

    Images whose boxes have one size share one `ref_mod` call (in training most boxes are the whole crop), their channels
    compacted and zero-padded to the group's largest count; `ref_mod` must treat images and channels independently, as `PAR`
    does.  The box sizes shape the launches, so a CUDA `img_box` is read on the host (in the same single read as `labels`);
    with `keys=[[channel ids], ...]` and a host `img_box` there is no read at all."""
    L = _L()
    images, cams = _f32(images, "images"), _f32(cams, "cams")
    if cams.dim() != 4 or images.dim() != 4 or images.shape[0] != cams.shape[0] or images.shape[2:] != cams.shape[2:] or images.shape[1] != 3:
        raise RuntimeError(f"images {tuple(images.shape)} must be (B, 3, H, W) and cams {tuple(cams.shape)} (B, C, H, W)")
    B, C, H, W = cams.shape
    rows = _box_rows(img_box, B)
    keys, extra = _present(labels, keys, B, C, extra=rows if isinstance(rows, torch.Tensor) else None)
    if extra is not None:
        rows = [[int(v) for v in r] for r in extra.tolist()]
    out = torch.zeros_like(cams)
    groups = {}
    for b in range(B):
        y0, y1, x0, x1 = _slice_bounds(rows[b], H, W)
        if not keys[b]:
            continue
        if y1 - y0 < 2 or x1 - x0 < 2:
            raise RuntimeError(f"refine_cams_with_cls_label: the box of image {b} is smaller than 2 x 2: nothing to down-sample")
        groups.setdefault((y1 - y0, x1 - x0), []).append((b, y0, x0))
    table, spans = [], []
    for (hb, wb), members in groups.items():
        Kg = max(len(keys[b]) for b, _, _ in members)
        spans.append((len(table), hb, wb, Kg, len(members)))
        for b, y0, x0 in members:
            table += [b, y0, x0] + keys[b] + [-1] * (Kg - len(keys[b]))
    if not table:
        return out
    meta = _upload_i32(table, cams.device)
    for off, hb, wb, Kg, G in spans:
        m = meta[off:off + G * (3 + Kg)]
        crop = torch.empty(G, Kg, hb, wb, device=cams.device, dtype=torch.float32)
        small = torch.empty(G, 3, hb // 2, wb // 2, device=cams.device, dtype=torch.float32)
        L.lib().wc_box_gather(L.ptr(cams, torch.float32, "cams"), L.ptr(images), ctypes.c_void_p(m.data_ptr()), L.ptr(crop),
                              L.ptr(small), G, B, C, H, W, hb, wb, Kg, L.stream())
        refined = _f32(ref_mod(small, crop), "ref_mod output")
        if tuple(refined.shape) != (G, Kg, hb, wb):
            raise RuntimeError(f"ref_mod returned {tuple(refined.shape)}, expected {(G, Kg, hb, wb)}")
        L.lib().wc_box_scatter(L.ptr(refined, torch.float32, "refined"), ctypes.c_void_p(m.data_ptr()), L.ptr(out), G, B, C, H, W,
                               hb, wb, Kg, L.stream())
    return out


# ---------------------------------------------------------------------------------------------------------------------
def _flip_pair_cam(model, inputs, size):
    """relu(max(cam(x), flip(cam(flip(x))))) at `size`, and the model's affinity output (reference :89-96)."""
    from ..resize import bilinear_resize
    b = inputs.shape[0]
    cam, aff = model(torch.cat([inputs, inputs.flip(-1)], dim=0), cam_only=True)
    cam = bilinear_resize(cam, size, align_corners=False)
    return F.relu(torch.max(cam[:b], cam[b:].flip(-1))), aff


def _multi_scale(model, inputs, scales):
    from ..resize import bilinear_resize
    _L()
    if not inputs.is_cuda:
        raise RuntimeError("inputs: expected a CUDA tensor (this package needs the GPU; there is no CPU path)")
    b, c, h, w = inputs.shape
    with torch.no_grad():
        cam, aff = _flip_pair_cam(model, inputs, (h, w))
        cam_list, aff_mat = [cam], [aff]
        for s in scales:
            if s != 1.0:
                _inputs = bilinear_resize(inputs, (int(s * h), int(s * w)), align_corners=False)
                cam, aff = _flip_pair_cam(model, _inputs, (h, w))
                cam_list.append(cam)
                aff_mat.append(aff)
        cam = torch.sum(torch.stack(cam_list, dim=0), dim=0)
        cam = cam - cam.amin(dim=(2, 3), keepdim=True)
        cam = cam / (cam.amax(dim=(2, 3), keepdim=True) + 1e-5)
    return cam, aff_mat


def multi_scale_cam(model, inputs, scales):
    """reference utils/camutils.py:85-113: the sum over the scales of the flip-maximum CAMs, min-max normalised per channel to
    [0, 1].  `model` is any callable with `model(x, cam_only=True) -> (cam, aff)`; its forward is all of the time, the rest is
    the package's `bilinear_resize` and elementwise ops."""
    return _multi_scale(model, inputs, scales)[0]


def multi_scale_cam_with_aff_mat(model, inputs, scales):
    """reference utils/camutils.py:115-147: (cam, aff_mat[np.argmax(scales)]).  As in the reference the index points into the
    list of affinity outputs, which holds the scale-1 entry first and then one entry per scale `s != 1.0` in the order given --
    NOT one entry per element of `scales`.  With scales (1.0, 0.5, 1.5) the list has three entries and index 2 is the 1.5
    run; with (0.5, 1.0, 1.5) it is the same list and the same entry; a `scales` whose largest element sits at a position past
    the end of that list, such as (0.5, 1.0, 1.0, 1.5), raises IndexError exactly as the reference does."""
    cam, aff_mat = _multi_scale(model, inputs, scales)
    return cam, aff_mat[np.argmax(scales)]
