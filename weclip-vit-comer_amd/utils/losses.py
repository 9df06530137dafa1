"""Loss functions of the reference (utils/losses.py:11-22 get_aff_loss; scripts/dist_clip_voc.py:105-113 get_seg_loss) in
stock PyTorch-ROCm ops, their fused HIP forms, and the dense energy loss (utils/losses.py:35-116:
get_energy_loss, DenseEnergyLossFunction, DenseEnergyLoss) on the GPU (csrc/energy.hip), with its training-step form
get_energy_loss_fused (csrc/energy_prep.hip)."""
import torch
import torch.nn.functional as F


def get_aff_loss(inputs, targets):
    pos = targets == 1
    neg = targets == 0
    pos_count = pos.sum() + 1
    neg_count = neg.sum() + 1
    pos_loss = (pos * (1 - inputs)).sum() / pos_count
    neg_loss = (neg * inputs).sum() / neg_count
    return 0.5 * pos_loss + 0.5 * neg_loss, pos_count, neg_count


def get_seg_loss(pred, label, ignore_index=255):
    bg = label.clone()
    bg[label != 0] = ignore_index
    fg = label.clone()
    fg[label == 0] = ignore_index
    return 0.5 * (F.cross_entropy(pred, bg.long(), ignore_index=ignore_index)
                  + F.cross_entropy(pred, fg.long(), ignore_index=ignore_index))


def _one_pass(entry, seg, label, ignore_index, n_sums):
    """The training form of csrc/losses.hip (`entry` = wc_seg_loss_fwd_bwd or wc_ce_loss_fwd_bwd): the loss sums and the
    gradient for an upstream gradient of 1 from one pass over the pixels -- the soft-max of a pixel is formed once, the
    up-sampled logits are never materialised, and there is no host synchronisation (the whole training step can be
    captured in a graph).  Returns (sums, grad)."""
    from .. import _lib as L
    B, nc, h, w = seg.shape
    H, W = label.shape[1:]
    nchunk = 1 if nc <= 32 else (nc + 31) // 32                    # classes go through the kernel in register chunks of 32
    nblk = ((W + 63) // 64) * ((h + 3) // 4) * B * nchunk
    part, sums, tmp = (torch.empty(n, device=seg.device, dtype=torch.float32) for n in (4 * nblk, n_sums, 2 * B * nc * h * W))
    grad = torch.empty_like(seg)
    # the two-term loss counts its background / foreground labels first: 2 x 1024 block partials
    cnt = [torch.empty(2048, device=seg.device, dtype=torch.float32)] if entry == "wc_seg_loss_fwd_bwd" else []
    getattr(L.lib(), entry)(L.ptr(seg, torch.float32, "seg"), L.ptr(label, torch.int64, "label"),
                            *[L.ptr(t) for t in cnt + [part, sums, tmp, grad]], B, nc, h, w, H, W, int(ignore_index), L.stream())
    return sums, grad


class _OnePassLossFn(torch.autograd.Function):
    """A loss whose forward saved its gradient for an upstream gradient of 1 (`_one_pass`): backward only scales it."""

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


class _SegLossFn(_OnePassLossFn):
    """get_seg_loss(F.interpolate(seg, (H,W), bilinear), label) without materialising the up-sampled logits
    (csrc/losses.hip): wc_seg_loss_fwd_bwd when a gradient is requested, else the forward-only wc_seg_loss_fwd."""

    @staticmethod
    def forward(ctx, seg, label, ignore_index):
        from .. import _lib as L
        seg = seg.float().contiguous()
        label = label.long().contiguous()
        if ctx.needs_input_grad[0]:
            sums, grad = _one_pass("wc_seg_loss_fwd_bwd", seg, label, ignore_index, 8)
            ctx.save_for_backward(grad)
            return sums[4].clone()
        B, nc, h, w = seg.shape
        H, W = label.shape[1:]
        nblk = ((W + 63) // 64) * ((H + 3) // 4) * B
        part = torch.empty(nblk * 4, device=seg.device, dtype=torch.float32)
        sums = torch.empty(8, device=seg.device, dtype=torch.float32)
        L.lib().wc_seg_loss_fwd(L.ptr(seg, torch.float32, "seg"), L.ptr(label, torch.int64, "label"), L.ptr(part),
                                L.ptr(sums), B, nc, h, w, H, W, int(ignore_index), L.stream())
        # mean over an empty set is NaN in F.cross_entropy too (0/0); the scalar tail is computed by the reduce kernel
        return sums[4].clone()


def get_seg_loss_fused(seg_lowres, label, ignore_index=255):
    """== get_seg_loss(F.interpolate(seg_lowres, label.shape[1:], 'bilinear', align_corners=False), label)."""
    return _SegLossFn.apply(seg_lowres, label, ignore_index)


def _ce_check(seg, label):
    """Host-side checks of get_ce_loss_fused, before anything is allocated or launched."""
    if not isinstance(seg, torch.Tensor) or not isinstance(label, torch.Tensor):
        raise TypeError("get_ce_loss_fused: seg and label must be tensors")
    if seg.dim() != 4:
        raise ValueError(f"get_ce_loss_fused: seg must be (B, nc, h, w), got shape {tuple(seg.shape)}")
    if label.dim() != 3:
        raise ValueError(f"get_ce_loss_fused: label must be (B, H, W), got shape {tuple(label.shape)}")
    if not seg.dtype.is_floating_point:
        raise TypeError(f"get_ce_loss_fused: seg must be a floating-point tensor, got {seg.dtype}")
    if label.dtype.is_floating_point or label.dtype.is_complex or label.dtype == torch.bool:
        raise TypeError(f"get_ce_loss_fused: label must be an integer tensor, got {label.dtype}")
    if seg.shape[0] != label.shape[0]:
        raise ValueError(f"get_ce_loss_fused: batch sizes differ (seg {seg.shape[0]}, label {label.shape[0]})")
    if not 1 <= seg.shape[1] <= 128:
        raise ValueError(f"get_ce_loss_fused: 1 <= nc <= 128, got {seg.shape[1]}")
    if min(seg.shape) == 0 or min(label.shape) == 0:
        raise ValueError("get_ce_loss_fused: empty input")
    if seg.device != label.device:
        raise ValueError(f"get_ce_loss_fused: seg on {seg.device}, label on {label.device}")


class _CELossFn(_OnePassLossFn):
    """F.cross_entropy(F.interpolate(seg, label.shape[1:], 'bilinear', align_corners=False), label, ignore_index) without
    materialising the up-sampled logits (csrc/losses.hip wc_ce_loss_fwd_bwd).  `last_sums` keeps
    [loss, 1/N_valid, N_valid, N_bad] of the last call on the device."""

    @staticmethod
    def forward(ctx, seg, label, ignore_index):
        sums, grad = _one_pass("wc_ce_loss_fwd_bwd", seg.float().contiguous(), label.long().contiguous(), ignore_index, 4)
        ctx.save_for_backward(grad)
        _CELossFn.last_sums = sums
        return sums[0].clone()


def get_ce_loss_fused(seg_lowres, label, ignore_index=255):
    """== F.cross_entropy(F.interpolate(seg_lowres, label.shape[1:], mode='bilinear', align_corners=False), label,
    ignore_index=ignore_index): the supervised variant's loss (our choice: the reference ships no training script for it).
    seg_lowres (B, nc, h, w) floating point, 1 <= nc <= 128; label (B, H, W) integer at any H x W.  All pixels ignored: the
    loss is NaN (as torch) and the gradient is zero (as torch).  A label outside [0, nc) that is not ignore_index is treated
    as ignored (torch raises instead); `ce_loss_counts()` reads how many there were in the last call."""
    _ce_check(seg_lowres, label)
    return _CELossFn.apply(seg_lowres, label, ignore_index)


def ce_loss_counts():
    """(N_valid, N_bad) of the last get_ce_loss_fused call as device floats (reading them synchronises)."""
    s = getattr(_CELossFn, "last_sums", None)
    if s is None:
        raise RuntimeError("get_ce_loss_fused has not run yet")
    return s[2], s[3]


class _AffLossFn(torch.autograd.Function):
    """get_aff_loss(attn_pred, cams_to_affinity_label(cam_label, radius mask)) in one pass (csrc/losses.hip),
    without the (B, hw, hw) label / mask tensors."""

    @staticmethod
    def forward(ctx, attn_pred, cam_label, radius, ignore_index):
        from .. import _lib as L
        ap = attn_pred.float().contiguous()
        lab = cam_label.long().contiguous()
        B, hw, _ = ap.shape
        H, W = lab.shape[1:]
        h, w = H // 16, W // 16
        if h * w != hw:
            raise RuntimeError("attn_pred does not match the 1/16 token grid of the labels")
        part = torch.empty(4 * B * ((hw + 7) // 8), device=ap.device, dtype=torch.float32)
        sums = torch.empty(8, device=ap.device, dtype=torch.float32)
        L.lib().wc_aff_loss_fwd(L.ptr(ap, torch.float32, "attn_pred"), L.ptr(lab, torch.int64, "cam_label"), L.ptr(part),
                                L.ptr(sums), B, h, w, H, W, int(radius), int(ignore_index), L.stream())
        ctx.save_for_backward(lab, sums)
        ctx.meta = (B, h, w, H, W, int(radius), int(ignore_index))
        return sums[4].clone()

    @staticmethod
    def backward(ctx, g):
        from .. import _lib as L
        lab, sums = ctx.saved_tensors
        B, h, w, H, W, radius, ignore = ctx.meta
        coef = sums[5:7] * g           # (-0.5 / (n_pos + 1), 0.5 / (n_neg + 1)) from the forward reduce kernel
        dap = torch.empty(B, h * w, h * w, device=lab.device, dtype=torch.float32)
        L.lib().wc_aff_loss_bwd(L.ptr(lab), L.ptr(coef, torch.float32, "coef"), L.ptr(dap), B, h, w, H, W, radius, ignore,
                                L.stream())
        return dap, None, None, None


def get_aff_loss_fused(attn_pred, cam_label, radius=8, ignore_index=255):
    """== get_aff_loss(attn_pred, cams_to_affinity_label(cam_label, get_mask_by_radius(h, w, radius)))[0]."""
    return _AffLossFn.apply(attn_pred, cam_label, radius, ignore_index)


# ---------------------------------------------------------------------------------------------------------------------
# Dense energy (regularised CRF) loss: reference utils/losses.py:35-116 with the `bilateralfilter_batch` call as the exact
# all-pairs sum on the GPU (csrc/energy.hip, C ABI `wc_energy_*` / `wc_dense_energy_*`).  The
# reference's extension (a permutohedral lattice) is not shipped with it; parity with the lattice is unpinned.
# bilateral="lattice" (opt-in, csrc/energy_lattice.hip) is our own lattice in the filter's place.
def _energy_workspace(N, K, H, W, device):
    import ctypes
    from .. import _lib as L
    n = ctypes.c_long()
    L.lib().wc_energy_workspace_floats(N, K, H, W, ctypes.byref(n))
    return torch.empty(n.value, device=device, dtype=torch.float32)


def _energy_shapes(images, segs, who):
    if images.dim() != 4 or images.shape[1] != 3:
        raise RuntimeError(f"{who}: images must be (N, 3, H, W), got {tuple(images.shape)}")
    if segs.dim() != 4 or segs.shape[0] != images.shape[0] or segs.shape[2:] != images.shape[2:]:
        raise RuntimeError(f"{who}: segmentations {tuple(segs.shape)} do not match images {tuple(images.shape)}")
    return segs.shape


BILATERAL_MODES = ("exact", "lattice")


def _bilateral_mode(bilateral, who):
    """Checks the filter's name before anything is allocated: "exact" (the all-pairs sum, the default everywhere) or "lattice"
    (the permutohedral lattice, csrc/energy_lattice.hip)."""
    if bilateral not in BILATERAL_MODES:
        raise ValueError(f"{who}: bilateral must be 'exact' or 'lattice', got {bilateral!r}")
    return bilateral


def _lattice_workspace(N, K, H, W, device, cache=None):
    """(lat, ws) byte tensors of the wc_*_lattice energy entries, sized by wc_energy_lattice_workspace_bytes alone.  `cache`
    (a dict, or None): one pair per (N, K, H, W, device), allocated on the first request and reused from then on."""
    import ctypes
    from .. import _lib as L
    key = (N, K, H, W, str(device))
    if cache is not None and key in cache:
        return cache[key]
    a, b = ctypes.c_long(), ctypes.c_long()
    L.lib().wc_energy_lattice_workspace_bytes(N, K, H, W, ctypes.byref(a), ctypes.byref(b))
    pair = tuple(torch.empty(n.value, device=device, dtype=torch.uint8) for n in (a, b))
    if cache is not None:
        cache[key] = pair
    return pair


def lattice_vertex_counts(lat, N):
    """(flag, M (N,)) of the last lattice call on the structure `lat`: flag != 0 when a colour lay outside [0, 256] and was
    clamped for the key; M the number of lattice vertices of every image.  Reading them synchronises; the entries never do."""
    meta = lat[:4 * (16 + N)].view(torch.int32)
    return meta[1], meta[16:16 + N]


def bilateral_filter_batch(images, segs, sigma_rgb, sigma_xy, bilateral="exact", workspace=None):
    """AS (N, K, H, W) f32 on the device: AS(n, k, i) = sum_j exp(-|p_i - p_j|^2 / (2 sigma_xy^2) - |I_n,i - I_n,j|^2 /
    (2 sigma_rgb^2)) segs(n, k, j) over every pixel j of image n (j = i included): what the reference's
    `bilateralfilter_batch(images, segs, AS, N, K, H, W, sigma_rgb, sigma_xy)` (losses.py:75) approximates.  images
    (N, 3, H, W) on the 0..255 scale; segs may be signed.  No autograd.
    bilateral="lattice": the same call with the permutohedral lattice as the filter (un-normalised, what the reference's extension
    is; about half the exact AS); workspace: a (lat, ws) pair of `_lattice_workspace` to use instead of allocating one."""
    from .. import _lib as L
    _bilateral_mode(bilateral, "bilateral_filter_batch")
    L.require_gpu()
    N, K, H, W = _energy_shapes(images, segs, "bilateral_filter_batch")
    img = images.detach().float().contiguous()
    seg = segs.detach().float().contiguous()
    AS = torch.empty_like(seg)
    if bilateral == "lattice":
        lat, ws = workspace or _lattice_workspace(N, K, H, W, seg.device)
        L.lib().wc_bilateral_filter_batch_lattice(L.ptr(img, torch.float32, "images"), L.ptr(seg, torch.float32, "segs"), L.ptr(AS),
                                                  L.ptr(lat), L.ptr(ws), N, K, H, W, float(sigma_rgb), float(sigma_xy), L.stream())
        return AS
    ws = _energy_workspace(N, K, H, W, seg.device)
    L.lib().wc_bilateral_filter_batch(L.ptr(img, torch.float32, "images"), L.ptr(seg, torch.float32, "segs"), L.ptr(AS), L.ptr(ws),
                                      N, K, H, W, float(sigma_rgb), float(sigma_xy), L.stream())
    return AS


def dense_energy_forward(images, segs, sigma_rgb, sigma_xy, rois, unlabel_region, bilateral="exact", workspace=None):
    """(loss (1,), A (N, K, H, W) = Gate * AS, Gate (N, H, W)) of DenseEnergyLossFunction.forward, all on the device.
    bilateral, workspace: as in `bilateral_filter_batch`."""
    from .. import _lib as L
    _bilateral_mode(bilateral, "DenseEnergyLossFunction")
    L.require_gpu()
    N, K, H, W = _energy_shapes(images, segs, "DenseEnergyLossFunction")
    if tuple(rois.shape) != (N, H, W) or tuple(unlabel_region.shape) != (N, H, W):
        raise RuntimeError(f"DenseEnergyLossFunction: ROIs {tuple(rois.shape)} / unlabel_region {tuple(unlabel_region.shape)} "
                           f"must be {(N, H, W)}")
    img = images.detach().float().contiguous()
    seg = segs.detach().float().contiguous()
    roi = rois.detach().float().contiguous()                 # the caller's ROIs is left as it is (the reference unsqueezes it)
    unl = (unlabel_region != 0).contiguous().view(torch.uint8)
    A = torch.empty_like(seg)
    gate = torch.empty_like(roi)
    loss = torch.empty(1, device=seg.device, dtype=torch.float32)
    if bilateral == "lattice":
        lat, ws = workspace or _lattice_workspace(N, K, H, W, seg.device)
        L.lib().wc_dense_energy_fwd_lattice(L.ptr(img, torch.float32, "images"), L.ptr(seg, torch.float32, "segmentations"),
                                            L.ptr(roi, torch.float32, "ROIs"), L.ptr(unl, torch.uint8, "unlabel_region"), L.ptr(A),
                                            L.ptr(gate), L.ptr(loss), L.ptr(lat), L.ptr(ws), N, K, H, W, float(sigma_rgb),
                                            float(sigma_xy), L.stream())
        return loss, A, gate
    ws = _energy_workspace(N, K, H, W, seg.device)
    L.lib().wc_dense_energy_fwd(L.ptr(img, torch.float32, "images"), L.ptr(seg, torch.float32, "segmentations"),
                                L.ptr(roi, torch.float32, "ROIs"), L.ptr(unl, torch.uint8, "unlabel_region"), L.ptr(A), L.ptr(gate),
                                L.ptr(loss), L.ptr(ws), N, K, H, W, float(sigma_rgb), float(sigma_xy), L.stream())
    return loss, A, gate


def dense_energy_backward(grad_output, A, rois):
    """grad_segmentations = -2 * grad_output * A * ROI / N (losses.py:87-91): one elementwise kernel, grad_output read on the
    device.  Computed and returned in f32 like the forward, which casts its inputs up; for half-precision segmentations
    autograd casts the gradient back."""
    from .. import _lib as L
    L.require_gpu()
    if A.dim() != 4 or tuple(rois.shape) != (A.shape[0],) + tuple(A.shape[2:]):
        raise RuntimeError(f"dense_energy_backward: A {tuple(A.shape)} and ROIs {tuple(rois.shape)} do not match")
    N, K, H, W = A.shape
    g = grad_output.detach().float().reshape(-1)[:1].contiguous()
    A = A.contiguous()
    roi = rois.detach().float().contiguous()
    out = torch.empty_like(A)
    L.lib().wc_dense_energy_bwd(L.ptr(A, torch.float32, "A"), L.ptr(roi, torch.float32, "ROIs"), L.ptr(g, torch.float32, "grad"),
                                L.ptr(out), N, K, H, W, L.stream())
    return out


class DenseEnergyLossFunction(torch.autograd.Function):
    """loss (1,) = -(1/N) sum S * Gate * AS with S = segmentations * ROIs, AS the bilateral filter of S and
    Gate = ROIs - max_k segmentations, 1 where unlabelled, 0 where negative (reference losses.py:52-91; argument order as
    there).  backward gives -2 * grad * Gate * AS * ROIs / N to `segmentations` and nothing else: the Gate is held constant
    and the factor 2 stands for the kernel's symmetry, as in the reference -- not the true derivative where the Gate varies.
    An optional seventh argument, bilateral ("exact", the default, or "lattice"), chooses the filter; with the lattice the
    factor 2 is an approximation in a second sense, because that filter is not a symmetric matrix."""

    @staticmethod
    def forward(ctx, images, segmentations, sigma_rgb, sigma_xy, ROIs, unlabel_region, *bilateral):
        if len(bilateral) > 1:
            raise TypeError("DenseEnergyLossFunction: at most one argument (bilateral) after unlabel_region")
        loss, A, _ = dense_energy_forward(images, segmentations, sigma_rgb, sigma_xy, ROIs, unlabel_region, *bilateral)
        ctx.save_for_backward(A, ROIs)
        ctx.n_extra = len(bilateral)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        A, rois = ctx.saved_tensors
        return (None, dense_energy_backward(grad_output, A, rois), None, None, None, None) + (None,) * ctx.n_extra


class DenseEnergyLoss(torch.nn.Module):
    """reference losses.py:94-116: the loss at `scale_factor` of the input size, times `weight`.  Images, ROIs and the label
    map are resampled nearest, the segmentations bilinear (align_corners=False); a label of 255 marks a pixel unlabelled;
    sigma_xy shrinks with the image.  bilateral="lattice" (ours; default "exact"): the permutohedral-lattice filter; its AS is
    about half the exact one, so a `weight` tuned for one mode does not carry over to the other."""

    def __init__(self, weight, sigma_rgb, sigma_xy, scale_factor, bilateral="exact"):
        super().__init__()
        self.bilateral = _bilateral_mode(bilateral, "DenseEnergyLoss")
        self.weight, self.scale_factor = weight, scale_factor
        self.sigma_rgb, self.sigma_xy = sigma_rgb, sigma_xy
        self.workspace_cache = None          # a dict here makes get_energy_loss_fused keep its lattice workspaces

    def _resample(self, x, mode="nearest"):
        kw = dict(align_corners=False) if mode == "bilinear" else {}
        return F.interpolate(x, scale_factor=self.scale_factor, mode=mode, **kw)

    def forward(self, images, segmentations, ROIs, seg_label):
        unlabelled = self._resample(seg_label).long().eq(255)[:, 0]
        rois = self._resample(ROIs[:, None])[:, 0]
        extra = () if self.bilateral == "exact" else (self.bilateral,)
        energy = DenseEnergyLossFunction.apply(self._resample(images), self._resample(segmentations, "bilinear"), self.sigma_rgb,
                                               self.sigma_xy * self.scale_factor, rois, unlabelled, *extra)
        return self.weight * energy

    def extra_repr(self):
        # nn.Module prints this between the brackets: the order and names are the reference's
        fields = ("sigma_rgb", "sigma_xy", "weight", "scale_factor")
        if self.bilateral != "exact":
            fields += ("bilateral",)
        return ", ".join(f"{k}={getattr(self, k)}" for k in fields)


def get_energy_loss(img, logit, label, img_box, loss_layer, mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375]):
    """reference losses.py:35-50: soft-max, crop mask from img_box rows (y0, y1, x0, x1), de-normalised image, loss_layer."""
    pred_prob = F.softmax(logit, dim=1)
    crop_mask = torch.zeros_like(pred_prob[:, 0])
    for idx, coord in enumerate(img_box):
        crop_mask[idx, int(coord[0]):int(coord[1]), int(coord[2]):int(coord[3])] = 1
    _img = torch.stack([img[:, c] * std[c] + mean[c] for c in range(3)], dim=1)
    return loss_layer(_img, pred_prob, crop_mask, label.type(torch.uint8).unsqueeze(1))


# ---------------------------------------------------------------------------------------------------------------------
# The same loss as a term of the training step (csrc/energy_prep.hip): from the low-resolution head
# output to a low-resolution gradient around the unchanged filter, with no full-resolution (N, K, H, W) tensor and no host
# read of a device img_box, so the step that contains it can be captured in a graph.
_ENERGY_SCALES = {1.0: 0, 0.5: 1, 0.25: 2}         # scale_factor = 2^-e: ATen's nearest / bilinear sources are exact
_ENERGY_MAX_HW = 640 * 640                        # the filter's limit on the scaled size


def _energy_term_check(img, seg, label, img_box, weight, sigma_rgb, sigma_xy, scale_factor, mean, std):
    """Host-side checks of get_energy_loss_fused, before anything is allocated or launched.  Returns e (scale_factor = 2^-e)."""
    who = "get_energy_loss_fused"
    if not all(isinstance(t, torch.Tensor) for t in (img, seg, label)):
        raise TypeError(f"{who}: img, seg_lowres and label must be tensors")
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"{who}: img must be (N, 3, H, W), got shape {tuple(img.shape)}")
    if seg.dim() != 4:
        raise ValueError(f"{who}: seg_lowres must be (N, K, h, w), got shape {tuple(seg.shape)}")
    if label.dim() != 3:
        raise ValueError(f"{who}: label must be (N, H, W), got shape {tuple(label.shape)}")
    if not img.dtype.is_floating_point or not seg.dtype.is_floating_point:
        raise TypeError(f"{who}: img and seg_lowres must be floating-point tensors, got {img.dtype} and {seg.dtype}")
    if label.dtype.is_floating_point or label.dtype.is_complex or label.dtype == torch.bool:
        raise TypeError(f"{who}: label must be an integer tensor, got {label.dtype}")
    if not (img.shape[0] == seg.shape[0] == label.shape[0]):
        raise ValueError(f"{who}: batch sizes differ (img {img.shape[0]}, seg_lowres {seg.shape[0]}, label {label.shape[0]})")
    if tuple(img.shape[2:]) != tuple(label.shape[1:]):
        raise ValueError(f"{who}: img {tuple(img.shape[2:])} and label {tuple(label.shape[1:])} differ in size")
    if not 1 <= seg.shape[1] <= 128:
        raise ValueError(f"{who}: 1 <= K <= 128, got {seg.shape[1]}")
    if min(img.shape) == 0 or min(seg.shape) == 0:
        raise ValueError(f"{who}: empty input")
    if not (img.device == seg.device == label.device):
        raise ValueError(f"{who}: img on {img.device}, seg_lowres on {seg.device}, label on {label.device}")
    e = _ENERGY_SCALES.get(float(scale_factor))
    if e is None:
        raise ValueError(f"{who}: scale_factor must be 1, 0.5 or 0.25, got {scale_factor} (DenseEnergyLoss serves the others)")
    Hs, Ws = img.shape[2] >> e, img.shape[3] >> e
    if Hs < 1 or Ws < 1 or Hs * Ws > _ENERGY_MAX_HW or img.shape[3] > 8192:
        raise ValueError(f"{who}: the scaled size {Hs} x {Ws} must be 1 .. 640*640 pixels and W <= 8192")
    for name, v in (("weight", weight), ("sigma_rgb", sigma_rgb), ("sigma_xy", sigma_xy)):
        if not isinstance(v, (int, float)) or isinstance(v, bool):
            raise TypeError(f"{who}: loss_layer.{name} must be a number, got {type(v).__name__}")
    if not (sigma_rgb > 0 and sigma_xy > 0):
        raise ValueError(f"{who}: sigmas must be > 0, got sigma_rgb {sigma_rgb}, sigma_xy {sigma_xy}")
    if len(mean) != 3 or len(std) != 3:
        raise ValueError(f"{who}: mean and std must have 3 entries")
    if isinstance(img_box, torch.Tensor):
        if img_box.dtype.is_floating_point or img_box.dtype.is_complex or img_box.dtype == torch.bool:
            raise TypeError(f"{who}: img_box must be an integer tensor, got {img_box.dtype}")
        if img_box.is_cuda and img_box.device != seg.device:
            raise ValueError(f"{who}: img_box on {img_box.device}, seg_lowres on {seg.device}")
        shape = tuple(img_box.shape)
    elif img_box is not None:
        try:
            shape = (len(img_box),) + tuple({len(r) for r in img_box})
        except TypeError:
            raise TypeError(f"{who}: img_box must be None, rows of (y0, y1, x0, x1) or an integer tensor") from None
    if img_box is not None and shape != (img.shape[0], 4):
        raise ValueError(f"{who}: img_box must be ({img.shape[0]}, 4): rows (y0, y1, x0, x1), got {shape}")
    return e


def energy_prep_forward(img, seg, label, box, e, mean, std):
    """wc_energy_prep_fwd: (images_s (N,3,Hs,Ws), P_s (N,K,Hs,Ws), rois_s (N,Hs,Ws), unlabel_u8 (N,Hs,Ws)), the inputs of
    wc_dense_energy_fwd at scale 2^-e.  img, seg f32 and label int64, contiguous, on the device; box None or int32 (N, 4) there."""
    import ctypes
    from .. import _lib as L
    N, K, h, w = seg.shape
    H, W = label.shape[1:]
    Hs, Ws = H >> e, W >> e
    images_s, P_s, rois_s = (torch.empty(N, c, Hs, Ws, device=seg.device, dtype=torch.float32) for c in (3, K, 1))
    rois_s = rois_s[:, 0]
    unl = torch.empty(N, Hs, Ws, device=seg.device, dtype=torch.uint8)
    F3 = ctypes.c_float * 3
    L.lib().wc_energy_prep_fwd(L.ptr(img, torch.float32, "img"), L.ptr(seg, torch.float32, "seg_lowres"), L.ptr(label, torch.int64, "label"),
                               L.ptr(box, torch.int32, "img_box"), F3(*[float(v) for v in mean]), F3(*[float(v) for v in std]),
                               L.ptr(images_s), L.ptr(P_s), L.ptr(rois_s), L.ptr(unl), N, K, h, w, H, W, e, L.stream())
    return images_s, P_s, rois_s, unl


def energy_prep_backward(A, rois_s, seg, coef, size, e):
    """wc_energy_prep_bwd: grad_seg (N,K,h,w) = coef * A * rois_s pulled back through the down-sample by 2^e, the soft-max and the
    up-sample of seg to `size` = (H, W)."""
    import ctypes
    from .. import _lib as L
    N, K, h, w = seg.shape
    H, W = size
    n = ctypes.c_long()
    L.lib().wc_energy_prep_workspace_floats(N, K, h, W, ctypes.byref(n))
    ws = torch.empty(n.value, device=seg.device, dtype=torch.float32)
    grad = torch.empty_like(seg)
    L.lib().wc_energy_prep_bwd(L.ptr(A, torch.float32, "A"), L.ptr(rois_s, torch.float32, "rois_s"), L.ptr(seg, torch.float32, "seg_lowres"),
                               L.ptr(grad), L.ptr(ws), float(coef), N, K, h, w, H, W, e, L.stream())
    return grad


def energy_term(img, seg, label, img_box, weight, sigma_rgb, sigma_xy, scale_factor, mean, std, need_grad=True, bilateral="exact",
                workspace_cache=None):
    """(weight * loss (1,), d(weight * loss) / d seg for an upstream gradient of 1, or None) of get_energy_loss_fused:
    wc_energy_prep_fwd, the filter (wc_dense_energy_fwd, unchanged, or wc_dense_energy_fwd_lattice when bilateral="lattice"),
    wc_energy_prep_bwd.  No host synchronisation.  workspace_cache: a dict that keeps the lattice's workspaces between calls."""
    from .. import _lib as L
    _bilateral_mode(bilateral, "get_energy_loss_fused")
    e = _energy_term_check(img, seg, label, img_box, weight, sigma_rgb, sigma_xy, scale_factor, mean, std)
    L.require_gpu()
    dev = seg.device
    img = img.detach().float().contiguous()
    seg = seg.detach().float().contiguous()
    label = label.long().contiguous()
    box = None
    if img_box is not None:        # a device tensor stays on the device; rows and host tensors are host data
        box = torch.as_tensor(img_box).to(device=dev, dtype=torch.int32).contiguous()
        if box.data_ptr() % 16:
            box = box.clone()
    N, K = seg.shape[:2]
    images_s, P_s, rois_s, unl = energy_prep_forward(img, seg, label, box, e, mean, std)
    Hs, Ws = rois_s.shape[1:]
    A, gate, loss = torch.empty_like(P_s), torch.empty_like(rois_s), torch.empty(1, device=dev, dtype=torch.float32)
    if bilateral == "lattice":
        lat, ws = _lattice_workspace(N, K, Hs, Ws, dev, workspace_cache)
        L.lib().wc_dense_energy_fwd_lattice(L.ptr(images_s), L.ptr(P_s), L.ptr(rois_s), L.ptr(unl), L.ptr(A), L.ptr(gate), L.ptr(loss),
                                            L.ptr(lat), L.ptr(ws), N, K, Hs, Ws, float(sigma_rgb), float(sigma_xy * scale_factor),
                                            L.stream())
    else:
        L.lib().wc_dense_energy_fwd(L.ptr(images_s), L.ptr(P_s), L.ptr(rois_s), L.ptr(unl), L.ptr(A), L.ptr(gate), L.ptr(loss),
                                    L.ptr(_energy_workspace(N, K, Hs, Ws, dev)), N, K, Hs, Ws, float(sigma_rgb),
                                    float(sigma_xy * scale_factor), L.stream())
    grad = energy_prep_backward(A, rois_s, seg, -2.0 * float(weight) / N, label.shape[1:], e) if need_grad else None
    return weight * loss, grad


class _EnergyTermFn(torch.autograd.Function):
    """get_energy_loss_fused: like `_OnePassLossFn`, the forward saves the gradient for an upstream gradient of 1 and the
    backward only scales it."""

    @staticmethod
    def forward(ctx, seg, img, label, img_box, params, mean, std, *opt):
        bilateral = opt[0] if opt else "exact"                 # optional: the filter, then a workspace cache
        workspace_cache = opt[1] if len(opt) > 1 else None
        loss, grad = energy_term(img, seg, label, img_box, *params, mean, std, need_grad=ctx.needs_input_grad[0], bilateral=bilateral,
                                 workspace_cache=workspace_cache)
        ctx.n_in = 7 + len(opt)
        if grad is not None:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g,) + (None,) * (ctx.n_in - 1)


def get_energy_loss_fused(img, seg_lowres, label, img_box, loss_layer, mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375]):
    """== get_energy_loss(img, F.interpolate(seg_lowres, label.shape[1:], mode='bilinear', align_corners=False), label, img_box,
    loss_layer) for a `DenseEnergyLoss` whose scale_factor is 1, 0.5 or 0.25 (any other: ValueError; the stock layer serves
    those), without the up-sampled logits, their soft-max or a full-resolution gradient.  img (N, 3, H, W) normalised,
    seg_lowres (N, K, h, w), 1 <= K <= 128, label (N, H, W) integer; img_box: None (the whole image), rows (y0, y1, x0, x1), or
    an integer tensor (N, 4) on the host or on the device -- a device tensor is never read on the host (rows with 0 <= y0, x0;
    Python's negative slice indices are not emulated).  Returns weight * loss, shape (1,); the Gate is a constant in backward.
    The filter follows loss_layer.bilateral ("exact" when the layer has none)."""
    try:
        params = tuple(getattr(loss_layer, k) for k in ("weight", "sigma_rgb", "sigma_xy", "scale_factor"))
    except AttributeError:
        raise TypeError("get_energy_loss_fused: loss_layer must be a DenseEnergyLoss (weight, sigma_rgb, sigma_xy, scale_factor)") from None
    bilateral = _bilateral_mode(getattr(loss_layer, "bilateral", "exact"), "get_energy_loss_fused")
    if bilateral == "exact":
        return _EnergyTermFn.apply(seg_lowres, img, label, img_box, params, mean, std)
    return _EnergyTermFn.apply(seg_lowres, img, label, img_box, params, mean, std, bilateral, getattr(loss_layer, "workspace_cache", None))
