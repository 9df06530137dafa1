"""`validate` of the reference's training scripts (scripts/dist_clip_voc.py:71-102, dist_clip_coco.py) on the device.

Image by image at each image's own size, as the reference runs it: the model in `mode="val"`, then ONE launch of
`wc_val_pair_hist` (csrc/trainlog.hip) that up-samples the low-resolution logits to the label grid, takes the arg-max and
counts (gt, prediction) and (gt, CAM label) into two int64 device histograms -- the (Hl, Wl) prediction map is never
written and nothing goes to the host per image (the reference moves every prediction, CAM and label map there as int16
numpy, :88-90).  The histograms and the out-of-range flag are read once, at the end of `run`.
"""
import torch

from . import _lib as L
from . import msc_flip
from .utils import evaluate

F32 = torch.float32
_flag = evaluate.range_flag                                # the flag `evaluate.check_predictions_in_range` reads


def val_pair_hist(seg, cam, gt, num_classes, seg_hist, cam_hist=None, flag=None):
    """seg (C,Hs,Ws) f32 logits, cam (Hl,Wl) int64 or None, gt (Hl,Wl) int64; adds into seg_hist / cam_hist (nc,nc) int64:
    seg_hist[gt, argmax_c bilinear(seg)[c]] += 1 and cam_hist[gt, cam] += 1 over the pixels with 0 <= gt < nc.  A prediction
    outside [0, nc) is skipped and raises `flag` (default: the flag of `evaluate.check_predictions_in_range`)."""
    L.require_gpu()
    C, Hs, Ws = seg.shape
    Hl, Wl = gt.shape
    if cam is not None and (cam_hist is None or tuple(cam.shape) != (Hl, Wl)):
        raise RuntimeError("val_pair_hist: cam needs cam_hist and the shape of gt")
    if flag is None:
        flag = _flag(seg.device)
    L.lib().wc_val_pair_hist(L.ptr(seg, F32, "seg"), L.ptr(cam, torch.int64, "cam"), L.ptr(gt, torch.int64, "gt"),
                             L.ptr(seg_hist, torch.int64, "seg_hist"),
                             L.ptr(cam_hist if cam is not None else None, torch.int64, "cam_hist"),
                             L.ptr(flag, torch.int32, "flag"), C, Hs, Ws, Hl, Wl, int(num_classes), L.stream())
    return seg_hist, cam_hist


def label_match_count(seg, label, counts=None):
    """counts int64[2] (overwritten) = [#pixels with argmax_c bilinear(seg)[c] == label, B*H*W]: numerator and denominator
    of the reference's pseudo_seg_mAcc (scripts/dist_clip_voc.py:274-277).  seg (B,C,Hs,Ws) f32, label (B,H,W) int64."""
    L.require_gpu()
    B, C, Hs, Ws = seg.shape
    if label.shape[0] != B or label.dim() != 3:
        raise RuntimeError("label_match_count: label must be (B, H, W) with seg's batch size")
    if counts is None:
        counts = torch.empty(2, device=seg.device, dtype=torch.int64)
    L.lib().wc_label_match_count(L.ptr(seg, F32, "seg"), L.ptr(label, torch.int64, "label"), L.ptr(counts, torch.int64, "counts"),
                                 B, C, Hs, Ws, label.shape[1], label.shape[2], L.stream())
    return counts


def step_pair_hist(seg, label, num_classes, hist, flag=None):
    """seg (B,C,Hs,Ws) f32 logits of a train step, label (B,H,W) int64 ground-truth masks; ADDS into hist (nc,nc) int64:
    hist[label, argmax_c bilinear(seg[b])[c]] += 1 over the pixels with 0 <= label < nc (255 and any other value are skipped).
    A prediction outside [0, nc) is skipped and raises `flag` (default: the flag of `evaluate.check_predictions_in_range`).
    One launch of `wc_step_pair_hist` on the current stream, no host read: it may run inside a graph capture."""
    L.require_gpu()
    B, C, Hs, Ws = seg.shape
    if label.dim() != 3 or label.shape[0] != B:
        raise RuntimeError("step_pair_hist: label must be (B, H, W) with seg's batch size")
    if tuple(hist.shape) != (int(num_classes), int(num_classes)):
        raise RuntimeError("step_pair_hist: hist must be (num_classes, num_classes)")
    if flag is None:
        flag = _flag(seg.device)
    L.lib().wc_step_pair_hist(L.ptr(seg, F32, "seg"), L.ptr(label, torch.int64, "label"), L.ptr(hist, torch.int64, "hist"),
                              L.ptr(flag, torch.int32, "flag"), B, C, Hs, Ws, label.shape[1], label.shape[2], int(num_classes),
                              L.stream())
    return hist


class Validator:
    """model: WeCLIP (VOC, COCO or the seg-only supervised variant) on the GPU.  rank / world: this process's share of the
    images under data parallelism (`msc_flip.shard`: images rank, rank + world, ...; replicas only, ONE all-reduce of the
    histograms at the end).  A model whose class says `val_logits_only = True` (model_attn_aff_voc_seg.py) is called as
    `model(inputs, mode="val")` and returns the logits alone: no CAM leg, `cam_score` None."""

    def __init__(self, model, num_classes, rank=0, world=1):
        L.require_gpu()
        self.model, self.nc, self.rank, self.world = model, int(num_classes), int(rank), int(world)
        self.device = next(model.parameters()).device
        self.reset()

    def reset(self):
        self.seg_hist = torch.zeros(self.nc, self.nc, device=self.device, dtype=torch.int64)
        self.cam_hist = torch.zeros(self.nc, self.nc, device=self.device, dtype=torch.int64)
        # the CAM leg: known from the model where it says so (a rank whose share is empty must agree with the others)
        self.has_cam = bool(getattr(self.model, "val_runs_cam", False))
        # the seg-only model: `model(inputs, mode="val")` -> the logits alone (a class attribute, so every rank agrees)
        self.logits_only = bool(getattr(self.model, "val_logits_only", False))
        self.images = 0
        self.seg_hist_host = self.cam_hist_host = None    # the summed histograms on the host, once finish() has read them

    @torch.no_grad()
    def add(self, inputs, labels, class_ids):
        """One image: inputs (1,3,H,W) normalised pixels, labels (1,Hl,Wl) integer class map (255 = ignore), class_ids the
        image's class ids (what the CAM leg of the VOC model builds its channels from; unused by a logits-only model)."""
        if self.logits_only:
            seg, cam = self.model(inputs, mode="val"), None
        else:
            out = self.model(inputs, [""], mode="val", labels=[list(class_ids)])
            seg, cam = out[0], out[1]
        gt = labels[0].to(self.device).long().contiguous()
        if cam is not None:
            cam = (cam[0] if isinstance(cam, (list, tuple)) else cam.reshape(cam.shape[-2:])).long().contiguous()
            self.has_cam = True
        val_pair_hist(seg[0].float().contiguous(), cam, gt, self.nc, self.seg_hist, self.cam_hist)
        self.images += 1

    def run(self, loader):
        """loader: a DeviceLoader over an aug=False Seg dataset (batch_size 1).  -> (seg_score, cam_score) dicts of
        `evaluate.scores_from_hist`; cam_score is None when the model returns no CAM map in 'val' (COCO).  Leaves the model
        in training mode, as the reference's validate does."""
        from .datasets import labels_from_onehot
        self.reset()
        self.model.eval()
        try:
            for _, inputs, labels, _ in msc_flip.shard_batches(loader, self.rank, self.world):
                self.add(inputs, labels, labels_from_onehot(loader.last_cls_labels)[0])
            return self.finish()
        finally:
            self.model.train()

    def finish(self):
        """All-reduce and read the two histograms, check the flag -> (seg_score, cam_score)."""
        msc_flip.reduce_hist(self.seg_hist)
        msc_flip.reduce_hist(self.cam_hist)               # (zeros without a CAM leg: every rank takes part either way)
        if not evaluate.check_predictions_in_range(self.device):
            raise RuntimeError("Validator: a predicted or CAM label lies outside [0, num_classes) -- the histograms skip such "
                               "pixels; check num_classes against the model and the CAM label maps")
        self.seg_hist_host = self.seg_hist.cpu().numpy()
        self.cam_hist_host = self.cam_hist.cpu().numpy() if self.has_cam else None
        seg_score = evaluate.scores_from_hist(self.seg_hist_host)
        cam_score = evaluate.scores_from_hist(self.cam_hist_host) if self.has_cam else None
        return seg_score, cam_score
