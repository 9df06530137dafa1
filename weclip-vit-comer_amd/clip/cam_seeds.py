"""CAM seeds to pseudo-labels on the device (csrc/camseed.hip): what everyone does with the dumpers' `.npy` maps,
done on the bucket buffer before it leaves the GPU.

    sweep_bins / confusion_from_bins / sweep_confusion   the background-threshold sweep: `_fast_hist(gt, cam_to_label(...))`
                                                         (reference utils/camutils.py:8-16, utils/evaluate.py:9-16) for T
                                                         thresholds in one pass over the maps
    seed_labels                                          the two slot maps of utils/camutils.py:55-79 at the image's own size
    merge_labels                                         :77-79 + `pseudo_scores` (utils/evaluate.py:38-60) + the colour image
    SeedEvaluator                                        the three steps over CamGenerator(..., to_numpy=False) payloads, with
                                                         the CRF of utils.dcrf between the slot maps and the merge, PNGs
                                                         through msc_flip_eval.WriterPool

The maps are (P, HW) fp16, the (image, class) pairs of an image consecutive; `keys` is one list of 0-based foreground class ids
per image, in the dumpers' first-seen order.  Every result is an integer count or label: exact.  Argument errors are raised on the
host as RuntimeError before anything is launched; importing needs no GPU."""
import ctypes
import json
import os

import numpy as np
import torch

from .. import _lib as L
from ..msc_flip_eval import WriterPool, to_json

F16, I32, I64, U8 = torch.float16, torch.int32, torch.int64, torch.uint8
MAX_THRESHOLDS = 64
MAX_CLASSES = 256
# The reference's YAMLs carry no cam.low_thre / cam.high_thre: these are the values of the AFA lineage's configs
DEFAULT_LOW_THRE, DEFAULT_HIGH_THRE = 0.35, 0.55
REFINE = ("none", "crf")


# ---- arguments -------------------------------------------------------------------------------------------------------
def parse_thresholds(text):
    """`0.05:0.80:0.05` (first:last:step, both ends included) or `0.3,0.4,0.5` -> list of floats."""
    text = str(text).strip()
    if ":" in text:
        parts = text.split(":")
        if len(parts) != 3:
            raise RuntimeError(f"thresholds: expected first:last:step, got {text!r}")
        a, b, s = (float(p) for p in parts)
        if not s > 0 or b < a:
            raise RuntimeError(f"thresholds: need step > 0 and last >= first, got {text!r}")
        n = int(np.floor((b - a) / s + 1e-9)) + 1
        vals = [round(a + i * s, 10) for i in range(n)]
    else:
        vals = [float(p) for p in text.split(",") if p.strip()]
    return check_thresholds(vals)


def check_thresholds(thresholds):
    vals = [float(t) for t in thresholds]
    if not 1 <= len(vals) <= MAX_THRESHOLDS:
        raise RuntimeError(f"thresholds: {len(vals)} values (1 <= T <= {MAX_THRESHOLDS})")
    # the kernel compares in f32: the order must hold there
    f = np.asarray(vals, np.float32)
    if not np.isfinite(f).all() or (len(f) > 1 and not (np.diff(f) > 0).all()):
        raise RuntimeError("thresholds must be finite and strictly ascending")
    return vals


def _check_classes(num_classes):
    nc = int(num_classes)
    if not 2 <= nc <= MAX_CLASSES:
        raise RuntimeError(f"num_classes = {nc} (2 <= num_classes <= {MAX_CLASSES})")
    return nc


def sweep_path(nc, Kmax, T):
    """"lds" when wc_cam_seed_sweep stages its counts in per-workgroup LDS cells for these sizes, "global" otherwise."""
    use = ctypes.c_int(0)
    L.lib().wc_cam_seed_sweep_path(int(nc), int(Kmax), int(T), ctypes.byref(use))
    return "lds" if use.value else "global"


class PairTables:
    """The device tables of a bucket from its per-image class-id lists, made with ONE pinned asynchronous copy: first (B+1)
    int32, keys (P) int32, slot_class (B, S) int32 (entry 0 = 0, entry s = 1 + the s-th smallest id; S = Kmax + 1)."""

    def __init__(self, keys, num_classes, device):
        nc = _check_classes(num_classes)
        ids = [[int(k) for k in (ks.tolist() if hasattr(ks, "tolist") else ks)] for ks in keys]
        if not ids:
            raise RuntimeError("keys: no image")
        for b, ks in enumerate(ids):
            if not ks:
                raise RuntimeError(f"keys: image {b} has no class id")
            if len(set(ks)) != len(ks):
                raise RuntimeError(f"keys: image {b} names a class twice: {ks}")
            if min(ks) < 0 or max(ks) >= nc - 1:
                raise RuntimeError(f"keys: image {b} has a class id outside [0, {nc - 1}): {ks}")
        self.ids, self.nc = ids, nc
        self.B, self.P = len(ids), sum(len(k) for k in ids)
        self.Kmax = max(len(k) for k in ids)
        self.S = self.Kmax + 1
        first = np.concatenate([[0], np.cumsum([len(k) for k in ids])])
        table = np.zeros((self.B, self.S), np.int64)
        for b, ks in enumerate(ids):
            table[b, 1:len(ks) + 1] = 1 + np.sort(ks)
        host = torch.from_numpy(np.concatenate([first, np.concatenate(ids), table.reshape(-1)]).astype(np.int32))
        dev = torch.device(device)
        if dev.type == "cuda":
            host = host.pin_memory()
        d = host.to(dev, non_blocking=True)
        self.first, self.keys = d[:self.B + 1], d[self.B + 1:self.B + 1 + self.P]
        self.slot_class = d[self.B + 1 + self.P:].view(self.B, self.S)

    @classmethod
    def from_device(cls, num_classes, first=None, keys=None, slot_class=None, Kmax=None):
        """Tables that are device tensors already (torch.ops.weclip.cam_seed_*): sizes only, no host check of the ids."""
        t = cls.__new__(cls)
        t.nc, t.ids = _check_classes(num_classes), None
        if first is not None:
            t.first, t.keys = first.to(I32).contiguous(), keys.to(I32).contiguous()
            t.B, t.P = t.first.numel() - 1, t.keys.numel()
            t.Kmax = int(Kmax) if Kmax is not None else min(t.P, 255)
        if slot_class is not None:
            t.slot_class = slot_class.to(I32).contiguous()
            t.B, t.S = t.slot_class.shape
        return t


_flags = {}


def _flag(device):
    f = _flags.get(device)
    if f is None:
        f = _flags[device] = torch.zeros(1, device=device, dtype=I32)
    return f


def check_tables_in_range(device):
    """True unless a kernel of this module on `device` met a pair table or a slot outside its range since start-up (one
    device -> host read: call it once, after the loop)."""
    f = _flags.get(torch.device(device))
    return f is None or int(f.item()) == 0


def _maps(cams, tables):
    if not isinstance(cams, torch.Tensor) or not cams.is_cuda or cams.dtype != F16:
        raise RuntimeError("cams: expected a CUDA float16 tensor (P, HW) or (P, H, W)")
    if cams.dim() not in (2, 3) or cams.shape[0] != tables.P:
        raise RuntimeError(f"cams: {tuple(cams.shape)} for {tables.P} (image, class) pairs")
    c = cams.reshape(tables.P, -1).contiguous()
    if c.data_ptr() % 16:
        c = c.clone()
    return c


def _gt(gt, B, HW, device):
    g = torch.as_tensor(gt)
    if g.dtype != U8 or g.shape[0] != B or g.numel() != B * HW:
        raise RuntimeError(f"gt: expected uint8 (B, HW) = ({B}, {HW}), got {g.dtype} {tuple(g.shape)}")
    g = g.to(device, non_blocking=True).reshape(B, HW).contiguous()
    return g.clone() if g.data_ptr() % 4 else g


# ---- the three kernels -----------------------------------------------------------------------------------------------
def sweep_bins(cams, keys, gt, thresholds, num_classes, bins=None, tables=None, force_global=False):
    """bins (nc, nc, T+1) int64 += counts of (gt, c, j*) over the pixels with gt < nc (wc_cam_seed_sweep), j* = the number of
    thresholds below the pixel's maximum.  `bins` accumulates across calls; a new zeroed tensor without it."""
    L.require_gpu()
    thr = check_thresholds(thresholds)
    tables = tables or PairTables(keys, num_classes, cams.device)
    nc, T = tables.nc, len(thr)
    c = _maps(cams, tables)
    HW = c.shape[1]
    g = _gt(gt, tables.B, HW, c.device)
    if bins is None:
        bins = torch.zeros(nc, nc, T + 1, device=c.device, dtype=I64)
    elif tuple(bins.shape) != (nc, nc, T + 1):
        raise RuntimeError(f"bins: expected {(nc, nc, T + 1)}, got {tuple(bins.shape)}")
    L.lib().wc_cam_seed_sweep(L.ptr(c, F16, "cams"), L.ptr(tables.first, I32), L.ptr(tables.keys, I32), L.ptr(g, U8, "gt"),
                              (ctypes.c_float * T)(*thr), L.ptr(bins, I64, "bins"), L.ptr(_flag(c.device)), tables.B, tables.P, HW,
                              nc, T, tables.Kmax, 1 if force_global else 0, L.stream())
    return bins


def confusion_from_bins(bins):
    """conf (T, nc, nc) from bins (nc, nc, T+1), on whichever device bins is (tensor or numpy): a pixel counted at j* is class c
    for the thresholds j < j* and background for the others, so
        conf[j][g][c] = sum_{s > j} bins[g][c][s]  (c >= 1),   conf[j][g][0] = sum_{c >= 1} sum_{s <= j} bins[g][c][s].
    Two cumulative sums of stock tensor ops, once per run: not a kernel."""
    b = torch.as_tensor(bins)
    T = b.shape[2] - 1
    above = b.flip(2).cumsum(2).flip(2)[:, :, 1:]                   # [g][c][j] = sum_{s >= j + 1}
    below = b.cumsum(2)[:, :, :T]                                    # [g][c][j] = sum_{s <= j}
    conf = above.permute(2, 0, 1).contiguous()
    conf[:, :, 0] = below[:, 1:, :].sum(1).permute(1, 0)
    return conf.numpy() if isinstance(bins, np.ndarray) else conf


def sweep_confusion(cams, keys, gt, thresholds, num_classes, bins=None, force_global=False):
    """conf (T, nc, nc) int64: conf[j] = `_fast_hist(gt, cam_to_label(cam, bkg_score=t_j), nc)` summed over the images (and over
    the earlier calls that filled `bins`)."""
    return confusion_from_bins(sweep_bins(cams, keys, gt, thresholds, num_classes, bins=bins, force_global=force_global))


def seed_labels(cams, keys, low_thre, high_thre, num_classes=MAX_CLASSES, tables=None):
    """(lab_low, lab_high), each (B, HW) int64 -- (B, H, W) for 3-D cams: slot 1 + rank of the winning class among the image's
    ids where the maximum exceeds the threshold, else 0 (wc_cam_seed_labels); the dtype utils.dcrf.unary_from_labels reads."""
    L.require_gpu()
    low, high = float(low_thre), float(high_thre)
    if not (np.isfinite(low) and np.isfinite(high) and low <= high):
        raise RuntimeError(f"seed_labels: need finite low_thre <= high_thre, got {low}, {high}")
    tables = tables or PairTables(keys, num_classes, cams.device)
    c = _maps(cams, tables)
    HW = c.shape[1]
    shape = (tables.B,) + tuple(cams.shape[1:]) if cams.dim() == 3 else (tables.B, HW)
    lab_low, lab_high = (torch.empty(shape, device=c.device, dtype=I64) for _ in range(2))
    L.lib().wc_cam_seed_labels(L.ptr(c, F16, "cams"), L.ptr(tables.first, I32), L.ptr(tables.keys, I32), L.ptr(lab_low), L.ptr(lab_high),
                               L.ptr(_flag(c.device)), tables.B, tables.P, HW, low, high, L.stream())
    return lab_low, lab_high


def merge_labels(lab_low, lab_high, keys, num_classes, gt=None, label=None, cmap=None, hist=None, cover=None, want_cmap=False,
                 tables=None):
    """The merge of utils/camutils.py:77-79 for the B images of a bucket in one launch (wc_cam_seed_merge).  lab_low / lab_high
    (B, ...) int64 slot maps, refined or not.  -> (label uint8 like lab_high, cmap (..., 3) uint8 or None, hist (nc, nc) int64 or
    None, cover int64[2] or None); label / cmap / hist / cover may be passed in (hist and cover accumulate)."""
    L.require_gpu()
    nc = _check_classes(num_classes)
    tables = tables or PairTables(keys, nc, lab_high.device)
    if lab_low.shape != lab_high.shape or lab_high.shape[0] != tables.B:
        raise RuntimeError(f"merge_labels: slot maps {tuple(lab_low.shape)} / {tuple(lab_high.shape)} for {tables.B} images")
    lo, hi = lab_low.contiguous(), lab_high.contiguous()
    dev, B = hi.device, tables.B
    HW = hi.numel() // B
    if label is None:
        label = torch.empty(hi.shape, device=dev, dtype=U8)
    if cmap is None and want_cmap:
        cmap = torch.empty(tuple(hi.shape) + (3,), device=dev, dtype=U8)
    if label.numel() != B * HW or (cmap is not None and cmap.numel() != 3 * B * HW):
        raise RuntimeError("merge_labels: label / cmap do not match the slot maps")
    g = None
    if gt is not None:
        g = _gt(gt, B, HW, dev)
        hist = torch.zeros(nc, nc, device=dev, dtype=I64) if hist is None else hist
        cover = torch.zeros(2, device=dev, dtype=I64) if cover is None else cover
        if tuple(hist.shape) != (nc, nc) or cover.numel() != 2:
            raise RuntimeError("merge_labels: hist must be (nc, nc) and cover (2,)")
    L.lib().wc_cam_seed_merge(L.ptr(lo, I64, "lab_low"), L.ptr(hi, I64, "lab_high"), L.ptr(tables.slot_class, I32), L.ptr(g),
                              L.ptr(label, U8, "label"), L.ptr(cmap, U8, "cmap"), L.ptr(hist, I64, "hist") if g is not None else None,
                              L.ptr(cover, I64, "cover") if g is not None else None, L.ptr(_flag(dev)), B, HW, tables.S, nc,
                              L.stream())
    return label, cmap, (hist if g is not None else None), (cover if g is not None else None)


# ---- scores ----------------------------------------------------------------------------------------------------------
def summarise(num_classes, thresholds, bins, mask_hist, cover, images, low_thre=None, high_thre=None, refine=None,
              crf_bilateral=None):
    """The result dict of SeedEvaluator.finish() from host arrays (also what the dumpers' parent builds from the sum of its
    workers' parts).  bins / mask_hist / cover may be None for a leg that did not run."""
    from ..utils.evaluate import scores_from_hist
    out = {"num_classes": int(num_classes), "images": int(images)}
    if bins is not None:
        bins = np.asarray(bins, np.int64)
        conf = confusion_from_bins(bins)
        rows = []
        for t, h in zip(thresholds, conf):
            s = scores_from_hist(h)
            rows.append({"threshold": float(t), "pAcc": s["pAcc"], "mAcc": s["mAcc"], "miou": s["miou"]})
        finite = [r for r in rows if np.isfinite(r["miou"])]
        out["thresholds"] = [float(t) for t in thresholds]
        out["sweep"] = rows
        out["best"] = dict(max(finite, key=lambda r: r["miou"])) if finite else None
        out["bins"] = bins.tolist()
    if mask_hist is not None:
        mask_hist, cover = np.asarray(mask_hist, np.int64), np.asarray(cover, np.int64)
        s = scores_from_hist(mask_hist)
        out["masks"] = {"low_thre": low_thre, "high_thre": high_thre, "refine": refine, "crf_bilateral": crf_bilateral,
                        "pAcc": s["pAcc"], "mAcc": s["mAcc"], "miou": s["miou"], "iou": s["iou"], "labelled": int(cover[0]),
                        "valid": int(cover[1]), "coverage": float(cover[0]) / float(cover[1]) if cover[1] else float("nan"),
                        "hist": mask_hist.tolist()}
    return out


def write_scores(path, result):
    with open(path, "w") as fh:
        json.dump(to_json(result), fh, allow_nan=False)


class BucketWriter(WriterPool):
    """msc_flip_eval.WriterPool with a whole bucket per slot: acquire(B * H, W) gives views that are the merge kernel's (B, HW)
    outputs, commit(slot, names) makes the ONE device -> host copy of the bucket, and a writer thread cuts it into the B pairs
    prediction/NAME.png (mode L), prediction_cmap/NAME.png (RGB)."""

    def _write(self, slot, names):
        from PIL import Image
        BH, W = slot.layout[:2]
        B = len(names)
        H = BH // B
        slot.copied.synchronize()
        pred = self.host(slot, "pred").reshape(B, H, W)
        cmap = self.host(slot, "cmap").reshape(B, H, W, 3)
        for b, name in enumerate(names):
            Image.fromarray(pred[b], mode="L").save(os.path.join(self.dirs["prediction"], name + ".png"))
            Image.fromarray(cmap[b], mode="RGB").save(os.path.join(self.dirs["prediction_cmap"], name + ".png"))


class SeedEvaluator:
    """The sweep, the masks and their scores over CamGenerator(..., to_numpy=False) payloads.

    thresholds: the background thresholds of the sweep (None: no sweep).  masks: build the seed label maps with (low_thre,
    high_thre) -- refine="crf" passes the two slot maps of every image through utils.dcrf.crf_inference_label(img, lab,
    n_labels=K+1) (t=10, gt_prob=0.7) before the merge.  out_dir: prediction/NAME.png (mode L) and prediction_cmap/NAME.png.
    Nothing is read back from the device until finish().  masks=False (or no thresholds) leaves that leg out."""

    def __init__(self, num_classes, thresholds=None, low_thre=DEFAULT_LOW_THRE, high_thre=DEFAULT_HIGH_THRE, refine="none",
                 crf_bilateral="exact", out_dir=None, masks=True, writers=4, keep_labels=False):
        from ..utils.dcrf import BILATERAL
        self.nc = _check_classes(num_classes)
        self.thresholds = check_thresholds(thresholds) if thresholds is not None and len(thresholds) else None
        self.low, self.high = float(low_thre), float(high_thre)
        if not (np.isfinite(self.low) and np.isfinite(self.high) and self.low <= self.high):
            raise RuntimeError(f"SeedEvaluator: need finite low_thre <= high_thre, got {self.low}, {self.high}")
        if refine not in REFINE:
            raise RuntimeError(f"SeedEvaluator: refine must be one of {REFINE}, got {refine!r}")
        if crf_bilateral not in BILATERAL:
            raise RuntimeError(f"SeedEvaluator: crf_bilateral must be one of {BILATERAL}, got {crf_bilateral!r}")
        self.refine, self.bilateral = refine, crf_bilateral
        self.masks = bool(masks) or out_dir is not None
        self.out_dir, self.writers = out_dir, writers
        self.pool = None
        self.bins = self.hist = self.cover = None
        self.device = None
        self.images = 0
        # keep_labels: the label maps of the last add() stay in `last_labels`, one (H0, W0) uint8 device tensor per payload that is
        # not None, in payload order (a copy when they were written into a writer slot)
        self.keep_labels, self.last_labels = bool(keep_labels), None

    @staticmethod
    def _runs(items):
        """Consecutive images of one size whose maps follow one another in memory: one (P, HW) view each, no copy."""
        runs = []
        for it in items:
            cam = it[0]
            last = runs[-1] if runs else None
            if (last is not None and last[-1][0].shape[1:] == cam.shape[1:] and cam.is_contiguous() and last[-1][0].is_contiguous()
                    and last[-1][0].data_ptr() + last[-1][0].numel() * 2 == cam.data_ptr()
                    and last[-1][0].untyped_storage().data_ptr() == cam.untyped_storage().data_ptr()):
                last.append(it)
            else:
                runs.append([it])
        return runs

    @torch.no_grad()
    def add(self, payloads, images_u8=None, gts_u8=None, names=None):
        """payloads: CamGenerator's list ({"keys", "attn_highres" (K, H0, W0) fp16 on the device} or None for a skipped image);
        images_u8: the (H0, W0, 3) uint8 images (the CRF's; needed with refine="crf"); gts_u8: (H0, W0) uint8 label maps, host or
        device, or None (no scores); names: file stems for the PNGs."""
        L.require_gpu()
        n = len(payloads)
        items = []
        for i, p in enumerate(payloads):
            if p is None:
                continue
            cam = p["attn_highres"]
            if not isinstance(cam, torch.Tensor) or not cam.is_cuda:
                raise RuntimeError("SeedEvaluator.add: payloads must hold device tensors (CamGenerator(..., to_numpy=False))")
            gt = None if gts_u8 is None else gts_u8[i]
            if gt is not None and tuple(gt.shape) != tuple(cam.shape[1:]):
                raise RuntimeError(f"SeedEvaluator.add: ground truth {tuple(gt.shape)} for maps of {tuple(cam.shape[1:])}")
            items.append((cam, p["keys"], None if images_u8 is None else images_u8[i], gt, None if names is None else names[i]))
        if gts_u8 is not None and len(gts_u8) != n:
            raise RuntimeError("SeedEvaluator.add: one ground truth per payload")
        # in memory order: the images of one CamGenerator bucket (equal sizes, one buffer) then stand next to each other, whatever
        # their places in the chunk
        order = sorted(range(len(items)), key=lambda i: (items[i][0].untyped_storage().data_ptr(), items[i][0].data_ptr()))
        self.last_labels = {}
        for run in self._runs([items[i] + (i,) for i in order]):
            self._run(run)
        self.last_labels = [self.last_labels[i] for i in sorted(self.last_labels)]

    def _run(self, run):
        from ..utils import dcrf
        first = run[0][0]
        dev, (H, W) = first.device, first.shape[1:]
        HW, B = H * W, len(run)
        self.device = dev
        P = sum(it[0].shape[0] for it in run)
        cams = first.as_strided((P, HW), (HW, 1)) if B > 1 else first.reshape(P, HW)
        tables = PairTables([it[1] for it in run], self.nc, dev)
        gt = None
        if run[0][3] is not None:
            gs = [it[3] for it in run]
            if isinstance(gs[0], torch.Tensor) and gs[0].is_cuda:
                gt = torch.stack([g.reshape(HW) for g in gs])
            else:                        # one pinned copy for the run
                host = torch.from_numpy(np.stack([np.asarray(g, np.uint8).reshape(HW) for g in gs])).pin_memory()
                gt = host.to(dev, non_blocking=True)
        if self.thresholds is not None and gt is not None:
            self.bins = sweep_bins(cams, None, gt, self.thresholds, self.nc, bins=self.bins, tables=tables)
        if self.masks:
            low, high = seed_labels(cams, None, self.low, self.high, tables=tables)
            if self.refine == "crf":
                for b, it in enumerate(run):
                    if it[2] is None:
                        raise RuntimeError('SeedEvaluator.add: refine="crf" needs the images')
                    img = it[2] if it[2].is_cuda else it[2].to(dev, non_blocking=True)
                    K = len(tables.ids[b])
                    for lab in (low, high):
                        lab[b] = dcrf.crf_inference_label(img, lab[b].view(H, W), n_labels=K + 1, bilateral=self.bilateral).view(HW)
            slot = label = cmap = None
            if self.out_dir is not None:
                if self.pool is None:
                    self.pool = BucketWriter(self.out_dir, writers=self.writers)
                slot = self.pool.acquire(B * H, W)
                label, cmap = slot.views["pred"], slot.views["cmap"]
            label, _, hist, cover = merge_labels(low, high, None, self.nc, gt=gt, label=label, cmap=cmap, hist=self.hist,
                                                 cover=self.cover, tables=tables)
            if gt is not None:
                self.hist, self.cover = hist, cover
            if self.keep_labels:
                kept = (label.clone() if slot is not None else label).view(B, H, W)      # a slot is reused by a later bucket
                self.last_labels.update({it[5]: kept[b] for b, it in enumerate(run)})
            if slot is not None:
                self.pool.commit(slot, [str(it[4]) for it in run])
        self.images += B

    def arrays(self):
        """The raw counts on the host: {"bins", "hist", "cover", "images"} (None for a leg that did not run): what a worker of
        the dumpers stores and their parent sums."""
        host = lambda t: None if t is None else t.cpu().numpy()       # noqa: E731
        return {"bins": host(self.bins), "hist": host(self.hist), "cover": host(self.cover), "images": self.images}

    def finish(self):
        """Drain the writers, check the device flag, read the counts (the only host read of the scores) -> summarise()'s dict:
        "sweep" [{threshold, pAcc, mAcc, miou}], "best", "masks" {pAcc, mAcc, miou, iou, coverage, ...}, "images"."""
        if self.pool is not None:
            self.pool.finish()
            self.pool = None
        if self.device is not None and not check_tables_in_range(self.device):
            raise RuntimeError("SeedEvaluator: a pair table, class id or slot label left its range; such pixels were not counted")
        a = self.arrays()
        return summarise(self.nc, self.thresholds, a["bins"], a["hist"], a["cover"], a["images"], self.low, self.high, self.refine,
                         self.bilateral)
