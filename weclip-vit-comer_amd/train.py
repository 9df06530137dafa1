"""The training driver: `train()` and `validate()` of the reference's scripts (scripts/dist_clip_voc.py:71-102, 137-296,
scripts/dist_clip_coco.py) around this package's graph-replayed step.

    python -m weclip_vit_comer_amd.train --config configs/voc_attn_reg.yaml --work_dir work_dir_voc --crop_size 320 \
        [--dataset voc|coco|seg] [--reference_root <reference checkout>] [--no-graph] [--max_iters N] [--resume <model .pth>]
        [--reg_loss [--reg_coef 0.01] [--reg_scale 0.5] [--reg_start <train.cam_iters>] [--reg_bilateral exact|lattice]] [--panel_iters N]
        [--optimizer AdamW|SGD]

`optimizer.type` of the YAML (AdamW when the key is missing; --optimizer overrides it) chooses between `PolyWarmupAdamW` and
`PolyWarmupSGD` (utils/optimizer.py), each one HIP launch per parameter group.  The choice is the first line of the log and
is stored in train_state_iter_N.pth; --resume refuses a state written by the other one.

The configuration is the reference's YAML file, unchanged.  Per step nothing leaves the GPU: the three loss scalars are added
into a device accumulator, and the reference's `pseudo_seg_mAcc` (:274-277) is counted by `wc_label_match_count`
(csrc/trainlog.hip) inside the captured step; every `log_iters` ONE read fetches both.  Validation is `validate.Validator`.
--reg_loss adds the dense energy (regularised) loss as a fourth scalar of the same accumulator (TrainStep(reg=...)).
Under `python -m torch.distributed.run` every rank trains on its share of each epoch (DeviceLoader rank / world), gradients
are averaged through `GradBucket`, every rank validates its share of the images, and rank 0 alone logs and saves.

--dataset seg trains the fully supervised variant (WeCLIP_model/model_attn_aff_voc_seg.py) on VOC's ground-truth masks: the same
YAML, `VOC12SegDataset(aug=True)` batches whose labels never visit the host, `LoggedSupervisedTrainStep`, and a log line of
this package's own (the reference ships no training script for the variant): the window's mean cross-entropy and the pAcc /
mAcc / mIoU of the window's confusion matrix, which `wc_step_pair_hist` (csrc/trainlog.hip) counts inside the captured step.

--panel_iters N (default 0: off) makes rank 0 render the reference's tensorboard image panels (utils/imutils.py; here
utils/panels.py, csrc/panels.hip) after iterations N, 2N, ...: `images`, `pseudo_label` (`gt_label` with --dataset seg),
`prediction`, `seg_conf` and, for the weakly supervised variants, `attn_pred_0..3`, written as <work_dir>/panels/iter_<n>_<name>.png
by writer threads (`PanelWriter`) and handed to tensorboard where it imports.  The step then snapshots its logits, label map and
four attn_pred rows inside the captured graph (`wc_panel_snapshot`); the render runs outside it, on panel iterations only, with
no forward and no host read.

Two optional keys extend the configuration, both under `clip_init`: `text_features` (a torch file holding {"bg", "fg"}: the
zero-shot text rows, for a machine without the reference checkout that `--reference_root` names) and `comer` (bool).
"""
import argparse
import datetime
import json
import logging
import os
import random
import re

import numpy as np
import torch
import torch.distributed as dist

from .entry import Config, _wrap, build_model, init_distributed, load_config, strict_json  # noqa: F401  (re-exported)
from .train_step import OPTIMIZER_TYPES, SupervisedTrainStep, TrainStep, make_optimizer
from .utils.writer_ring import WriterRing, _cuda_alloc, _cuda_event

LOG = logging.getLogger("weclip.train")
LOG_FORMAT = "Iter: %d; Elasped: %s; ETA: %s; LR: %.3e;, pseudo_seg_loss: %.4f, attn_loss: %.4f, pseudo_seg_mAcc: %.4f"   # :280
SEG_LOG_FORMAT = "Iter: %d; Elasped: %s; ETA: %s; LR: %.3e;, seg_loss: %.4f, seg_pAcc: %.4f, seg_mAcc: %.4f, seg_mIoU: %.4f"   # --dataset seg
REG_FORMAT = ", reg_loss: %.4e"                         # appended with --reg_loss only


class _SaveAfter(dict):
    """First iteration past which checkpoints are written, per --dataset.  "seg" runs on VOC's YAML and has no entry of its
    own: it reads VOC's, so the two cannot drift apart (and the table still lists exactly the reference's two scripts)."""

    def __missing__(self, kind):
        if kind == "seg":
            return self["voc"]
        raise KeyError(kind)


SAVE_AFTER = _SaveAfter(voc=26000, coco=40000)          # dist_clip_voc.py:288, dist_clip_coco.py:287
MODEL_FILE, STATE_FILE = "WeCLIP_model_iter_%d.pth", "train_state_iter_%d.pth"


# ---------------------------------------------------------------------------------------------- the command line
def build_parser():
    p = argparse.ArgumentParser(prog="python -m weclip_vit_comer_amd.train", description=__doc__.split("\n\n")[0])
    p.add_argument("--config", type=str, required=True, help="the reference's YAML (configs/voc_attn_reg.yaml, coco_attn_reg.yaml)")
    p.add_argument("--seg_detach", action="store_true", help="accepted and ignored, as in the reference")
    p.add_argument("--work_dir", default=None, type=str)
    p.add_argument("--radius", default=8, type=int, help="affinity radius (unused with --dataset seg)")
    p.add_argument("--crop_size", default=320, type=int)
    p.add_argument("--dataset", choices=("voc", "coco", "seg"), default="voc",
                   help="seg: the fully supervised variant on VOC's ground-truth masks (the word's meaning in msc_flip_eval)")
    p.add_argument("--reference_root", type=str, default=None, help="reference checkout holding clip/clip_text.py and the BPE merges")
    p.add_argument("--graph", action=argparse.BooleanOptionalAction, default=True, help="HIP-graph replay of the step")
    p.add_argument("--threads", type=int, default=8, help="decode threads of the loaders")
    p.add_argument("--prefetch", type=int, default=2)
    p.add_argument("--max_iters", type=int, default=None, help="overrides train.max_iters")
    p.add_argument("--save_after", type=int, default=None,
                   help="checkpoints are written past this iteration (voc and seg 26000, coco 40000)")
    p.add_argument("--resume", type=str, default=None, help="a WeCLIP_model_iter_N.pth; its train_state_iter_N.pth is loaded with it")
    p.add_argument("--optimizer", type=str, default=None, choices=OPTIMIZER_TYPES,
                   help="overrides optimizer.type of the YAML (a YAML without the key means AdamW)")
    p.add_argument("--reg_loss", action="store_true",
                   help="add the dense energy (regularised) loss to the step; its all-pairs filter costs about four plain steps at "
                        "batch 16 / crop 512 (DESIGN.md section 15.2; --reg_bilateral lattice: half a step, section 15.3)")
    p.add_argument("--reg_coef", type=float, default=0.01, help="weight of the energy term in the step's loss")
    p.add_argument("--reg_scale", type=float, default=0.5, choices=(1.0, 0.5, 0.25), help="scale_factor of the DenseEnergyLoss")
    p.add_argument("--reg_start", type=int, default=None, help="the term starts after this iteration (default: train.cam_iters)")
    p.add_argument("--reg_bilateral", type=str, default="exact", choices=("exact", "lattice"),
                   help="the term's bilateral filter: the exact all-pairs sum, or the permutohedral lattice (much cheaper; about half "
                        "the exact value, so --reg_coef does not carry over; DESIGN.md section 15.3)")
    p.add_argument("--panel_iters", type=int, default=0,
                   help="rank 0 writes the image panels (<work_dir>/panels/iter_<n>_<name>.png) every this many iterations; 0: off")
    return p


def prepare_work_dir(cfg, timestamp=None, create=True):
    """The tree of :308-318: <dir>/<ckpt_dir>/<timestamp>, <dir>/<pred_dir>, <dir>/<tb_logger_dir>/<timestamp>; returns the
    path of <dir>/<timestamp>.log.  create=False (ranks other than 0) only resolves the names."""
    timestamp = timestamp or "{0:%Y-%m-%d-%H-%M}".format(datetime.datetime.now())
    wd = cfg.work_dir
    wd.ckpt_dir = os.path.join(wd.dir, wd.ckpt_dir, timestamp)
    wd.pred_dir = os.path.join(wd.dir, wd.pred_dir)
    wd.tb_logger_dir = os.path.join(wd.dir, wd.tb_logger_dir, timestamp)
    if create:
        for d in (wd.ckpt_dir, wd.pred_dir, wd.tb_logger_dir):
            os.makedirs(d, exist_ok=True)
    return os.path.join(wd.dir, timestamp + ".log")


def checkpoint_paths(ckpt_dir, n_iter):
    """(model file in the reference's format, the training state beside it)."""
    return os.path.join(ckpt_dir, MODEL_FILE % n_iter), os.path.join(ckpt_dir, STATE_FILE % n_iter)


def state_path_of(model_path):
    """WeCLIP_model_iter_N.pth -> its sibling train_state_iter_N.pth."""
    d, name = os.path.split(model_path)
    m = re.match(r"^WeCLIP_model_iter_(\d+)\.pth$", name)
    if not m:
        raise ValueError(f"--resume wants a {MODEL_FILE % 0}-style file name, got {name}")
    return os.path.join(d, STATE_FILE % int(m.group(1)))


def format_log_line(n_iter, delta, eta, lr, seg_loss, attn_loss, seg_macc, reg_loss=None):
    line = LOG_FORMAT % (n_iter, delta, eta, lr, seg_loss, attn_loss, seg_macc)
    return line if reg_loss is None else line + REG_FORMAT % reg_loss


def log_record(n_iter, lr, host, steps):
    """The metrics.jsonl record of a window of `steps` steps from the one host read: host = the window sums (loss, seg_loss,
    attn_loss[, reg_loss with --reg_loss]) followed by the last step's (matches, pixels)."""
    rec = {"iter": n_iter, "lr": lr, "seg_loss": host[1] / steps, "attn_loss": host[2] / steps, "pseudo_seg_mAcc": host[-2] / host[-1]}
    if len(host) == 6:
        rec["reg_loss"] = host[3] / steps
    return rec


def format_seg_log_line(n_iter, delta, eta, lr, seg_loss, pacc, macc, miou, reg_loss=None):
    line = SEG_LOG_FORMAT % (n_iter, delta, eta, lr, seg_loss, pacc, macc, miou)
    return line if reg_loss is None else line + REG_FORMAT % reg_loss


def seg_log_record(n_iter, lr, host, steps, num_classes):
    """The metrics.jsonl record of a window of `steps` supervised steps from the one host read: host = the window sums (loss,
    seg_loss[, reg_loss with --reg_loss]) followed by the window's (nc, nc) confusion matrix, row-major.  pAcc / mAcc / miou
    are `evaluate.scores_from_hist` of that matrix: scores of the WHOLE window, not of its last step as `pseudo_seg_mAcc` is."""
    from .utils.evaluate import scores_from_hist
    cells = int(num_classes) ** 2
    sums = len(host) - cells
    if sums not in (2, 3):
        raise ValueError(f"seg_log_record: {len(host)} values are not 2 or 3 sums and a {num_classes} x {num_classes} matrix")
    score = scores_from_hist(np.asarray(host[sums:], dtype=np.float64).reshape(num_classes, num_classes))
    rec = {"iter": n_iter, "lr": lr, "seg_loss": host[1] / steps, "pAcc": float(score["pAcc"]), "mAcc": float(score["mAcc"]),
           "miou": float(score["miou"])}
    if sums == 3:
        rec["reg_loss"] = host[2] / steps
    return rec


def optimizer_type(cfg, args=None):
    """The optimizer the run uses, as make_optimizer spells it: --optimizer if given, else the YAML's optimizer.type (any
    letter case), else AdamW."""
    name = getattr(args, "optimizer", None) or cfg.optimizer.get("type") or "AdamW"
    for known in OPTIMIZER_TYPES:
        if str(name).lower() == known.lower():
            return known
    raise ValueError(f"optimizer.type must be one of {', '.join(OPTIMIZER_TYPES)}, got {name!r}")


def check_state_optimizer(state, configured, path="the training state"):
    """--resume: the optimizer a train_state file was written by (files from before the key existed: AdamW) must be the
    configured one; its tensors would not load into the other."""
    saved = state.get("optimizer_type", "AdamW")
    if saved != configured:
        raise RuntimeError(f"{path} was written by a run with optimizer {saved}, but this run is configured for {configured} "
                           "(optimizer.type of the YAML, or --optimizer): resume with the same optimizer")


def reg_settings(cfg, args):
    """The `reg` argument of the train step from the command line: None without --reg_loss."""
    if not getattr(args, "reg_loss", False):
        return None
    start = getattr(args, "reg_start", None)
    reg = {"coef": float(getattr(args, "reg_coef", 0.01)), "scale_factor": float(getattr(args, "reg_scale", 0.5)),
           "start_iter": int(cfg.train.cam_iters if start is None else start)}
    if getattr(args, "reg_bilateral", "exact") != "exact":      # without the flag the settings are what they were
        reg["bilateral"] = str(args.reg_bilateral)
    return reg


def append_metrics(path, record):
    with open(path, "a") as f:
        f.write(json.dumps(strict_json(record), allow_nan=False) + "\n")


def read_metrics(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def setup_seed(seed):
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True


def setup_logger(filename=None):
    """:44-56, on this module's logger: the file and the console."""
    fmt = logging.Formatter("%(asctime)s - %(filename)s - %(levelname)s: %(message)s")
    LOG.setLevel(logging.INFO)
    for h in [logging.StreamHandler()] + ([logging.FileHandler(filename, mode="w")] if filename else []):
        h.setFormatter(fmt)
        LOG.addHandler(h)


def cal_eta(time0, cur_iter, total_iter):
    """:59-68."""
    now = datetime.datetime.now().replace(microsecond=0)
    delta = now - time0
    eta = delta * ((total_iter - cur_iter) / float(cur_iter))
    fin = now + eta
    return str(delta), str(fin.replace(microsecond=0) - now)


# ---------------------------------------------------------------------------------------------- the step
class LoggedTrainStep(TrainStep):
    """TrainStep whose losses() also counts, on the device, the pixels where the up-sampled logits' arg-max equals the
    pseudo label (`counts` int64[2] = [matches, pixels], overwritten by every step).  The launch sits between the parent's
    loss kernels and the backward, so in graph mode it is part of the captured step; the returned losses are the parent's.
    panels (default None: nothing about the step changes): a `utils.panels.StepSnapshot`; one more launch beside the counting
    kernel then copies the logits, the pseudo labels (as uint8) and the four attn_pred rows of the attention panels into it."""

    def __init__(self, model, *args, panels=None, **kw):
        super().__init__(model, *args, **kw)
        self.counts = torch.zeros(2, device=next(model.parameters()).device, dtype=torch.int64)
        self.panels = panels

    def losses(self, seg, cam, attn_pred):
        out = super().losses(seg, cam, attn_pred)
        if seg.is_cuda:
            from .validate import label_match_count
            label_match_count(seg.detach().float().contiguous(), cam.long().contiguous(), self.counts)
            if self.panels is not None:
                self.panels.take(seg.detach().float().contiguous(), cam.long().contiguous(), attn_pred.detach().float().contiguous())
        return out


class LoggedSupervisedTrainStep(SupervisedTrainStep):
    """SupervisedTrainStep whose loss() also counts, on the device, the step's confusion matrix: `hist` (nc, nc) int64 gets
    hist[label, arg-max of the up-sampled logits] += 1 over the pixels with 0 <= label < nc (255 borders and crop padding are
    NOT in any denominator, unlike LoggedTrainStep's pixel count, which is right for pseudo labels only).  The step ADDS into
    `hist`; whoever reads it zeroes it.  `ce` (a static scalar) holds the step's cross-entropy, which under `reg` is not
    among the returned values.  Both launches sit between the parent's loss kernels and the backward, so in graph mode they
    are part of the captured step; they read `seg.detach()` and `label` only, and the returned loss is the parent's.
    panels (default None: nothing about the step changes): a `utils.panels.StepSnapshot` that one more launch fills with the
    logits and the ground-truth labels (as uint8)."""

    def __init__(self, model, *args, panels=None, **kw):
        super().__init__(model, *args, **kw)
        self.panels = panels
        dev = next(model.parameters()).device
        nc = int(model.num_classes)
        self.hist = torch.zeros(nc, nc, device=dev, dtype=torch.int64)
        self.ce = torch.zeros((), device=dev, dtype=torch.float32)
        self._flag = None
        if dev.type == "cuda":
            from .validate import _flag
            self._flag = _flag(dev)                  # created here, not inside a capture

    def loss(self, seg, label):
        out = super().loss(seg, label)
        if seg.is_cuda:
            from .validate import step_pair_hist
            self.ce.copy_(out.detach())
            step_pair_hist(seg.detach().float().contiguous(), label.long().contiguous(), self.hist.shape[0], self.hist, self._flag)
            if self.panels is not None:
                self.panels.take(seg.detach().float().contiguous(), label.long().contiguous())
        return out


# ---------------------------------------------------------------------------------------------- the panel files
class PanelWriter(WriterRing):
    """The panel files behind the ring of utils/writer_ring.py:

        slot = pw.acquire({"images": (h, w), ...})   # waits for the slot's writer; slot.views[name]: zeroed (3,h,w) uint8 canvases
        ... the panel kernels paint the canvases ...
        pw.commit(slot, n_iter)                      # ONE asynchronous copy device -> host, one event, the job is queued

    A writer waits for the slot's event and saves out_dir/iter_<n_iter>_<name>.png with Pillow; `on_image(name, chw, n_iter)`
    (tensorboard's add_image, where it imports) is called with the same host array."""

    def __init__(self, out_dir, writers=2, depth=2, on_image=None, alloc=_cuda_alloc, event=_cuda_event):
        self.out_dir, self.on_image = out_dir, on_image
        os.makedirs(out_dir, exist_ok=True)
        super().__init__(writers, depth, alloc, event, thread_name="weclip-panel")

    def acquire(self, shapes):
        slot = self.next_slot()
        used = self.carve(slot, [(name, (3, h, w), torch.uint8) for name, (h, w) in shapes.items()])
        slot.dev[:used].zero_()                          # the grids' borders: the kernels write the tiles only
        slot.layout = [(name, slot.spans[name][0], h, w) for name, (h, w) in shapes.items()]
        return slot

    def _write(self, slot, n_iter):
        from PIL import Image
        slot.copied.synchronize()
        for name in slot.spans:
            chw = self.host(slot, name)
            Image.fromarray(np.ascontiguousarray(chw.transpose(1, 2, 0)), mode="RGB").save(
                os.path.join(self.out_dir, f"iter_{n_iter}_{name}.png"))
            if self.on_image is not None:
                self.on_image(name, chw, n_iter)


# ---------------------------------------------------------------------------------------------- the driver
class Trainer:
    """cfg: load_config(); args: build_parser().parse_args().  model: a ready WeCLIP instead of the one built from
    cfg.clip_init (embedding, tests).  rank_dump_dir: every rank writes `rank<r>.pth` (trainable parameters, iteration,
    model.iter_num, the validation histograms) there at the end of fit() -- a cross-rank check, not part of the work_dir."""

    seed = 1                                             # setup_seed(1), :322

    def __init__(self, cfg, args, model=None, rank_dump_dir=None, timestamp=None):
        from . import _lib as L
        from .datasets import DeviceLoader
        from .validate import Validator
        L.require_gpu()
        self.cfg, self.args, self.rank_dump_dir = cfg, args, rank_dump_dir
        ddp = dist.is_available() and dist.is_initialized()
        self.rank, self.world = (dist.get_rank(), dist.get_world_size()) if ddp else (0, 1)
        self.kind = getattr(args, "dataset", "voc")
        self.max_iters = int(args.max_iters if getattr(args, "max_iters", None) is not None else cfg.train.max_iters)
        self.save_after = int(args.save_after if getattr(args, "save_after", None) is not None else SAVE_AFTER[self.kind])
        self.log_path = prepare_work_dir(cfg, timestamp, create=self.rank == 0)
        self.metrics_path = os.path.join(cfg.work_dir.dir, "metrics.jsonl")
        self.val_metrics_path = os.path.join(cfg.work_dir.dir, "val_metrics.jsonl")
        setup_seed(self.seed)

        ds = cfg.dataset
        if self.kind in ("voc", "seg"):
            from .datasets.voc import VOC12ClsDataset as ClsDataset, VOC12SegDataset as SegDataset
            val_stage = "train"                          # dist_clip_voc.py:162
        else:
            from .datasets.coco import CocoClsDataset as ClsDataset, CocoSegDataset as SegDataset
            val_stage = "val"                            # dist_clip_coco.py:163
        if self.kind == "seg":                          # ground-truth masks, label-aware augmentation (DeviceSegAugment)
            self.train_dataset = SegDataset(root_dir=ds.root_dir, name_list_dir=ds.name_list_dir, split=cfg.train.split,
                                            stage="train", aug=True, crop_size=ds.crop_size, img_fliplr=True,
                                            ignore_index=ds.ignore_index, num_classes=ds.num_classes)
        else:
            self.train_dataset = ClsDataset(root_dir=ds.root_dir, name_list_dir=ds.name_list_dir, split=cfg.train.split,
                                            stage="train", aug=True, resize_range=ds.resize_range, rescale_range=ds.rescale_range,
                                            crop_size=ds.crop_size, img_fliplr=True, ignore_index=ds.ignore_index,
                                            num_classes=ds.num_classes)
        self.val_dataset = SegDataset(root_dir=ds.root_dir, name_list_dir=ds.name_list_dir, split=cfg.val.split, stage=val_stage,
                                      aug=False, ignore_index=ds.ignore_index, num_classes=ds.num_classes)
        threads, prefetch = getattr(args, "threads", 8), getattr(args, "prefetch", 2)
        self.train_loader = DeviceLoader(self.train_dataset, batch_size=cfg.train.samples_per_gpu, shuffle=True, drop_last=True,
                                         seed=self.seed, rank=self.rank, world=self.world, threads=threads, prefetch=prefetch)
        self.val_loader = DeviceLoader(self.val_dataset, batch_size=1, shuffle=False, rank=self.rank, world=self.world,
                                       threads=threads, prefetch=prefetch)
        # decided from the global sizes, so that under DP every rank takes the same branch (the smallest share is n // world)
        if len(self.train_dataset) // self.world < int(cfg.train.samples_per_gpu):
            raise RuntimeError("Trainer: the training split holds fewer images than one batch per rank")

        self.model = model if model is not None else self.build_model()
        self.model.train()
        opt, sch = cfg.optimizer, cfg.scheduler
        self.optimizer_type = optimizer_type(cfg, args)
        betas = opt.get("betas", (0.9, 0.999) if self.optimizer_type == "SGD" else None)      # SGD ignores them
        if betas is None:
            raise KeyError("optimizer.betas is missing from the config (only optimizer.type SGD does without it)")
        self.opt = make_optimizer(self.model, lr=float(opt.learning_rate), weight_decay=float(opt.weight_decay),
                                  betas=tuple(float(b) for b in betas), warmup_iter=int(sch.warmup_iter),
                                  max_iter=self.max_iters, warmup_ratio=float(sch.warmup_ratio), power=float(sch.power),
                                  type=self.optimizer_type)
        self.reg = reg_settings(cfg, args)
        self.panel_iters = max(0, int(getattr(args, "panel_iters", 0) or 0))
        self.snapshot = self.panel_writer = self._last_inputs = None
        if self.panel_iters and self.rank == 0:          # without the flag the step is the parent's: same launches, same graph
            from .utils.panels import StepSnapshot
            self.snapshot = StepSnapshot()
        if self.kind == "seg":
            self.step = LoggedSupervisedTrainStep(self.model, self.opt, ignore_index=ds.ignore_index,
                                                  graph=bool(getattr(args, "graph", True)), reg=self.reg, panels=self.snapshot)
        else:
            self.step = LoggedTrainStep(self.model, self.opt, radius=getattr(args, "radius", 8), ignore_index=ds.ignore_index,
                                        graph=bool(getattr(args, "graph", True)), reg=self.reg, panels=self.snapshot)
        self.validator = Validator(self.model, ds.num_classes, self.rank, self.world)
        dev = next(self.model.parameters()).device
        # window sums of (loss, seg_loss, attn_loss[, reg_loss with --reg_loss]); seg: (loss, seg_loss[, reg_loss])
        self.acc = torch.zeros((2 if self.kind == "seg" else 3) + (self.reg is not None), device=dev, dtype=torch.float32)
        self.window = 0                                                 # steps in the window (host)
        self.n_iter = 0
        self.time0 = datetime.datetime.now().replace(microsecond=0)
        self._batches = None
        self.writer = None
        if self.rank == 0:
            try:
                from torch.utils.tensorboard import SummaryWriter
                self.writer = SummaryWriter(cfg.work_dir.tb_logger_dir)
            except ImportError:
                pass
        if self.snapshot is not None:
            on_image = None
            if self.writer is not None:
                on_image = lambda name, chw, n: self.writer.add_image("train/" + name, chw, global_step=n)      # noqa: E731
            self.panel_writer = PanelWriter(os.path.join(cfg.work_dir.dir, "panels"), on_image=on_image)
        if getattr(args, "resume", None):
            self.resume(args.resume)

    def build_model(self):
        return build_model(self.cfg, self.kind, getattr(self.args, "reference_root", None))

    # ---- one iteration --------------------------------------------------------------------------------------------
    def _next_batch(self):
        """Endless over epochs (:240-244): every pass over the DeviceLoader is one epoch and moves on to the next."""
        while True:
            if self._batches is None:
                self._batches = iter(self.train_loader)
            try:
                return next(self._batches)
            except StopIteration:
                self._batches = None

    def step_once(self):
        """One training iteration -> the step's (loss, seg_loss, attn_loss[, reg_loss]) device scalars.  No host read."""
        if self.kind == "seg":
            return self._seg_step_once()
        from .datasets import labels_from_onehot
        _, inputs, _, img_box = self._next_batch()
        self._last_inputs = inputs
        labels = labels_from_onehot(self.train_loader.last_cls_labels)      # the host copy: graph mode needs explicit labels
        out = self.step(inputs, labels=labels) if self.reg is None else self.step(inputs, labels=labels, img_box=img_box)
        self.acc.add_(torch.stack(out))
        self.window += 1
        self.n_iter += 1
        return out

    def _seg_step_once(self):
        """--dataset seg: (inputs, labels) of the batch go straight to the step, the labels stay on the device; with
        --reg_loss the batch's img_box (DeviceLoader.last_img_box, a device tensor) goes with them."""
        _, inputs, labels, _ = self._next_batch()
        self._last_inputs = inputs
        if self.reg is None:
            out = (self.step(inputs, labels),)
        else:
            out = self.step(inputs, labels, self.train_loader.last_img_box)
        self.acc.add_(torch.stack((out[0], self.step.ce) + tuple(out[1:])))
        self.window += 1
        self.n_iter += 1
        return out

    def render_panels(self):
        """Rank 0 with --panel_iters: the panel set of the step that just ran, from the step's snapshot and the batch's input
        images, painted into a slot of the PanelWriter's ring.  Kernels and one asynchronous copy on the stream: no forward
        (model.iter_num stays), no host read.  -> the slot (its views are valid until the ring comes round), or None."""
        if self.panel_writer is None or self.snapshot.seg is None:
            return None
        from .msc_flip import resize_argmax
        from .utils import panels as P
        snap, imgs = self.snapshot, self._last_inputs.detach().float().contiguous()
        B, _, H, W = imgs.shape
        geo = P.grid_geometry(B, H, W, 2)
        label_name = "gt_label" if self.kind == "seg" else "pseudo_label"
        shapes = {name: (geo.canvas_h, geo.canvas_w) for name in ("images", label_name, "prediction", "seg_conf")}
        if snap.rows is not None:
            ageo = P.grid_geometry(B, 224, 224, 4, colmajor=True)
            shapes.update({f"attn_pred_{j}": (ageo.canvas_h, ageo.canvas_w) for j in range(4)})
        slot = self.panel_writer.acquire(shapes)
        v = slot.views
        conf = torch.softmax(snap.seg, dim=1)[:, 1:].contiguous()        # the head's confidence without its background channel
        P.tensorboard_image(imgs, conf, out=(v["images"], v["seg_conf"]))
        P.paint_labels(snap.label, v[label_name], geo)
        pred = torch.stack([resize_argmax(snap.seg[b], (H, W)) for b in range(B)])
        P.paint_labels(pred, v["prediction"], geo)
        if snap.rows is not None:
            for j in range(4):
                P.attn_rows_grid([snap.rows[:, j]], n_row=4, out=v[f"attn_pred_{j}"])
        self.panel_writer.commit(slot, self.n_iter)
        return slot

    def _seg_log(self):
        """--dataset seg: the window's loss sums and its confusion matrix in ONE device-to-host read; the matrix is then
        zeroed on the stream.  pAcc / mAcc / mIoU are those of the whole window (seg_log_record)."""
        hist = self.step.hist
        host = torch.cat([self.acc.double(), hist.flatten().double()]).cpu().tolist() if self.rank == 0 else None
        self.acc.zero_()
        hist.zero_()
        steps, self.window = self.window, 0
        if host is None:
            return None
        rec = seg_log_record(self.n_iter, self.opt.param_groups[0]["lr"], host, steps, hist.shape[0])
        delta, eta = cal_eta(self.time0, max(self.n_iter, 1), self.max_iters)
        LOG.info(format_seg_log_line(rec["iter"], delta, eta, rec["lr"], rec["seg_loss"], rec["pAcc"], rec["mAcc"], rec["miou"],
                                     rec.get("reg_loss")))
        append_metrics(self.metrics_path, rec)
        if self.writer is not None:
            self.writer.add_scalars("train/loss", {"seg_loss": rec["seg_loss"]}, global_step=self.n_iter)
        return rec

    def log(self):
        """The log line of :269-282 for the window since the last call: ONE device-to-host read (loss sums + counts).
        pseudo_seg_mAcc is the LAST step's, as the reference's.  Needs at least one step since the last call."""
        if self.window == 0:
            raise RuntimeError("Trainer.log: no step since the last log line (there is no window to average)")
        if self.kind == "seg":
            return self._seg_log()
        host = torch.cat([self.acc.double(), self.step.counts.double()]).cpu().tolist() if self.rank == 0 else None
        self.acc.zero_()
        steps, self.window = self.window, 0
        if host is None:
            return None
        rec = log_record(self.n_iter, self.opt.param_groups[0]["lr"], host, steps)
        delta, eta = cal_eta(self.time0, max(self.n_iter, 1), self.max_iters)
        LOG.info(format_log_line(rec["iter"], delta, eta, rec["lr"], rec["seg_loss"], rec["attn_loss"], rec["pseudo_seg_mAcc"],
                                 rec.get("reg_loss")))
        append_metrics(self.metrics_path, rec)
        if self.writer is not None:
            self.writer.add_scalars("train/loss", {"seg_loss": rec["seg_loss"], "attn_loss": rec["attn_loss"]}, global_step=self.n_iter)
        return rec

    def validate(self):
        """Validator.run over the val split -> (seg_score, cam_score), logged as :291-294 on rank 0.  The model counts every
        forward in `iter_num`, validation included (the reference's seg-trans switch at 15000 counts them too): afterwards the
        counter stands where a single process validating ALL images leaves it, on every rank."""
        before = self.model.iter_num
        seg_score, cam_score = self.validator.run(self.val_loader)
        self.model.iter_num = before + len(self.val_dataset)
        if self.rank == 0:
            if self.kind != "seg":                       # the supervised variant has no CAM leg: cam_score is None
                LOG.info("cams score:")
                LOG.info(cam_score)
            LOG.info("segs score:")
            LOG.info(seg_score)
            brief = lambda s: None if s is None else {k: float(s[k]) for k in ("pAcc", "mAcc", "miou")}      # noqa: E731
            append_metrics(self.val_metrics_path, {"iter": self.n_iter, "seg": brief(seg_score), "cam": brief(cam_score),
                                                   "seg_hist_sum": int(self.validator.seg_hist_host.sum()),
                                                   "cam_hist_sum": None if cam_score is None else int(self.validator.cam_hist_host.sum())})
        return seg_score, cam_score

    def save_model(self):
        """Rank 0: WeCLIP_model_iter_N.pth = model.state_dict(), the reference's format (what test_msc_flip_* and
        MscFlipEvaluator load)."""
        if self.rank != 0:
            return None
        path = checkpoint_paths(self.cfg.work_dir.ckpt_dir, self.n_iter)[0]
        torch.save(self.model.state_dict(), path)
        return path

    def save_state(self):
        """Rank 0: train_state_iter_N.pth beside the model file: optimizer, iteration, model.iter_num and loader epoch as
        they stand now (fit() writes it after the validation, whose forwards model.iter_num counts)."""
        if self.rank != 0:
            return None
        path = checkpoint_paths(self.cfg.work_dir.ckpt_dir, self.n_iter)[1]
        torch.save({"optimizer": self.opt.state_dict(), "optimizer_type": self.optimizer_type,
                    "global_step": self.opt.global_step, "iter": self.n_iter,
                    "model_iter_num": self.model.iter_num, "loader_epoch": self.train_loader.epoch}, path)
        return path

    def save(self):
        """Both files of the current iteration -> (model path, state path) on rank 0."""
        return self.save_model(), self.save_state()

    def resume(self, model_path):
        """Parameters, optimizer tensors, iteration, model.iter_num and the loader epoch of a checkpoint pair: the LR schedule
        and the seg-trans switch continue where they stopped.  The dropout and augmentation streams restart, and the loader
        starts a fresh epoch, so the continuation is not bit-equal to the uninterrupted run."""
        state = torch.load(state_path_of(model_path), map_location="cpu", weights_only=False)
        check_state_optimizer(state, self.optimizer_type, state_path_of(model_path))
        self.model.load_state_dict(torch.load(model_path, map_location="cpu"), strict=True)
        self.opt.load_state_dict(state["optimizer"])
        self.opt.global_step = int(state["global_step"])
        self.n_iter = int(state["iter"])
        if self.step.reg is not None:
            self.step.reg.step_num = self.n_iter         # the term's start counts the training iterations
        self.model.iter_num = int(state["model_iter_num"])
        self.train_loader.set_epoch(int(state["loader_epoch"]))
        self._batches = None
        if self.rank == 0:
            LOG.info("resumed from %s at iteration %d", model_path, self.n_iter)

    def fit(self, until=None):
        """The loop of :238-294 up to `until` (default: max_iters)."""
        cfg = self.cfg.train
        stop = self.max_iters if until is None else min(int(until), self.max_iters)
        while self.n_iter < stop:
            self.step_once()
            if self.panel_iters and self.n_iter % self.panel_iters == 0:
                self.render_panels()
            if self.n_iter % cfg.log_iters == 0:
                self.log()
            if self.n_iter % cfg.eval_iters == 0:
                if self.rank == 0:
                    LOG.info("Validating...")
                if self.n_iter > self.save_after:
                    self.save_model()                    # before the validation, as :288-290
                self.validate()
                if self.n_iter > self.save_after:
                    self.save_state()                    # after it: the state holds model.iter_num as it now stands
        if self.n_iter >= self.max_iters:
            self.close()
        return True

    def close(self):
        if self._batches is not None:
            self._batches.close()                        # ends the loader's decode threads
            self._batches = None
        if self.panel_writer is not None:
            pw, self.panel_writer = self.panel_writer, None
            pw.finish()                                  # before the tensorboard writer its threads feed is closed
        if self.writer is not None:
            self.writer.close()
        if self.rank_dump_dir:
            params = torch.cat([p.detach().flatten() for p in self.model.get_param_groups()[3]]).cpu()
            torch.save({"rank": self.rank, "params": params, "iter": self.n_iter, "model_iter_num": self.model.iter_num,
                        "seg_hist": self.validator.seg_hist.cpu(), "cam_hist": self.validator.cam_hist.cpu()},
                       os.path.join(self.rank_dump_dir, f"rank{self.rank}.pth"))
            self.rank_dump_dir = None


def main(argv=None):
    args = build_parser().parse_args(argv)
    cfg = load_config(args.config, crop_size=args.crop_size, work_dir=args.work_dir)
    world = init_distributed()
    try:
        # WECLIP_TRAIN_RANK_DUMP=<dir>: Trainer(rank_dump_dir=...), the cross-rank check of the DP test
        trainer = Trainer(cfg, args, rank_dump_dir=os.environ.get("WECLIP_TRAIN_RANK_DUMP") or None)
        if trainer.rank == 0:
            setup_logger(trainer.log_path)
            LOG.info("\noptimizer: %s\nargs: %s", trainer.optimizer_type, args)
            LOG.info("\nconfigs: %s", cfg)
        trainer.fit()
        trainer.close()
        if world > 1:
            dist.barrier()
    finally:
        if world > 1 and dist.is_initialized():
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
