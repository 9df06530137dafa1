"""The training step around `WeCLIP.forward` (what reference scripts/dist_clip_voc.py:238-267 does
per iteration) and its data-parallel form: one process per GPU, image batch sharded over ranks,
one RCCL all-reduce of the adapter+decoder gradients (5,985,045 fp32 = 23.9 MB in ONE flat bucket;
the frozen CLIP encoder is replicated and never reduced).  The reference itself is single-GPU
(SURVEY.md §0-3); this is the DP launcher the build adds beside it.
"""
import os

import torch
import torch.distributed as dist
import torch.nn.functional as F

from .utils.camutils import cams_to_affinity_label, get_mask_by_radius
from .utils.losses import (DenseEnergyLoss, get_aff_loss, get_aff_loss_fused, get_ce_loss_fused, get_energy_loss_fused,
                           get_seg_loss, get_seg_loss_fused)
from .utils.optimizer import PolyWarmupAdamW, PolyWarmupSGD

OPTIMIZER_TYPES = ("AdamW", "SGD")                  # optimizer.type of the YAML, compared without letter case


def make_optimizer(model, lr=2e-4, weight_decay=0.01, betas=(0.9, 0.999), warmup_iter=50, max_iter=30000,
                   warmup_ratio=1e-6, power=1.0, type="AdamW"):
    """configs/voc_attn_reg.yaml:29-38 + scripts/dist_clip_voc.py:196-234: only group 3 is non-empty
    and runs at 10x the base lr.  type: "AdamW" (PolyWarmupAdamW) or "SGD" (PolyWarmupSGD, the reference's second optimizer,
    over the same groups; it ignores betas), in any letter case."""
    cls = {"adamw": PolyWarmupAdamW, "sgd": PolyWarmupSGD}.get(str(type).lower())
    if cls is None:
        raise ValueError(f"make_optimizer: type must be one of {', '.join(OPTIMIZER_TYPES)}, got {type!r}")
    g = model.get_param_groups()
    groups = [
        {"params": g[0], "lr": lr, "weight_decay": weight_decay},
        {"params": g[1], "lr": 0.0, "weight_decay": 0.0},
        {"params": g[2], "lr": lr * 10, "weight_decay": weight_decay},
        {"params": g[3], "lr": lr * 10, "weight_decay": weight_decay},
    ]
    return cls(groups, lr=lr, weight_decay=weight_decay, betas=list(betas),
               warmup_iter=warmup_iter, max_iter=max_iter, warmup_ratio=warmup_ratio, power=power)


class RegTerm:
    """The regularised (dense energy) loss as a term of a training step: `reg` (RegTerm.of(None) is None: no term) is a dict
    or an object with any of
        coef (0.01): the term's weight in the step's loss;  start_iter (0): the term is active at 1-based step numbers > start_iter;
        weight (1e-7), sigma_rgb (15), sigma_xy (100), scale_factor (0.5): the DenseEnergyLoss, the lineage's parameters.
        bilateral ("exact"): the term's filter, "exact" or "lattice" (utils.losses).  The lattice's
        workspaces are allocated once per (batch, classes, scaled size) and kept; the filter is part of the graph signature.
    `coef` and `start_iter` are this package's choice (the reference checkout never calls its get_energy_loss; DESIGN.md
    section 15.2).  scale_factor must be 1, 0.5 or 0.25 (utils.losses.get_energy_loss_fused)."""

    DEFAULTS = dict(coef=0.01, weight=1e-7, sigma_rgb=15, sigma_xy=100, scale_factor=0.5, start_iter=0, bilateral="exact")

    @classmethod
    def of(cls, reg):
        return None if reg is None else cls(reg)

    def __init__(self, reg):
        if isinstance(reg, dict):
            unknown = set(reg) - set(self.DEFAULTS)
            if unknown:
                raise ValueError(f"reg: unknown keys {sorted(unknown)} (known: {sorted(self.DEFAULTS)})")
            reg = type("reg", (), reg)
        for k, v in self.DEFAULTS.items():
            setattr(self, k, getattr(reg, k, v))
        if float(self.scale_factor) not in (1.0, 0.5, 0.25):
            raise ValueError(f"reg: scale_factor must be 1, 0.5 or 0.25, got {self.scale_factor}")
        self.start_iter = int(self.start_iter)
        self.layer = DenseEnergyLoss(self.weight, self.sigma_rgb, self.sigma_xy, self.scale_factor, self.bilateral)   # ValueError
        if self.bilateral != "exact":
            self.layer.workspace_cache = {}
        self.step_num = 0                    # steps begun (1-based number of the current one)

    def begin_step(self):
        """Counts the step that begins and returns whether the term is active in it."""
        self.step_num += 1
        return self.step_num > self.start_iter

    def box_buffer(self, img):
        return torch.empty(img.shape[0], 4, device=img.device, dtype=torch.int32)

    def fill_box(self, buf, img_box, img):
        """img_box (None: the whole image, rows, or a tensor on either side) -> the static (B, 4) int32 buffer, no host read."""
        if img_box is None:
            img_box = [[0, img.shape[2], 0, img.shape[3]]] * img.shape[0]
        buf.copy_(torch.as_tensor(img_box).reshape(buf.shape))

    def add(self, loss, img, seg, label, img_box, active):
        """(loss + coef * energy, energy) when active, else (loss, 0): energy = the DenseEnergyLoss of the up-sampled `seg`."""
        if not active:
            return loss, torch.zeros((), device=seg.device, dtype=torch.float32)
        energy = get_energy_loss_fused(img, seg, label, img_box, self.layer)[0]
        return loss + self.coef * energy, energy.detach()


class GradBucket:
    """Flat fp32 bucket aliasing every trainable gradient, so the DP exchange is one collective."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        # every gradient starts on a 16-byte boundary (the fused AdamW and SGD steps and the split-K reductions use 16-byte accesses):
        # an odd-sized tensor (the 21-class bias) is followed by <= 3 padding elements, which stay zero
        offs, off = [], 0
        for p in self.params:
            offs.append(off)
            off = (off + p.numel() + 3) & ~3
        self.flat = torch.zeros(off, device=self.params[0].device, dtype=torch.float32)
        self.offsets = offs
        for p, o in zip(self.params, offs):
            p.grad = self.flat[o:o + p.numel()].view_as(p)

    def zero(self):
        self.flat.zero_()

    def all_reduce_mean(self, group=None):
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
            self.flat.div_(dist.get_world_size(group))


class _StepBase:
    """What the training steps of both model variants share: optimizer, gradient bucket and the engines' `direct_grads`,
    the backward half of a step, the gradient exchange, and the eager -> capture -> replay sequence around a HIP graph.
    A variant supplies `_fwd_bwd` (its forward and losses, ending in `_backward`) and, for graph mode, `_signature`,
    `_static_target` and `_refill`."""

    def __init__(self, model, optimizer, bucket, graph, reg):
        self.model = model
        self.reg = RegTerm.of(reg)
        self.opt = optimizer or make_optimizer(model)
        self.bucket = GradBucket(model.get_param_groups()[3]) if bucket else None
        self.graph = bool(graph)
        self._graphs = {}
        self._pool = None
        # the HIP head and the insert engine write their gradients straight into the views of THIS bucket (zeroed each step,
        # each gradient written exactly once per backward; a .grad that lies elsewhere is accumulated through autograd as
        # usual); a step without a bucket clears the opt-in
        rng = None
        if self.bucket is not None and os.environ.get("WECLIP_DIRECT_GRADS", "1") != "0":
            lo = self.bucket.flat.data_ptr()
            rng = (lo, lo + 4 * self.bucket.flat.numel())
        for owner in (getattr(model, "head_engine", None), getattr(model, "comer", None)):
            if owner is not None:
                owner.direct_grads = rng

    def _reduce_grads(self):
        """One exchange per step: mean of the trainable gradients over the data-parallel ranks."""
        if self.bucket is not None:
            return self.bucket.all_reduce_mean()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            # no flat bucket: reduce the gradients tensor by tensor (slower, same result) rather than let ranks diverge
            world = dist.get_world_size()
            for p in self.model.get_param_groups()[3]:
                if p.grad is not None:
                    dist.all_reduce(p.grad, op=dist.ReduceOp.SUM)
                    p.grad.div_(world)

    def _backward(self, losses, img, seg, label, img_box, reg_active):
        """The half of a step behind the variant's `losses` (total first): energy term of `seg` against `img` and the `label`
        map, zeroed gradients, backward.  -> the detached scalars, total first, the energy last when `reg` is set."""
        loss = losses[0]
        if self.reg is not None:
            loss, energy = self.reg.add(loss, img, seg, label, img_box, reg_active)
            losses = (loss,) + tuple(losses[1:]) + (energy,)
        if self.bucket is not None:
            self.bucket.zero()
        else:
            self.opt.zero_grad()
        loss.backward()
        if img.is_cuda:      # backward nodes of a head that ran beside the CAM chain execute on the model's side stream
            cur = torch.cuda.current_stream()
            for s in getattr(self.model, "side_streams", lambda: [])():
                cur.wait_stream(s)
        return tuple(l.detach() for l in losses)

    def __call__(self, img, target, img_box=None, names=None):
        """One step on `img` and the variant's `target`; a step of one scalar returns it bare, any other a tuple."""
        active = self.reg is not None and self.reg.begin_step()
        if self.graph and target is not None and img.is_cuda and self.bucket is not None:
            out = self._graphed(img, target, img_box, active)
        else:
            out = self._fwd_bwd(img, target, None, names, img_box, active)
        self._reduce_grads()
        self.opt.step()
        return out[0] if len(out) == 1 else out

    def _graphed(self, img, target, img_box, reg_active):
        """HIP-graph replay: per batch signature the first step runs eagerly on the static buffers (it warms every lazy
        initialisation), the second captures, every later one replays.  Whether the energy term is active is part of the
        signature; `img_box` goes through a static (B, 4) buffer."""
        m = self.model
        sig = self._signature(img, target) + ((True,) if reg_active else ())
        if reg_active and self.reg.bilateral != "exact":
            sig += (self.reg.bilateral,)
        ent = self._graphs.get(sig)
        first = ent is None
        if first:
            ent = self._graphs[sig] = {"graph": None, "img": torch.empty(img.shape, device=img.device, dtype=torch.float32),
                                       "target": self._static_target(img, target),
                                       "box": self.reg.box_buffer(img) if reg_active else None}
        else:
            self._refill(ent["target"], target)
        ent["img"].copy_(img)
        if reg_active:
            self.reg.fill_box(ent["box"], img_box, img)
        if first:
            return self._fwd_bwd(ent["img"], target, ent["target"], None, ent["box"], reg_active)
        if ent["graph"] is None:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            it = m.iter_num
            # thread_local: other threads (RCCL's watchdog polling its events, the autograd workers allocating) must not
            # abort the capture; the kernels the autograd workers launch on the capturing stream are captured all the same
            with torch.cuda.graph(g, pool=self._pool, capture_error_mode="thread_local"):
                ent["out"] = torch.stack(self._fwd_bwd(ent["img"], target, ent["target"], None, ent["box"], reg_active))
            m.iter_num = it                  # the capture ran forward()'s counter once without executing a step
            self._pool = self._pool or g.pool()
            ent["graph"] = g
        ent["graph"].replay()
        m.iter_num += 1
        return tuple(ent["out"].clone())     # the graph's pool memory is rewritten by the next replay


class TrainStep(_StepBase):
    """forward -> losses -> backward -> (DP: gradient all-reduce) -> optimizer step (PolyWarmupAdamW, or PolyWarmupSGD from
    make_optimizer(type="SGD")).  This class holds the weakly supervised variant's forward, `losses` (the override point) and PairPlan statics; everything behind the losses is `_StepBase`.

    graph=True (CUDA tensors + explicit `labels` only): forward + losses + backward of a batch signature
    (image shape, number of (image, class) pairs, max classes per image, affinity branch) are captured once into a
    HIP graph and replayed from then on -- one graph launch instead of ~420 kernel launches through Python, which is
    what the step costs on the host otherwise (BENCH_r01: 9.8 ms of enqueue per 14.5 ms step).  Inputs are copied
    into static buffers (images; the pair index tensors via PairPlan.update); the gradient all-reduce and the
    optimizer stay outside the graph (RCCL and the host-computed learning-rate schedule).

    pad_plans (default on in graph mode): the signature is BUCKETED (clip_tool.PairPlan pad=True: pair count to a multiple
    of 8 with dropped dummy pairs, channel capacity K to the next even number), so batches whose images carry 1..5
    classes share a few graphs instead of one per distinct (pair count, max classes); losses, gradients and parameters
    stay bit-identical to the unpadded eager step (tests/test_graph_step_gpu.py).

    reg (default None: nothing changes): a `RegTerm` description.  The loss becomes seg_loss + 0.1 * attn_loss + coef * energy
    at step numbers > start_iter, energy = the dense energy loss of the up-sampled logits against the step's input image and
    pseudo labels inside `img_box` (an argument of the call: None = the whole image, or (B, 4) rows (y0, y1, x0, x1) on either
    side); the step then returns a fourth value, the energy before `coef` (zero while the term is inactive)."""

    def __init__(self, model, optimizer=None, radius=8, ignore_index=255, bucket=True, graph=False, pad_plans=True, reg=None):
        super().__init__(model, optimizer, bucket, graph, reg)
        self.radius, self.ignore = radius, ignore_index
        self._mask = {}
        self.pad_plans = bool(pad_plans)

    def mask(self, h, w, device):
        key = (h, w, str(device))
        if key not in self._mask:
            self._mask[key] = get_mask_by_radius(h, w, self.radius, device=device)
        return self._mask[key]

    def losses(self, seg, cam, attn_pred):
        h, w = cam.shape[1] // 16, cam.shape[2] // 16
        if seg.is_cuda:     # label->affinity-label + affinity loss, and up-sampling + both CE terms, fused (csrc/losses.hip)
            attn_loss = get_aff_loss_fused(attn_pred, cam, radius=self.radius, ignore_index=self.ignore)
            seg_loss = get_seg_loss_fused(seg, cam, ignore_index=self.ignore)
        else:
            aff_label = cams_to_affinity_label(cam, mask=self.mask(h, w, cam.device), ignore_index=self.ignore)
            attn_loss, _, _ = get_aff_loss(attn_pred, aff_label)
            segs = F.interpolate(seg, size=cam.shape[1:], mode="bilinear", align_corners=False)
            seg_loss = get_seg_loss(segs, cam.long(), ignore_index=self.ignore)
        return seg_loss + 0.1 * attn_loss, seg_loss, attn_loss

    def _fwd_bwd(self, img, labels, plan=None, names=None, img_box=None, reg_active=False):
        kw = {"plan": plan} if plan is not None else {}
        seg, cam, attn_pred = self.model(img, names if names is not None else [""] * img.shape[0], labels=labels, **kw)
        return self._backward(self.losses(seg, cam, attn_pred), img, seg, cam, img_box, reg_active)

    def __call__(self, img, names=None, labels=None, img_box=None):
        return super().__call__(img, labels, img_box, names)

    # ------------------------------------------------------------- graph mode: the signature, and a PairPlan as static target
    def _signature(self, img, labels):
        from .clip.clip_tool import PairPlan
        m = self.model
        seg_trans = (m.iter_num + 1) > m.seg_trans_after
        return tuple(img.shape), PairPlan.signature(labels, self.pad_plans), bool(seg_trans), bool(m.training)

    def _static_target(self, img, labels):
        from .clip.clip_tool import PairPlan
        m = self.model
        return PairPlan(labels, m.fg_text_features.shape[0], m.bg_text_features.shape[0], img.device, pad=self.pad_plans)

    def _refill(self, plan, labels):
        plan.update(labels)


class SupervisedTrainStep(_StepBase):
    """forward -> cross-entropy -> backward -> (DP: gradient all-reduce) -> optimizer step (AdamW or SGD) for the fully supervised variant
    (WeCLIP_model/model_attn_aff_voc_seg.py), whose labels are ground-truth masks.  The loss is
    F.cross_entropy(F.interpolate(seg, label.shape[1:], bilinear, align_corners=False), label, ignore_index): the
    reference ships no training script for this variant, so the loss is this package's choice; on the GPU
    it runs fused (utils.losses.get_ce_loss_fused: the up-sampled logits are never materialised).

    `step(img, label)`: img (B, 3, H, W) and label (B, Hl, Wl) integer device tensors the caller has prepared (any
    augmentation happens before); returns the detached loss.  graph=True (CUDA tensors, with a bucket): forward + loss +
    backward are captured once per (image shape, label shape, training flag) -- the first step of a signature runs eagerly,
    the second captures -- and replayed from static input buffers; the all-reduce and the optimizer stay outside the graph.
    That sequence, like everything else behind `loss`, is `_StepBase`'s, the one TrainStep runs.

    reg (default None: nothing changes): a `RegTerm` description, as in TrainStep.  The loss becomes ce + coef * energy at step
    numbers > start_iter, with the ground-truth label and `img_box` (third argument of the call; None = the whole image); the
    step then returns (loss, energy before `coef`), the energy zero while the term is inactive."""

    def __init__(self, model, optimizer=None, ignore_index=255, bucket=True, graph=False, reg=None):
        super().__init__(model, optimizer, bucket, graph, reg)
        self.ignore = int(ignore_index)

    def loss(self, seg, label):
        if seg.is_cuda:
            return get_ce_loss_fused(seg, label, ignore_index=self.ignore)
        segs = F.interpolate(seg, size=label.shape[1:], mode="bilinear", align_corners=False)
        return F.cross_entropy(segs, label.long(), ignore_index=self.ignore)

    def _fwd_bwd(self, img, label, static=None, names=None, img_box=None, reg_active=False):
        label = label if static is None else static
        seg = self.model(img, mode="train")
        return self._backward((self.loss(seg, label),), img, seg, label, img_box, reg_active)

    step = _StepBase.__call__

    # ------------------------------------------------------- graph mode: the signature, and an int64 label buffer as static target
    def _signature(self, img, label):
        return tuple(img.shape), tuple(label.shape), bool(self.model.training)

    def _static_target(self, img, label):
        return torch.empty(label.shape, device=img.device, dtype=torch.int64).copy_(label)

    def _refill(self, buf, label):
        buf.copy_(label)
