"""What a command-line run of this package needs, whichever entry point it is (train.py, msc_flip_eval.py, predict.py): the
reference's YAML as a `Config`, the process group, the model and dataset of `--dataset`, the CRF of `--crf`, and the options
the entry points share.  A leaf module: it imports none of the entry points, and they re-export what they expose from here."""
import argparse
import contextlib
import math
import os
import re

import torch
import torch.distributed as dist

DEFAULTS = {"voc": ("configs/voc_attn_reg.yaml", "/your/path/WeCLIP/WeCLIP_model_iter_30000.pth"),      # test_msc_flip_voc.py:20-28
            "coco": ("configs/coco_attn_reg.yaml", "/your/path/WeCLIP/WeCLIP_model_iter_80000.pth"),    # test_msc_flip_coco.py:20-28
            "seg": ("configs/voc_attn_reg.yaml", "/your/path/WeCLIP/WeCLIP_model_iter_30000.pth")}      # test_msc_flip_seg.py:20-28
CRF_PARAMS = dict(iter_max=10, pos_xy_std=3, pos_w=3, bi_xy_std=64, bi_rgb_std=5, bi_w=4)               # test_msc_flip_voc.py:126-133
_SCI = re.compile(r"^[+-]?(\d+\.?\d*|\.\d+)[eE][+-]?\d+$")


# ---------------------------------------------------------------------------------------------- configuration
class Config(dict):
    """A dict with attribute access (`cfg.train.max_iters`), the part of OmegaConf the reference's scripts use."""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key) from None

    def __setattr__(self, key, value):
        self[key] = value


def _wrap(v):
    if isinstance(v, dict):
        return Config((k, _wrap(x)) for k, x in v.items())
    if isinstance(v, (list, tuple)):
        return [_wrap(x) for x in v]
    if isinstance(v, str) and _SCI.match(v.strip()):    # YAML 1.1 (PyYAML) reads `2e-4` / `1e-6` as strings: it wants a dot
        return float(v)
    return v


def load_config(path, crop_size=None, work_dir=None):
    """The reference's YAML -> Config.  Numbers spelt without a dot in the mantissa (`2e-4`) come out as floats; crop_size /
    work_dir override `dataset.crop_size` / `work_dir.dir` as the reference's command line does (:302-306)."""
    import yaml
    with open(path) as f:
        cfg = _wrap(yaml.safe_load(f))
    if crop_size is not None:
        cfg.dataset.crop_size = int(crop_size)
    if work_dir is not None:
        cfg.work_dir.dir = work_dir
    return cfg


def strict_json(v):
    """Non-finite floats -> None, recursively: `json.dumps` would write them as the bare tokens NaN / Infinity, which strict
    JSON readers refuse.  (A window's loss IS NaN when a batch's pseudo labels hold no foreground pixel, as in the reference.)"""
    if isinstance(v, dict):
        return {k: strict_json(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [strict_json(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return None
    return v


# ---------------------------------------------------------------------------------------------- the process group
def init_distributed():
    """Under `python -m torch.distributed.run`: RCCL, one rank per GPU; WECLIP_DIST_BACKEND=gloo is the rehearsal switch of
    bench.py (ranks share the GPUs that exist, gradients exchanged through the host).  Starts no processes."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("WECLIP_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)
    return world


@contextlib.contextmanager
def distributed_run():
    """The process group of a command-line run: -> (rank, world).  A run that ends well meets the other ranks in a barrier; the
    group is destroyed either way."""
    world = init_distributed()
    try:
        yield (dist.get_rank() if world > 1 else 0), world
        if world > 1:
            dist.barrier()
    finally:
        if world > 1 and dist.is_initialized():
            dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------- model, dataset, CRF
def build_model(cfg, kind="voc", reference_root=None):
    """The WeCLIP of `cfg.clip_init` for `kind` ("voc", "coco", or "seg": the supervised variant) with its text rows."""
    if reference_root:
        from . import install_dropin
        install_dropin(reference_root=reference_root)
    if kind == "voc":
        from .WeCLIP_model.model_attn_aff_voc import WeCLIP
    elif kind == "coco":
        from .WeCLIP_model.model_attn_aff_coco import WeCLIP
    else:
        from .WeCLIP_model.model_attn_aff_voc_seg import WeCLIP
    ci = cfg.clip_init
    text = None
    if ci.get("text_features"):
        rows = torch.load(ci.text_features, map_location="cuda")
        text = (rows["bg"].float(), rows["fg"].float())
    extra = {} if kind == "seg" else {"comer": bool(ci.get("comer", False))}
    return WeCLIP(num_classes=cfg.dataset.num_classes, clip_model=ci.clip_pretrain_path, embedding_dim=ci.embedding_dim,
                  in_channels=list(ci.in_channels), dataset_root_path=cfg.dataset.root_dir, device="cuda", text_features=text,
                  **extra)


def load_model(cfg, args):
    """The model of `--dataset` with the weights of `--model_path`, in eval mode."""
    model = build_model(cfg, args.dataset, args.reference_root)
    model.load_state_dict(torch.load(args.model_path, map_location="cpu"), strict=False)      # test_msc_flip_voc.py:194-196
    return model.eval()


def split_dataset(cfg, args, split, stage):
    """The Seg dataset of `--dataset` over `split` ("val" reads the label PNGs, "test" does not)."""
    ds = cfg.dataset
    if args.dataset == "coco":
        from .datasets.coco import CocoSegDataset as SegDataset
    else:
        from .datasets.voc import VOC12SegDataset as SegDataset
    return SegDataset(root_dir=ds.root_dir, name_list_dir=ds.name_list_dir, split=split, stage=stage, aug=False,
                      ignore_index=ds.ignore_index, num_classes=ds.num_classes)


def crf_of(args):
    """The DenseCRF of `--crf` / `--crf_bilateral` with the reference's parameters, or None."""
    if not args.crf:
        return None
    from .utils.dcrf import DenseCRF
    return DenseCRF(**CRF_PARAMS, bilateral=args.crf_bilateral)


# ---------------------------------------------------------------------------------------------- the shared options
def parse_scales(text):
    return [float(s) for s in str(text).split(",") if s.strip()]


def add_model_arguments(p):
    """Which model on which images at which scales: the options of msc_flip_eval.py and predict.py alike."""
    p.add_argument("--config", default=None, type=str, help="the reference's YAML (default: configs/voc_attn_reg.yaml, coco_attn_reg.yaml)")
    p.add_argument("--model_path", default=None, type=str, help="a WeCLIP_model_iter_N.pth (model.state_dict())")
    p.add_argument("--dataset", choices=("voc", "coco", "seg"), default="voc", help="which model; seg: the supervised variant on VOC")
    p.add_argument("--reference_root", type=str, default=None, help="reference checkout holding clip/clip_text.py and the BPE merges")
    p.add_argument("--scales", type=parse_scales, default=[1.0, 0.75], help="comma-separated scale factors of the multi-scale average")
    p.add_argument("--resize_long", default=512, type=int, help="resize the long side")


def add_run_arguments(p):
    """How the run goes about it: host threads and the CRF leg."""
    p.add_argument("--threads", type=int, default=8, help="decode threads of the loader")
    p.add_argument("--writers", type=int, default=4, help="host threads that write the PNG files")
    p.add_argument("--crf", action=argparse.BooleanOptionalAction, default=False,
                   help="dense CRF on the multi-scale logits (the crf_proc leg, commented out in the reference)")
    p.add_argument("--crf_bilateral", choices=("exact", "lattice"), default="exact",
                   help="the CRF's bilateral message: the exact all-pairs sum, or the permutohedral lattice (as pydensecrf)")


def fill_defaults(args):
    """`--config` / `--model_path` left out: those of the reference's script for `--dataset`.  -> args."""
    config, model_path = DEFAULTS[args.dataset]
    args.config = args.config or config
    args.model_path = args.model_path or model_path
    return args
