"""HIP-backed counterpart of the reference `clip` package (model, myAtt, clip_tool, utils, tokenize)."""
from .clip import load, build_model, tokenize, set_bpe_path  # noqa: F401


def __getattr__(name):
    """`clip.SeedEvaluator` and the wrappers of clip/cam_seeds.py (sweep, masks and scores of the dumpers' maps on the device),
    imported on first use: the dumpers' plain run never loads them."""
    if name in ("SeedEvaluator", "sweep_confusion", "seed_labels", "merge_labels", "sweep_path"):
        from . import cam_seeds
        return getattr(cam_seeds, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
