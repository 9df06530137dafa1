"""reference WeCLIP_model/segformer_head_seg.py: the seg variant's head.  It differs from segformer_head.py only in
comments, so this module re-exports the same classes (same parameter names)."""
from .segformer_head import MLP, SegFormerHead  # noqa: F401
