"""reference WeCLIP_model/Decoder/TransDecoder_seg.py: the seg variant's decoder.  It differs from TransDecoder.py only
in comments, so this module re-exports the same classes (same parameter names)."""
from .TransDecoder import DecoderTransformer, LayerNorm, QuickGELU, ResidualAttentionBlock, Transformer  # noqa: F401
