"""HIP-backed counterpart of the reference `clip` package (model, myAtt, clip_tool, utils, tokenize)."""
from .clip import load, build_model, tokenize, set_bpe_path  # noqa: F401
