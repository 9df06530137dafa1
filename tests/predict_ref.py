"""A plain NumPy restatement of `wc_predict_finish` (csrc/predict.hip): the contract the GPU tests compare against.

Only the bilinear values are float32, because the device's arg-max is DEFINED by them (it must be `wc_resize_argmax`'s bit for
bit): the source rule and the lerp are those of tests/preprocess_ref.py `bilinear_resize_f32`, operation by operation.
Everything after them is float64 or integer: first-maximum arg-max, soft-max confidence, rounding, the ignore rule, the colour
from the golden table, the integer overlay, the statistics.
"""
import numpy as np

from preprocess_ref import bilinear_resize_f32


def values(src, out_hw):
    """(C,Hs,Ws) f32 -> (C,H,W) f32: ATen bilinear, align_corners=False, scale = in / out."""
    H, W = out_hw
    return np.stack([bilinear_resize_f32(np.asarray(p, np.float32), H, W) for p in src])


def confidence(src, out_hw, mode):
    """-> (best (H,W) int64: the first maximum, x (H,W) float64: 255 * conf before rounding)."""
    v = values(src, out_hw)
    best = v.argmax(0)                                        # numpy: the first maximum
    v64 = v.astype(np.float64)
    top = np.take_along_axis(v64, best[None], 0)[0]
    if mode == 0:
        conf = 1.0 / np.exp(v64 - top[None]).sum(0)
    else:
        conf = np.clip(top, 0.0, 1.0)
    return best, 255.0 * conf


def band(x, C):
    """Pixels where float32 may round the other way: 255 * conf within d = 255 (2C + 16) 2^-24 of some k + 0.5."""
    d = 255.0 * (2 * C + 16) * 2.0 ** -24
    return np.abs(x - np.floor(x) - 0.5) <= d


def finish(best, conf_u8, cmap, C, image=None, alpha256=128, ignore_below=0):
    """Everything that follows from the arg-max and the uint8 confidence, in integers: -> dict(pred, cmap, conf, overlay or None,
    stats int64 (2C + 1,)).  cmap: the (256, 3) golden VOC table."""
    conf_u8 = np.asarray(conf_u8).astype(np.int64)
    pred = np.where((ignore_below > 0) & (conf_u8 < ignore_below), 255, best).astype(np.uint8)
    colour = cmap[pred].astype(np.int64)
    overlay = None
    if image is not None:
        overlay = ((alpha256 * colour + (256 - alpha256) * image.astype(np.int64) + 128) >> 8).astype(np.uint8)
    stats = np.zeros(2 * C + 1, np.int64)
    kept = pred != 255
    stats[:C] = np.bincount(pred[kept].astype(np.int64), minlength=C)[:C]
    stats[C:2 * C] = np.bincount(pred[kept].astype(np.int64), weights=conf_u8[kept], minlength=C)[:C].astype(np.int64)
    stats[2 * C] = int((~kept).sum())
    return dict(pred=pred, cmap=colour.astype(np.uint8), conf=conf_u8.astype(np.uint8), overlay=overlay, stats=stats)


def predict_finish(src, out_hw, cmap, image=None, mode=0, alpha256=128, ignore_below=0):
    """The whole kernel: conf_u8 = floor(255 * conf + 0.5).  -> finish()'s dict plus x (255 * conf, float64) and best."""
    C = src.shape[0]
    best, x = confidence(src, out_hw, mode)
    out = finish(best, np.floor(x + 0.5), cmap, C, image=image, alpha256=alpha256, ignore_below=ignore_below)
    out.update(x=x, best=best)
    return out
