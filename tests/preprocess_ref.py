"""numpy restatement of the two new steps of the stand-alone CAM dumpers (csrc/preprocess.hip).

`bicubic_resize_u8` is Pillow's 8-bit `Image.resize((w, h), BICUBIC)` (Resample.c: precompute_coeffs,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc, ImagingResampleVertical_8bpc), written out so that the kernel
can be debugged without a GPU and without Pillow; tests/test_camgen_cpu.py pins it to Pillow bit for bit.
`clip_normalize` is torchvision's ToTensor + Normalize in fp32.  `scale_cam_resize_f16` is scale_cam_image
(pytorch_grad_cam/utils/image.py:51-61) with the bilinear rule of OpenCV's INTER_LINEAR on a float image, then float16.
"""
import math

import numpy as np

PREC = 22
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def target_size(H0, W0, scale=1.0, patch=16):
    """(h, w) of img_ms_and_flip (generate_cams_voc12.py:87)."""
    return int(np.ceil(scale * int(H0) / patch) * patch), int(np.ceil(scale * int(W0) / patch) * patch)


def _bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """[(first tap, int weights)] per output coordinate: precompute_coeffs + normalize_coeffs_8bpc."""
    scale = float(np.float32(in_size)) / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    ss = 1.0 / fscale
    out = []
    for o in range(out_size):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        # C's (int) truncates towards zero: round half away from zero
        out.append((xmin, [int(-0.5 + v * (1 << PREC)) if v < 0 else int(0.5 + v * (1 << PREC)) for v in k]))
    return out


def _pass(img, out_size, axis):
    """One separable pass along `axis` of an (H, W, C) uint8 array."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    dst = np.empty((out_size,) + src.shape[1:], np.uint8)
    for o, (xmin, k) in enumerate(coeffs(src.shape[0], out_size)):
        acc = np.full(src.shape[1:], 1 << (PREC - 1), np.int64)
        for i, w in enumerate(k):
            acc += w * src[xmin + i]
        dst[o] = np.clip(acc >> PREC, 0, 255)
    return np.moveaxis(dst, 0, axis)


def bicubic_resize_u8(img, h, w):
    """(H0, W0, 3) uint8 -> (h, w, 3) uint8; horizontal pass first, uint8 between the passes."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.shape[1] != w:
        img = _pass(img, w, 1)
    if img.shape[0] != h:
        img = _pass(img, h, 0)
    return img


def clip_normalize(u8, mean=CLIP_MEAN, std=CLIP_STD):
    """(h, w, 3) uint8 -> (3, h, w) f32: x / 255, - mean, / std, each rounded to fp32."""
    x = u8.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    x = x - np.asarray(mean, np.float32)[:, None, None]
    return (x / np.asarray(std, np.float32)[:, None, None]).astype(np.float32)


def bilinear_resize_f32(img, oh, ow):
    gh, gw = img.shape
    img = img.astype(np.float32)
    sy, sx = np.float32(gh) / np.float32(oh), np.float32(gw) / np.float32(ow)
    fy = np.maximum(sy * (np.arange(oh, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    fx = np.maximum(sx * (np.arange(ow, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    y0 = np.minimum(fy.astype(np.int64), gh - 1)
    x0 = np.minimum(fx.astype(np.int64), gw - 1)
    y1, x1 = np.minimum(y0 + 1, gh - 1), np.minimum(x0 + 1, gw - 1)
    ly, lx = (fy - y0.astype(np.float32))[:, None], (fx - x0.astype(np.float32))[None, :]
    hy, hx = np.float32(1) - ly, np.float32(1) - lx
    a, b = img[y0][:, x0], img[y0][:, x1]
    c, d = img[y1][:, x0], img[y1][:, x1]
    return (hy * (hx * a + lx * b) + ly * (hx * c + lx * d)).astype(np.float32)


def scale_cam_resize_f16(cam, oh, ow):
    """(gh, gw) f32 refined CAM -> (oh, ow) float16."""
    cam = cam.astype(np.float32)
    cam = cam - cam.min()
    cam = cam / (np.float32(1e-7) + cam.max())
    return bilinear_resize_f32(cam, oh, ow).astype(np.float16)


def split_dataset(dataset, n_splits):
    """The share of every worker as the dumpers cut it (generate_cams_voc12.py:39-48): equal parts, remainder to the last."""
    if n_splits == 1:
        return [dataset]
    part = len(dataset) // n_splits
    return [dataset[i * part:(i + 1) * part] for i in range(n_splits - 1)] + [dataset[(n_splits - 1) * part:]]


def f16_ulp_distance(a, b):
    """Distance in units of the last place between two float16 arrays (finite values)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float16).view(np.int16).astype(np.int32)
        return np.where(i < 0, -(i & 0x7FFF), i)
    return np.abs(key(a) - key(b))


assert math.isclose(_bicubic(0.0), 1.0)
