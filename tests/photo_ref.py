"""numpy restatement of OpenCV's 8-bit `COLOR_BGR2HSV` / `COLOR_HSV2BGR` (what `mmcv.bgr2hsv` / `mmcv.hsv2bgr` call for
uint8 images): H in [0, 180), S and V in [0, 255].

Restated from the public OpenCV sources, modules/imgproc/src/color_hsv.simd.hpp (4.x; color.cpp in 2.x / 3.x):

  * `RGB2HSV_b` (forward, integer): v = max, diff = max - min, two division tables built once with
    `saturate_cast<int>` (= cvRound, round half to even) of `(255 << 12) / (1. * i)` and `(180 << 12) / (6. * i)`,
    s = (diff * sdiv[v] + 2048) >> 12, the sector expression for h, h = (h * hdiv[diff] + 2048) >> 12 with an arithmetic
    shift, h += 180 when negative;
  * `HSV2RGB_b` -> `HSV2RGB_native` (inverse, float32): s and v scaled by 1.f / 255.f, h * (6.f / 180), fmod 6, the sector
    table {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}} over tab = {v, v(1-s), v(1-s h), v(1-s(1-h))}, then
    `saturate_cast<uchar>(x * 255.f)` (cvRound + clamp).

Neither OpenCV nor mmcv can be imported where this project is built, so this file is UNVERIFIED AGAINST REAL OPENCV; it pins
the device kernels (csrc/augment_seg.hip, bit for bit on all 2^24 colours) and stands in for `mmcv.bgr2hsv` / `hsv2bgr` when
tests/golden/make_segaug_golden.py runs the reference's PhotoMetricDistortion.
"""
import numpy as np

HSV_SHIFT = 12


def _tables():
    i = np.arange(1, 256, dtype=np.float64)
    sdiv = np.zeros(256, np.int64)
    hdiv = np.zeros(256, np.int64)
    sdiv[1:] = np.rint((255 << HSV_SHIFT) / (1.0 * i)).astype(np.int64)
    hdiv[1:] = np.rint((180 << HSV_SHIFT) / (6.0 * i)).astype(np.int64)
    return sdiv, hdiv


SDIV, HDIV180 = _tables()


def bgr2hsv(img):
    """uint8 (..., 3) BGR -> uint8 (..., 3) HSV."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    v = np.maximum(b, np.maximum(g, r))
    diff = v - np.minimum(b, np.minimum(g, r))
    s = (diff * SDIV[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV180[diff] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT          # numpy's >> on int64 is arithmetic
    h = h + np.where(h < 0, 180, 0)
    return np.stack([np.clip(h, 0, 255), s & 255, v], axis=-1).astype(np.uint8)


def hsv2bgr(img):
    """uint8 (..., 3) HSV -> uint8 (..., 3) BGR."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    f32 = np.float32
    h = img[..., 0].astype(f32)
    s = img[..., 1].astype(f32) * f32(1.0 / 255.0)
    v = img[..., 2].astype(f32) * f32(1.0 / 255.0)
    h = np.fmod(h * (f32(6.0) / f32(180.0)), f32(6.0))
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, f32(0), h).astype(f32)
    one = f32(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    assert tab.dtype == np.float32
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]], np.int64)
    bgr = np.take_along_axis(tab, sd[sector], axis=-1)
    bgr = np.where((s == 0)[..., None], v[..., None], bgr).astype(f32)
    return np.clip(np.rint(bgr * f32(255.0)), 0, 255).astype(np.uint8)


def all_colours():
    """(2^24, 3) uint8: every triple, channel 0 slowest."""
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], axis=-1).astype(np.uint8)
