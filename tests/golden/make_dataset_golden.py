"""Fixture of the dataset path with images of different sizes: tests/golden/dataset_ragged_ref.npz.

Runs the UNMODIFIED reference's `datasets.transforms` on six small synthetic images of six different sizes, in the order of

    VOC12ClsDataset.__transforms (datasets/voc.py:109-144):  random_scaling -> random_fliplr -> random_crop -> normalize_img -> CHW
    VOC12SegDataset.__transforms (datasets/voc.py:216-251):  random_fliplr(image, label) -> PhotoMetricDistortion
                                                             -> random_crop(image, label) -> normalize_img -> CHW

(`datasets.voc` itself needs packages absent at import time, so the calls are made here, as make_golden.py and
make_segaug_golden.py do), with the reference's random sources replaced by seeded recording proxies of the same generators.
The file holds the sources, every draw, the float32 outputs, the labels, the `img_box` values, and, for the aug=False path,
`normalize_img` of two of the uint8 images themselves (numpy evaluates that one in double precision and rounds once).

The set: one image smaller than the crop at every scale of [0.5, 2.0], one portrait, one of odd width, one of odd height, and
scales on both sides of 1 (asserted below).

Saturation and hue of the Seg chain go through `mmcv.bgr2hsv` / `mmcv.hsv2bgr`, which are tests/photo_ref.py here: a
restatement of OpenCV's 8-bit conversions that is UNVERIFIED AGAINST REAL OPENCV.  Only those two steps see it.

    python tests/golden/make_dataset_golden.py          (needs the reference tree; regenerates the file bit-identically)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from oracle import refharness, synth  # noqa: E402
import photo_ref  # noqa: E402
from make_segaug_golden import save_npz  # noqa: E402

SEED, CROP = 64, 96
SIZES = [(40, 44), (150, 100), (120, 131), (96, 128), (181, 190), (64, 160)]     # (H, W): small, portrait, odd W, =crop, odd H, wide
NORMALIZE_OF = (0, 2)                                                             # images of the aug=False records


def sources():
    """[(image uint8 (H,W,3), label uint8 (H,W))] of the six sizes."""
    out = []
    for i, (H, W) in enumerate(SIZES):
        f = synth.make_images(1, H, W, seed=810 + i)
        img = (f * 58.0 + 118.0).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()[0]
        lab = synth.make_label_maps(1, H, W, regions=3 + 2 * i, seed=31 + i).numpy()[0].copy()
        out.append((img, lab))
    out[4][1][:, :60] = 255                                                       # a stretch of ignore
    return out


def main():
    refharness.install()
    mm = sys.modules["mmcv"]
    mm.bgr2hsv, mm.hsv2bgr = photo_ref.bgr2hsv, photo_ref.hsv2bgr
    import random as pyrandom
    import datasets.transforms as T
    assert T.__file__.startswith(refharness.REF)
    draws = []

    class Rec:
        def __init__(self, rng):
            self.rng = rng

        def __getattr__(self, name):
            fn = getattr(self.rng, name)

            def call(*a, **k):
                v = fn(*a, **k)
                draws[-1].append((name, float(v)))
                return v
            return call

    py, nprs = Rec(pyrandom.Random(SEED)), Rec(np.random.RandomState(SEED))
    orig = T.random, np.random.randint
    T.random, np.random.randint = py, nprs.randint
    cases = sources()
    out = {"n_cases": np.int64(len(cases)), "crop": np.int64(CROP), "seed": np.int64(SEED), "sizes": np.array(SIZES, np.int64)}
    try:
        cls_draws = []
        for i, (image, label) in enumerate(cases):                                # the Cls chain
            out[f"image_{i}"], out[f"label_{i}"] = image.copy(), label.copy()
            draws.append([])
            x = np.array(image)
            x = T.random_scaling(x, scale_range=[0.5, 2.0])
            x = T.random_fliplr(x)
            x, img_box = T.random_crop(x, crop_size=CROP, mean_rgb=[0, 0, 0], ignore_index=255)
            x = T.normalize_img(x)
            assert [n for n, _ in draws[-1]] == ["uniform", "random", "randint", "randint", "randrange", "randrange"]
            cls_draws.append([v for _, v in draws[-1]])
            out[f"cls_out_{i}"] = np.transpose(x, (2, 0, 1)).astype(np.float32)
            assert img_box.dtype == np.int16
            out[f"cls_img_box_{i}"] = img_box
        out["cls_draws"] = np.array(cls_draws, np.float64)       # (6, 6): scale, p_flip, pad_y, pad_x, crop_y, crop_x
        for i, (image, label) in enumerate(cases):                                # the Seg chain
            draws.append([])
            x, y = T.random_fliplr(np.array(image), label)
            x = T.PhotoMetricDistortion()(x)
            assert x.dtype == np.uint8
            x, y, img_box = T.random_crop(x, y, crop_size=CROP, ignore_index=255)
            x = T.normalize_img(x)
            names, vals = [n for n, _ in draws[-1]], [v for _, v in draws[-1]]
            k = names.index("randrange")
            assert all(n == "randrange" for n in names[k:]) and (len(names) - k) % 2 == 0
            out[f"seg_draw_names_{i}"], out[f"seg_draw_vals_{i}"] = np.array(names), np.array(vals, np.float64)
            out[f"seg_cand_{i}"] = np.array(vals[k:], np.int64).reshape(-1, 2)
            out[f"seg_out_{i}"] = np.transpose(x, (2, 0, 1)).astype(np.float32)
            out[f"seg_out_label_{i}"] = y.astype(np.int64)
            out[f"seg_img_box_{i}"] = img_box
    finally:
        T.random, np.random.randint = orig
    for i in NORMALIZE_OF:                                                        # aug=False: voc.py:137-143 on the uint8 image
        out[f"norm_{i}"] = np.transpose(T.normalize_img(cases[i][0]), (2, 0, 1))
        assert out[f"norm_{i}"].dtype == np.float32
    out["normalize_of"] = np.array(NORMALIZE_OF, np.int64)
    s = out["cls_draws"][:, 0]
    print("scales", np.round(s, 3), "flips", (out["cls_draws"][:, 1] > 0.5).astype(int))
    assert (s < 0.9).sum() >= 2 and (s > 1.1).sum() >= 2, s
    assert max(int(2.0 * v) for v in SIZES[0]) < CROP, "image 0 is smaller than the crop at every scale"
    assert SIZES[1][0] > SIZES[1][1] and SIZES[2][1] % 2 == 1 and len(set(SIZES)) == 6
    assert {bool(v > 0.5) for v in out["cls_draws"][:, 1]} == {True, False}
    print("seg tries", [len(out[f"seg_cand_{i}"]) for i in range(len(cases))])
    path = os.path.join(HERE, "dataset_ragged_ref.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
