"""Fixture of the label-aware input chain of the fully supervised variant: tests/golden/seg_augment_ref.npz.

Runs the UNMODIFIED reference's `datasets.transforms` in the order of `VOC12SegDataset.__transforms` (datasets/voc.py:216-251;
that module itself needs packages absent here at import time, so the four calls are made below, as make_golden.py does for
the image-only chain):

    [random_scaling(image, label)]  ->  random_fliplr(image, label)  ->  PhotoMetricDistortion()(image)
    ->  random_crop(image, label, crop_size)  ->  normalize_img(image), HWC -> CHW

with the reference's random sources replaced by seeded recording proxies of the same generators, so the fixture holds every
draw (name and value, in call order), every candidate box tried and what `np.unique` returned for it, next to the outputs.

Two things are not the reference's:
  * `mmcv.bgr2hsv` / `mmcv.hsv2bgr` (OpenCV's 8-bit conversions) are tests/photo_ref.py, a restatement that is UNVERIFIED
    AGAINST REAL OPENCV, installed before `datasets.transforms` is imported.  Only the saturation and hue steps see it.
  * in the rescale group the float32 image that `random_scaling` returns (whole numbers: it is Pillow's uint8 result) is
    cast back to uint8 before PhotoMetricDistortion, which is written for uint8 images (its 8-bit HSV steps).

    python tests/golden/make_segaug_golden.py          (needs the reference tree; regenerates the file bit-identically)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refharness, synth  # noqa: E402
import photo_ref  # noqa: E402

SEED, CROP = 47, 64
SMALL, LARGE = (54, 76), (96, 120)          # augment_ref.npz's source size; both sides larger than the crop


def sources():
    """[(group, image uint8 (H,W,3), label uint8 (H,W))]: group 0 small, 1 large, 2 small with random_scaling first."""
    def images(n, hw, seed):
        f = synth.make_images(n, hw[0], hw[1], seed=seed)
        return (f * 58.0 + 118.0).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    cases = []
    im = images(6, SMALL, 710)
    lab = synth.make_label_maps(6, *SMALL, regions=7, seed=21).numpy().copy()
    lab[4] = synth.make_label_maps(1, *SMALL, regions=1, seed=1).numpy()[0]            # single class: all candidates rejected
    lab[5] = synth.make_label_maps(1, *SMALL, regions=2, seed=5).numpy()[0]
    cases += [(0, im[i], lab[i]) for i in range(6)]
    im = images(5, LARGE, 720)
    lab = synth.make_label_maps(5, *LARGE, regions=9, seed=22).numpy().copy()
    lab[1][:, :100] = 255                                                              # most windows see only ignore
    lab[2][:85, :] = 255
    lab[3] = synth.make_label_maps(1, *LARGE, regions=3, seed=8).numpy()[0]
    cases += [(1, im[i], lab[i]) for i in range(5)]
    im = images(4, SMALL, 730)
    lab = synth.make_label_maps(4, *SMALL, regions=7, seed=23).numpy()
    cases += [(2, im[i], lab[i]) for i in range(4)]
    return cases


def save_npz(path, arrays):
    """np.savez_compressed with fixed entry timestamps, so the same arrays give the same bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    refharness.install()
    mm = sys.modules["mmcv"]
    mm.bgr2hsv, mm.hsv2bgr = photo_ref.bgr2hsv, photo_ref.hsv2bgr
    import random as pyrandom
    import datasets.transforms as T
    assert T.__file__.startswith(refharness.REF)
    draws, uniq = [], []

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
    orig = T.random, np.random.randint, np.unique

    def rec_unique(a, *args, **k):
        r = orig[2](a, *args, **k)
        if k.get("return_counts"):
            uniq[-1].append((r[0].copy(), r[1].copy()))
        return r

    T.random, np.random.randint, np.unique = py, nprs.randint, rec_unique
    cases = sources()
    out = {}
    stats = []
    try:
        for i, (group, image, label) in enumerate(cases):
            draws.append([])
            uniq.append([])
            src_img, src_lab = image.copy(), label.copy()
            if group == 2:
                image, label = T.random_scaling(image, label, scale_range=[0.5, 2.0])
                assert np.array_equal(image, np.rint(image)) and label.dtype == np.uint8
                image = image.astype(np.uint8)
            image, label = T.random_fliplr(image, label)
            image = T.PhotoMetricDistortion()(image)
            assert image.dtype == np.uint8
            image, label, img_box = T.random_crop(image, label, crop_size=CROP, ignore_index=255)
            image = T.normalize_img(image)
            names = [n for n, _ in draws[-1]]
            vals = [v for _, v in draws[-1]]
            k = names.index("randrange")
            cand = np.array(vals[k:], np.int64).reshape(-1, 2)
            assert all(n == "randrange" for n in names[k:]) and len(cand) == len(uniq[-1]) <= 10
            out[f"image_{i}"], out[f"label_{i}"] = src_img, src_lab
            out[f"draw_names_{i}"], out[f"draw_vals_{i}"] = np.array(names), np.array(vals, np.float64)
            out[f"cand_{i}"] = cand
            out[f"out_{i}"] = np.transpose(image, (2, 0, 1)).astype(np.float32)
            out[f"out_label_{i}"] = label.astype(np.int64)
            out[f"img_box_{i}"] = img_box.astype(np.int64)
            # what the reference itself saw per try: non-ignored counts of np.unique
            cnts = [c[ix != 255] for ix, c in uniq[-1]]
            ok = [len(c) > 0 and np.max(c) / np.sum(c) < 0.75 for c in cnts]
            assert not any(ok[:-1]), "the reference stops at the first accepted candidate"
            flip = vals[names.index("random")] > 0.5
            # gates, from the draw stream in the order of PhotoMetricDistortion.__call__
            it = iter(zip(names[(2 if group == 2 else 1):], vals[(2 if group == 2 else 1):]))

            def gate():
                n, v = next(it)
                assert n == "randint"
                if v:
                    next(it)
                return int(v)
            bright = gate()
            mode = int(next(it)[1])
            contrast = gate() if mode == 1 else None
            sat, hue = gate(), gate()
            if mode == 0:
                contrast = gate()
            stats.append(dict(group=group, tries=len(cand), accepted=bool(ok[-1]), empty=any(len(c) == 0 for c in cnts), flip=flip,
                              bright=bright, mode=mode, contrast=contrast, sat=sat, hue=hue, img_box=img_box.tolist()))
    finally:
        T.random, np.random.randint, np.unique = orig
    for s in stats:
        print(s)
    # coverage, from the reference's own behaviour
    assert any(s["tries"] == 1 and s["accepted"] for s in stats), "a first-try accept"
    assert any(2 <= s["tries"] <= 9 and s["accepted"] for s in stats), "an accept after 2-9 tries"
    assert any(s["tries"] == 10 and not s["accepted"] for s in stats), "all 10 rejected"
    assert stats[4]["tries"] == 10 and not stats[4]["accepted"], "the single-class label exhausts its candidates"
    assert any(s["empty"] for s in stats), "a window that is entirely padding / ignore"
    for key in ("flip", "bright", "contrast", "sat", "hue", "mode"):
        assert {bool(s[key]) for s in stats} == {True, False}, key
    assert all(s["flip"] in (True, False) for s in stats)
    assert any(s["group"] == 0 for s in stats), "padding on one axis (54 < 64) and cropping on the other (76 > 64)"
    out["n_cases"], out["crop"], out["seed"] = np.int64(len(cases)), np.int64(CROP), np.int64(SEED)
    out["group"] = np.array([c[0] for c in cases], np.int64)
    path = os.path.join(HERE, "seg_augment_ref.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
