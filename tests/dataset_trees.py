"""Test-side helpers of the dataset tests: tiny VOC- and COCO-shaped trees written with Pillow, and the recorded draws of
tests/golden/dataset_ragged_ref.npz in the form `DeviceAugment` / `DeviceSegAugment` take.

The VOC tree holds the fixture's six images.  JPEG is lossy, so to let a test compare a decoded file with the fixture's
arrays exactly, those six are stored LOSSLESSLY (PNG payload) under their `.jpg` names -- Pillow picks the decoder from the
content -- next to one real JPEG.  The COCO tree holds real JPEGs, one of them grey."""
import os

import numpy as np
from PIL import Image

import segaug_ref


def fixture_cases(g):
    return [(g[f"image_{i}"], g[f"label_{i}"]) for i in range(int(g["n_cases"]))]


def onehot20(label):
    present = [c for c in np.unique(label) if c not in (0, 255) and c <= 20]
    v = np.zeros(20, np.float32)
    v[[c - 1 for c in present] or [0]] = 1
    return v


def smooth_image(H, W, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([127 + 100 * np.sin(xx / (5.0 + c) + seed) * np.cos(yy / (7.0 + c)) for c in range(3)], -1)
    return np.clip(img + rs.randint(-8, 9, img.shape), 0, 255).astype(np.uint8)


def write_voc_tree(root, g):
    """-> (root_dir, name_list_dir, names).  train.txt: the six fixture images (lossless) + one real JPEG; val.txt: two."""
    cases = fixture_cases(g)
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "SegmentationClassAug"))
    lists = os.path.join(root, "lists")
    os.makedirs(lists)
    names, onehot = [], {}
    for i, (img, lab) in enumerate(cases):
        name = f"2007_{i:06d}"
        Image.fromarray(img).save(os.path.join(root, "JPEGImages", name + ".jpg"), format="PNG")
        pil = Image.fromarray(lab)
        if i == 1:                                         # a palette PNG: the indices must come back, not the colours
            pil = pil.convert("P")
            pil.putpalette([(7 * k) % 256 for k in range(768)])
            pil.putdata(lab.reshape(-1).tolist())
        pil.save(os.path.join(root, "SegmentationClassAug", name + ".png"))
        names.append(name)
        onehot[name] = onehot20(lab)
    name = "2008_000001"
    img = smooth_image(75, 111, 3)
    Image.fromarray(img).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=90)
    lab = np.zeros((75, 111), np.uint8)
    lab[10:50, 20:90] = 5
    lab[40:70, 5:40] = 12
    Image.fromarray(lab).save(os.path.join(root, "SegmentationClassAug", name + ".png"))
    names.append(name)
    onehot[name] = onehot20(lab)
    with open(os.path.join(lists, "train.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    with open(os.path.join(lists, "val.txt"), "w") as f:
        f.write("\n".join(names[:3]) + "\n")
    np.save(os.path.join(lists, "cls_labels_onehot.npy"), onehot)
    return root, lists, names


def write_coco_tree(root):
    """-> (root_dir, name_list_dir, full names).  Four train JPEGs of different sizes, the third one grey (mode L)."""
    lists = os.path.join(root, "lists")
    os.makedirs(lists)
    for sub in ("train", "val"):
        os.makedirs(os.path.join(root, "JPEGImages", sub))
        os.makedirs(os.path.join(root, "SegmentationClass", sub))
    onehot = {}
    out = {}
    for sub, prefix, sizes in (("train", "COCO_train2014_", [(60, 80), (90, 70), (64, 64), (55, 101)]),
                               ("val", "COCO_val2014_", [(48, 72), (70, 50)])):
        names = []
        for i, (H, W) in enumerate(sizes):
            short = f"{i + 9:012d}"
            full = prefix + short
            img = smooth_image(H, W, 10 + i)
            pil = Image.fromarray(img[:, :, 0], mode="L") if (sub, i) == ("train", 2) else Image.fromarray(img)
            pil.save(os.path.join(root, "JPEGImages", sub, full + ".jpg"), quality=92)
            lab = np.zeros((H, W), np.uint8)
            lab[H // 4:H // 2, W // 4:] = 3 + i
            lab[H // 2:, :W // 2] = 60 + i
            lab[:2] = 255
            Image.fromarray(lab).save(os.path.join(root, "SegmentationClass", sub, short + ".png"))
            v = np.zeros(80, np.float32)
            v[[2 + i, 59 + i]] = 1
            onehot[full] = v
            names.append(full)
        with open(os.path.join(lists, sub + ".txt"), "w") as f:
            f.write("\n".join(names) + "\n")
        out[sub] = names
    np.save(os.path.join(lists, "cls_labels_onehot.npy"), onehot)
    return root, lists, out


def cls_draw(vals, H, W):
    """One recorded Cls draw (scale, p_flip, pad_y, pad_x, crop_y, crop_x) -> a DeviceAugment.draw_one() tuple."""
    s = float(vals[0])
    return (s, int(vals[1] > 0.5), int(s * H), int(s * W), int(vals[2]), int(vals[3]), int(vals[4]), int(vals[5]))


def seg_draw(aug, g, i, filler="min"):
    """The recorded Seg draws of case i through DeviceSegAugment's own host code (filler candidates past the recorded ones)."""
    lab = g[f"label_{i}"]
    return segaug_ref.replay_draw(aug, [str(n) for n in g[f"seg_draw_names_{i}"]], g[f"seg_draw_vals_{i}"], *lab.shape,
                                  filler=filler)[0]
