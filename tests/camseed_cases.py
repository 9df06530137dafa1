"""Inputs of the CAM-seed tests and of tests/golden/camseed_ref.npz, rebuilt bit for bit wherever they are needed (integer hashing
and correctly rounded float64 arithmetic only: camutils_cases.noise / smooth), so the fixture stores the reference's outputs and
a checksum of every input, not the inputs.

A case is a dict: cams [(K, H, W) float16 per image], keys [[class id, ...] per image, the dumpers' first-seen order], gt
(B, H, W) uint8, nc, thresholds."""
import zlib

import numpy as np

from camutils_cases import noise, smooth

LOW_THRE, HIGH_THRE = 0.35, 0.55                      # camutils_cases.THRE[0], THRE[2]: the AFA lineage's values
SWEEP_16 = [round(0.05 + 0.05 * i, 10) for i in range(16)]          # --eval_thresholds 0.05:0.80:0.05


def _maps(K, H, W, seed):
    """(K, H, W) float16 in [0, 1]: a smooth field per class (so that every threshold of a sweep cuts through it) plus noise."""
    v = 0.85 * smooth((K,), H, W, seed, cell=6) + 0.15 * noise((K, H, W), seed + 1)
    return v.astype(np.float16)


def _gt(H, W, classes, seed):
    """Rectangles of the given class values over background."""
    g = np.zeros((H, W), np.uint8)
    r = (noise((len(classes), 4), seed) * np.array([H, H, W, W])).astype(int)
    for c, (y0, y1, x0, x1) in zip(classes, r):
        y0, y1, x0, x1 = min(y0, y1), max(y0, y1) + 3, min(x0, x1), max(x0, x1) + 3
        g[y0:y1, x0:x1] = c
    return g


def check(case):
    c = 0
    for a in case["cams"] + [case["gt"], np.asarray(case["thresholds"], np.float64)]:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    for k in case["keys"]:
        c = zlib.crc32(np.asarray(k, np.int64).tobytes(), c)
    return c


def case1():
    """Sweep on the LDS path; labels and merge.  B = 3 images of 37 x 29 (HW = 1073, odd: pairs 1, 3, 5 start at an odd
    element), K = (3, 1, 2).  Planted: a tie between classes 14 and 3 (3 must win although 14 is the first pair), values equal to
    a threshold (0.25 and 0.5 are fp16 numbers and entries 4 and 9 of the sweep), an all-zero pixel, a gt row of 255, gt values
    of 37 (>= nc: skipped like 255)."""
    H, W, nc = 37, 29, 21
    keys = [[14, 3, 7], [0], [19, 5]]
    cams = [_maps(len(k), H, W, 100 + 10 * b) for b, k in enumerate(keys)]
    gt = np.stack([_gt(H, W, [15, 4, 8, 1], 201), _gt(H, W, [1, 12], 202), _gt(H, W, [20, 6, 20], 203)])
    # ties between pair 0 (class 14) and pair 1 (class 3) above every other value, across several thresholds
    for i, (y, x) in enumerate([(0, 0), (5, 7), (36, 28), (20, 11), (9, 1)]):
        v = np.float16([0.97, 0.61, 0.33, 0.5, 0.08][i])
        cams[0][0, y, x] = cams[0][1, y, x] = v
        cams[0][2, y, x] = np.float16(0.02)
    # a maximum equal to a threshold: background AT that threshold, foreground below it
    for b, (y, x, v) in enumerate([(3, 3, 0.5), (10, 20, 0.25), (30, 2, 0.75)]):
        cams[b][:, y, x] = np.float16(0.01)
        cams[b][-1, y, x] = np.float16(v)
    cams[0][:, 12, 12] = 0                                       # all-zero pixels
    cams[1][:, 0, 28] = 0
    cams[2][:, 36, 0] = 0
    gt[0, 17, :] = 255
    gt[1, :, 5] = 255
    gt[2, 4:9, 10:14] = 37
    gt[0, 0, 0], gt[0, 5, 7], gt[0, 3, 3] = 4, 15, 8             # the planted pixels are counted
    return dict(cams=cams, keys=keys, gt=gt, nc=nc, thresholds=SWEEP_16)


def case2():
    """The smallest: one 7 x 9 image, one class, one threshold."""
    cams = [_maps(1, 7, 9, 300)]
    return dict(cams=cams, keys=[[6]], gt=_gt(7, 9, [7, 2], 301)[None], nc=21, thresholds=[0.4])


def case3():
    """The global-atomic path: nc = 81, one 16 x 20 image, K = 12, T = 64 (81 * 12 * 65 cells do not fit 64 KiB)."""
    keys = [[40, 2, 79, 11, 0, 63, 5, 17, 30, 71, 8, 55]]
    cams = [_maps(12, 16, 20, 400)]
    cams[0][3, 2, 2] = cams[0][1, 2, 2] = np.float16(0.99)      # tie: class 2 (pair 1) beats class 11 (pair 3)
    gt = _gt(16, 20, [41, 3, 80, 12, 1, 64], 401)[None]
    gt[0, 15, :] = 255
    gt[0, 0, :4] = 81
    return dict(cams=cams, keys=keys, gt=gt, nc=81, thresholds=[round((i + 1) / 65.0, 10) for i in range(64)])


def case5_image():
    """Blocks plus noise, RGB uint8 (37, 29, 3): the CRF's image for image 0 of case 1."""
    H, W = 37, 29
    blocks = np.floor(noise((5, 4, 3), 500) * 200).astype(np.int64)
    img = blocks[(np.arange(H) // 8)[:, None], (np.arange(W) // 8)[None, :]]
    return np.clip(img + np.floor(noise((H, W, 3), 501) * 40), 0, 255).astype(np.uint8)


def flat(case):
    """The kernels' layout: ((P, HW) float16, (B, HW) uint8)."""
    B = len(case["cams"])
    return np.concatenate([c.reshape(c.shape[0], -1) for c in case["cams"]]), case["gt"].reshape(B, -1)
