"""numpy restatement of the CAM-seed semantics, written the slow way: image by image, threshold by threshold, the
confusion matrix by np.bincount -- not the one-increment bin trick of the kernel.  Pinned to the unmodified reference's
`cam_to_label`, `_fast_hist` and `pseudo_scores` by tests/golden/camseed_ref.npz (tests/test_camseed_cpu.py)."""
import numpy as np


def pixel_max(cam, keys):
    """cam (K, H, W) float16, keys (K,) -> (v (H, W) float32, c (H, W) int64 = 1 + the class id attaining v, the smallest class id
    on a tie)."""
    cam = np.asarray(cam).astype(np.float32)
    keys = np.asarray(keys, np.int64)
    order = np.argsort(keys, kind="stable")               # ascending class id: np.argmax then takes the smallest on a tie
    c = keys[order][np.argmax(cam[order], axis=0)] + 1
    return cam.max(axis=0), c


def fast_hist(gt, pred, nc):
    gt, pred = np.asarray(gt).reshape(-1).astype(np.int64), np.asarray(pred).reshape(-1).astype(np.int64)
    keep = gt < nc
    return np.bincount(nc * gt[keep] + pred[keep], minlength=nc * nc).reshape(nc, nc)


def threshold_label(v, c, t):
    """The prediction at background threshold t: c where v > t (in float32), 0 otherwise."""
    return np.where(v > np.float32(t), c, 0)


def sweep_confusion(cams, keys, gt, thresholds, nc):
    """conf (T, nc, nc) int64: for every threshold, the confusion matrix of every image, summed."""
    conf = np.zeros((len(thresholds), nc, nc), np.int64)
    for cam, ks, g in zip(cams, keys, gt):
        v, c = pixel_max(cam, ks)
        for j, t in enumerate(thresholds):
            conf[j] += fast_hist(g, threshold_label(v, c, t), nc)
    return conf


def sweep_bins(cams, keys, gt, thresholds, nc):
    """bins (nc, nc, T+1): the pixel counts over (gt, c, j*), j* = the number of thresholds below v."""
    T = len(thresholds)
    thr = np.asarray(thresholds, np.float32)
    bins = np.zeros((nc, nc, T + 1), np.int64)
    for cam, ks, g in zip(cams, keys, gt):
        v, c = pixel_max(cam, ks)
        js = (thr[:, None, None] < v[None]).sum(0)
        keep = g < nc
        np.add.at(bins, (g[keep].astype(np.int64), c[keep], js[keep]), 1)
    return bins


def ignore_mid_label(cam, keys, low, high):
    """cam_to_label(..., ignore_mid=True) with a full-image box: c where v > high, 255 where low < v <= high, 0 where v <= low."""
    v, c = pixel_max(cam, keys)
    lab = c.copy()
    lab[v <= np.float32(high)] = 255
    lab[v <= np.float32(low)] = 0
    return lab.astype(np.uint8)


def slot_maps(cam, keys, low, high):
    """(lab_low, lab_high) int64: slot = 1 + rank of the winning class among the image's ids ascending where v > thre, else 0."""
    v, c = pixel_max(cam, keys)
    rank = np.searchsorted(np.sort(np.asarray(keys, np.int64)), c - 1) + 1
    return np.where(v > np.float32(low), rank, 0), np.where(v > np.float32(high), rank, 0)


def merge(lab_low, lab_high, keys):
    """utils/camutils.py:77-79: the class value of slot high, then 255 where high == 0, then 0 where high == 0 and low == 0."""
    table = np.concatenate([[0], np.sort(np.asarray(keys, np.int64)) + 1])
    lab = table[lab_high]
    lab[lab_high == 0] = 255
    lab[(lab_high == 0) & (lab_low == 0)] = 0
    return lab.astype(np.uint8)


def mask_hist(gts, labels, nc):
    """pseudo_scores' histogram (utils/evaluate.py:41-45): a pixel labelled 255 is dropped.  -> hist (nc, nc) int64."""
    hist = np.zeros((nc, nc), np.int64)
    for g, lab in zip(gts, labels):
        g, lab = np.asarray(g).reshape(-1).astype(np.int64), np.asarray(lab).reshape(-1).astype(np.int64)
        hist += fast_hist(np.where(lab == 255, 255, g), np.where(lab == 255, 0, lab), nc)
    return hist


def coverage(gts, labels, nc):
    """[labelled pixels with gt < nc, pixels with gt < nc]"""
    lab = np.concatenate([np.asarray(a).reshape(-1) for a in labels])
    g = np.concatenate([np.asarray(a).reshape(-1) for a in gts])
    return np.array([int(((lab != 255) & (g < nc)).sum()), int((g < nc).sum())], np.int64)
