"""Test-side helpers for the label-aware input pipeline (data.DeviceSegAugment): a replaying random source that feeds a
fixture's recorded draws through the class's own host code, and a numpy restatement of the whole chain
(datasets/voc.py:216-251 over datasets/transforms.py) that is itself pinned to tests/golden/seg_augment_ref.npz on the CPU
(tests/test_seg_augment_cpu.py) before the GPU tests use it at sizes the fixture does not hold."""
import numpy as np

import photo_ref

MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


class Replay:
    """Stands in for `random.Random` / `np.random.RandomState`: hands out recorded (name, value) pairs in order and checks
    the method asked for; once the record is exhausted (the reference stopped drawing candidates), filler candidates:
    `filler` = "min" / "max" gives the first / last valid origin of the randrange asked for."""

    def __init__(self, names, vals, filler="min"):
        self.names, self.vals, self.i, self.filler, self.filled = list(names), list(vals), 0, filler, 0

    def _next(self, name):
        if self.i >= len(self.names):
            assert name == "randrange", name
            self.filled += 1
            return self.filler
        assert self.names[self.i] == name, (self.i, self.names[self.i], name)
        v = self.vals[self.i]
        self.i += 1
        return v

    def uniform(self, *a):
        return float(self._next("uniform"))

    def random(self):
        return float(self._next("random"))

    def randrange(self, start, stop, step=1):
        v = self._next("randrange")
        return int({"min": start, "max": stop - 1}.get(v, v)) if isinstance(v, str) else int(v)

    def randint(self, *a):
        return int(self._next("randint"))


def replay_draw(aug, names, vals, H, W, filler="min"):
    """One draw_one() of `aug` fed from a recorded draw stream (both generators share the one recorded sequence)."""
    r = Replay(names, vals, filler)
    aug.py_rng = aug.np_rng = r
    d = aug.draw_one(H, W)
    assert r.i == len(r.names), "draws left over"
    return d, r.filled


def convert(x, alpha=1, beta=0):
    """PhotoMetricDistortion.convert (transforms.py:191-195) with float32 amounts."""
    return np.clip(x.astype(np.float32) * np.float32(alpha) + np.float32(beta), 0, 255).astype(np.uint8)


def photometric(img, photo, beta, alpha_c, alpha_s, hue):
    """transforms.py:235-264 on a uint8 (H,W,3) image with the gates / amounts of a DeviceSegAugment record."""
    if photo & 1:
        img = convert(img, beta=beta)
    if photo & 2 and photo & 16:
        img = convert(img, alpha=alpha_c)
    if photo & 4:
        hsv = photo_ref.bgr2hsv(img)
        hsv[..., 1] = convert(hsv[..., 1], alpha=alpha_s)
        img = photo_ref.hsv2bgr(hsv)
    if photo & 8:
        hsv = photo_ref.bgr2hsv(img)
        hsv[..., 0] = (hsv[..., 0].astype(int) + hue) % 180
        img = photo_ref.hsv2bgr(hsv)
    if photo & 2 and not photo & 16:
        img = convert(img, alpha=alpha_c)
    return img


def accept(window, ignore=255):
    idx, cnt = np.unique(window, return_counts=True)
    cnt = cnt[idx != ignore]
    return len(cnt) > 0 and np.max(cnt) / np.sum(cnt) < 0.75


def chain(img, lab, draw, crop, ignore=255, mean=MEAN, std=STD):
    """img uint8 (H,W,3), lab uint8 (H,W), draw: a draw_one() tuple -> (image f32 (3,crop,crop), label int64 (crop,crop),
    img_box (4,), chosen candidate index, accepted)."""
    s, flip, rh, rw, pad_y, pad_x, photo, beta, alpha_c, alpha_s, hue, cands = draw
    if (rh, rw) != lab.shape:
        from PIL import Image
        img = np.asarray(Image.fromarray(img).resize((rw, rh), resample=Image.BILINEAR))
        lab = np.asarray(Image.fromarray(lab).resize((rw, rh), resample=Image.NEAREST))
    if flip:
        img, lab = np.fliplr(img), np.fliplr(lab)
    img = photometric(np.ascontiguousarray(img), photo, beta, alpha_c, alpha_s, hue)
    Hc, Wc = max(crop, rh), max(crop, rw)
    pi = np.zeros((Hc, Wc, 3), np.float32)
    pl = np.full((Hc, Wc), ignore, np.int64)
    pi[pad_y:pad_y + rh, pad_x:pad_x + rw] = img
    pl[pad_y:pad_y + rh, pad_x:pad_x + rw] = lab
    chosen, ok = len(cands) - 1, False
    for c, (y, x) in enumerate(cands):
        if accept(pl[y:y + crop, x:x + crop], ignore):
            chosen, ok = c, True
            break
    y, x = cands[chosen]
    out = pi[y:y + crop, x:x + crop]
    out = (out - np.array(mean, np.float32)) / np.array(std, np.float32)          # normalize_img: float32 arithmetic
    box = np.array([max(pad_y - y, 0), min(y + crop, pad_y + rh), max(pad_x - x, 0), min(x + crop, pad_x + rw)], np.int64)
    return np.transpose(out, (2, 0, 1)), pl[y:y + crop, x:x + crop], box, chosen, ok
