"""Generate tests/golden/camseed_ref.npz by RUNNING THE UNMODIFIED REFERENCE's utils/camutils.py `cam_to_label` (both branches,
full-image box) and utils/evaluate.py `_fast_hist` / `pseudo_scores` on the CPU.

Build-container only (needs the reference checkout; oracle/refharness.py imports it without its missing packages).
    python tests/golden/make_camseed_golden.py
The inputs are the functions of tests/camseed_cases.py (rebuilt bit for bit by the tests; their checksums are recorded here).
Recorded, as data only: the reference's outputs -- label maps as uint8, histograms as int64, pseudo_scores' numbers as float64.
The CRF leg has no recording (pydensecrf is not installed here): it is pinned to this package's own crf_inference_label."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import camseed_cases as K  # noqa: E402
from camutils_cases import make_cfg  # noqa: E402


def dense(case):
    """The reference's inputs: cam (B, nc - 1, H, W) float32 with the image's maps at their class channels, cls_label one-hot."""
    B, nc = len(case["cams"]), case["nc"]
    H, W = case["gt"].shape[1:]
    cam = torch.zeros(B, nc - 1, H, W)
    cls = torch.zeros(B, nc - 1)
    for b, (maps, keys) in enumerate(zip(case["cams"], case["keys"])):
        cam[b, keys] = torch.from_numpy(maps.astype(np.float32))
        cls[b, keys] = 1
    return cam, cls


def main():
    from oracle import refharness
    refharness.install()
    import utils.camutils as RC
    import utils.evaluate as RE
    out = {}
    for name in ("case1", "case2", "case3"):
        case = getattr(K, name)()
        nc, gt = case["nc"], case["gt"]
        cam, cls = dense(case)
        B, H, W = gt.shape
        out[f"{name}_check"] = np.array([K.check(case)], np.int64)
        conf, labs = [], []
        for t in case["thresholds"]:
            cfg = make_cfg()
            cfg.cam.bkg_score = t
            lab = RC.cam_to_label(cam.clone(), cls, cfg=cfg).numpy()
            labs.append(lab.astype(np.uint8))
            conf.append(sum(RE._fast_hist(gt[b].flatten(), lab[b].flatten(), nc) for b in range(B)))
        out[f"{name}_conf"] = np.stack(conf).astype(np.int64)
        if name == "case1":
            out["case1_labels"] = np.stack(labs)                              # (T, B, H, W) uint8
            cfg = make_cfg()
            cfg.cam.low_thre, cfg.cam.high_thre = K.LOW_THRE, K.HIGH_THRE
            _, mid = RC.cam_to_label(cam.clone(), cls, img_box=[[0, H, 0, W]] * B, ignore_mid=True, cfg=cfg)
            mid = mid.numpy()
            assert mid.min() >= 0 and mid.max() <= 255
            out["case1_ignore_mid"] = mid.astype(np.uint8)
            s = RE.pseudo_scores([gt[b].copy() for b in range(B)], [mid[b].copy() for b in range(B)], num_classes=nc)
            out["case1_pseudo_scores"] = np.array([s["pAcc"], s["mAcc"], s["miou"]], np.float64)
            out["case1_pseudo_iou"] = np.array([s["iou"][c] for c in range(nc)], np.float64)
            # the histogram pseudo_scores builds inside (it returns only the ratios): its own two masking lines, its _fast_hist
            hist = np.zeros((nc, nc), np.int64)
            for b in range(B):
                lt, lp = gt[b].flatten(), mid[b].flatten()
                lt[lp == 255] = 255
                lp[lp == 255] = 0
                hist += RE._fast_hist(lt, lp, nc)
            out["case1_mask_hist"] = hist
    path = os.path.join(HERE, "camseed_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
