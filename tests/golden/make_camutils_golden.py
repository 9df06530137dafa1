"""Generate tests/golden/camutils_ref.npz by RUNNING THE UNMODIFIED REFERENCE's utils/camutils.py and WeCLIP_model/PAR.py on the CPU.

Build-container only (needs the reference checkout; oracle/refharness.py imports it without its missing packages).
    python tests/golden/make_camutils_golden.py
The inputs are the functions of tests/camutils_cases.py (rebuilt bit for bit by the tests; their checksums are recorded here).
Recorded, as data only: the reference's outputs -- labels as uint8, maps as f32 -- and, for the two refine_* functions, what a
small recording wrapper around the reference's PAR saw leave it: the refined soft-max stacks, from which the top-2 margin after
the reference's own up-sample is taken.  A pixel is `sure` for a tolerance t when that margin exceeds 2 t; the masks for the two
PAR tolerances (3e-5 exact, 5e-4 fast) are stored, and at most 2 % of a case's pixels may be unsure (asserted here)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import camutils_cases as K  # noqa: E402
import camutils_ref as R  # noqa: E402

TOLS = {"exact": 3e-5, "fast": 5e-4}          # tests/test_par_gpu.py
CAP = 0.02


class Recorder(torch.nn.Module):
    def __init__(self, mod):
        super().__init__()
        self.mod, self.outs = mod, []

    def forward(self, imgs, masks):
        out = self.mod(imgs, masks)
        self.outs.append(out.detach().clone())
        return out


def in_box(box, H, W):
    m = torch.zeros(len(box), H, W, dtype=torch.bool)
    for b, r in enumerate(box):
        m[b, r[0]:r[1], r[2]:r[3]] = True
    return m


def sure_masks(margin, inside, what):
    """{mode: packed bits of (margin > 2 tol or outside the box)}; the cap is asserted for every mode."""
    out = {}
    for mode, t in TOLS.items():
        sure = (margin > 2 * t) | ~inside
        frac = 1.0 - sure.float().mean().item()
        print(f"  {what}: {frac:.3%} of the pixels within {2 * t:.0e} of a tie ({mode})")
        assert frac <= CAP, f"{what}: {frac:.3%} of the pixels are near-ties: change the seed or the scale, never the cap"
        out[mode] = np.packbits(sure.numpy())
    return out


def bkg_stack_and_margin(outs, H, W):
    """The recorder's 2 B outputs (image 0 high, image 0 low, image 1 high, ...) as the compact (B, 2 Kmax, h2, w2) stack, and the
    per-pixel smaller top-2 margin of the two after the reference's own up-sample."""
    B = len(outs) // 2
    Kmax = max(o.shape[1] for o in outs)
    stack = torch.zeros(B, 2 * Kmax, *outs[0].shape[2:])
    margin = torch.zeros(B, H, W)
    for b in range(B):
        for half in range(2):
            o = outs[2 * b + half]
            stack[b, half * Kmax:half * Kmax + o.shape[1]] = o[0]
        up = [F.interpolate(outs[2 * b + half], size=(H, W), mode="bilinear", align_corners=False)[0] for half in range(2)]
        margin[b] = torch.minimum(R.top2_margin(up[0]), R.top2_margin(up[1]))
    return stack, margin


def main():
    from oracle import refharness
    refharness.install()
    import utils.camutils as RC
    from WeCLIP_model.PAR import PAR
    from weclip_vit_comer_amd.utils.camutils import get_mask_by_radius
    out = {"sigmoid_table": K.sigmoid_table()}
    table = out["sigmoid_table"]

    # ---- labels
    c = K.label_case()
    cfg = K.make_cfg()
    out["lab_check"] = np.array([K.check(c["cam"], c["cls"])], np.int64)
    nobox = RC.cam_to_label(c["cam"].clone(), c["cls"], cfg=cfg)
    out["lab_nobox"] = nobox.numpy().astype(np.uint8)
    for mid in (0, 1):
        valid, lab = RC.cam_to_label(c["cam"].clone(), c["cls"], img_box=c["box"], ignore_mid=bool(mid), cfg=cfg)
        out[f"lab_mid{mid}"] = lab.numpy().astype(np.uint8)
        out[f"lab_valid_check{mid}"] = np.array([K.check(valid)], np.int64)
    out["lab_ign_i64"] = RC.ignore_img_box(nobox, c["box"], 255).numpy().astype(np.uint8)
    out["lab_ign_f32"] = RC.ignore_img_box(nobox.float() + 0.25, c["box"], 255).numpy()

    # ---- random walk
    for gi, (h, w) in enumerate(K.WALK_GRIDS):
        n = h * w
        for C in K.WALK_C:
            c = K.walk_case(h, w, C, table)
            out[f"walk_check_{n}_{C}"] = np.array([K.check(c["aff"], c["cams"], c["cls"])], np.int64)
            for masked in (0, 1):
                mask = get_mask_by_radius(h, w, radius=8) if masked else None
                o = RC.propagte_aff_cam_with_bkg(c["cams"].clone(), aff=c["aff"].clone(), mask=mask, cls_labels=c["cls"], bkg_score=K.THRE[0])
                out[f"walk_bkg_{n}_{C}_{masked}"] = o.reshape(3, C + 1, n).numpy()
                # (at n = 400 every 7th column only: all columns of all twelve combinations would be 1 MB of f32 noise on their
                #  own; every 32-column block of the kernel still has four or five recorded columns)
                o = RC.propagte_aff_cam(c["cams"].clone(), aff=c["aff"].clone(), mask=mask)
                out[f"walk_plain_{n}_{C}_{masked}"] = o.reshape(3, C, n)[..., ::K.WALK_STRIDE[n]].numpy()

    # ---- the two refine_* functions
    for i, (B, C, H, W) in enumerate(K.REFINE_SHAPES):
        print(f"refine case {i} {(B, C, H, W)}")
        c = K.refine_case(i)
        out[f"ref{i}_check"] = np.array([K.check(c["images"], c["cams"], c["cls"])], np.int64)
        rec = Recorder(PAR(num_iter=K.NUM_ITER, dilations=K.DILATIONS))
        lab = RC.refine_cams_with_bkg_v2(rec, c["images"], cams=c["cams"], cls_labels=c["cls"], cfg=c["cfg"], img_box=c["box_bkg"])
        stack, margin = bkg_stack_and_margin(rec.outs, H, W)
        out[f"ref{i}_bkg_label"] = lab.numpy().astype(np.uint8)
        out[f"ref{i}_bkg_stack"] = stack.numpy()
        for mode, bits in sure_masks(margin, in_box(c["box_bkg"], H, W), "refine_cams_with_bkg_v2").items():
            out[f"ref{i}_bkg_sure_{mode}"] = bits
        o = RC.refine_cams_with_cls_label(PAR(num_iter=K.NUM_ITER, dilations=K.DILATIONS), c["images"], labels=c["cls"], cams=c["cams"],
                                          img_box=c["box_cls"])
        out[f"ref{i}_cls_out"] = o.numpy()

    # ---- multi-scale CAMs
    x = K.msc_inputs()
    out["msc_check"] = np.array([K.check(x)], np.int64)
    out["msc_cam"] = RC.multi_scale_cam(K.msc_model, x, K.MSC_SCALES).numpy()
    cam, aff = RC.multi_scale_cam_with_aff_mat(K.msc_model, x, K.MSC_SCALES)
    assert torch.equal(cam, torch.from_numpy(out["msc_cam"]))
    out["msc_aff"] = aff.numpy()

    # ---- the lineage's training step, scripts/.ipynb_checkpoints/dist_train_voc-checkpoint.py:310-339
    print("chain")
    c = K.chain_case(table)
    cfg, box, cls, (H, W) = c["cfg"], c["box"], c["cls"], c["cams"].shape[2:]
    par = PAR(num_iter=K.NUM_ITER, dilations=K.DILATIONS)
    mask = get_mask_by_radius(*K.CHAIN_GRID, radius=K.CHAIN_RADIUS)
    out["chain_check"] = np.array([K.check(c["images"], c["cams"], cls, c["aff"])], np.int64)
    valid_cam, pseudo_label = RC.cam_to_label(c["cams"].clone(), cls_label=cls, img_box=box, ignore_mid=True, cfg=cfg)
    resized = F.interpolate(valid_cam, size=K.CHAIN_GRID, mode="bilinear", align_corners=False)
    refined, labels = {}, {}
    for name, thre in (("l", cfg.cam.low_thre), ("h", cfg.cam.high_thre)):
        a = RC.propagte_aff_cam_with_bkg(resized, aff=c["aff"].clone(), mask=mask, cls_labels=cls, bkg_score=thre)
        a = F.interpolate(a, size=(H, W), mode="bilinear", align_corners=False)
        refined[name] = RC.refine_cams_with_cls_label(par, c["images"], cams=a, labels=torch.cat([torch.ones(3, 1), cls], 1), img_box=box)
        labels[name] = refined[name].argmax(dim=1)
    lab = labels["h"].clone()
    lab[labels["h"] == 0] = cfg.dataset.ignore_index
    lab[(labels["h"] + labels["l"]) == 0] = 0
    lab = RC.ignore_img_box(lab, img_box=box, ignore_index=cfg.dataset.ignore_index)
    rec = Recorder(par)
    rpl = RC.refine_cams_with_bkg_v2(rec, c["images"], cams=c["cams"], cls_labels=cls, cfg=cfg, img_box=box)
    amask = torch.ones(4, 4)
    amask[0, 3] = amask[3, 0] = 0
    aff_label = RC.cams_to_affinity_label(rpl, mask=amask, ignore_index=cfg.dataset.ignore_index)
    inside = in_box(box, H, W)
    out["chain_pseudo_label"] = pseudo_label.numpy().astype(np.uint8)
    out["chain_aff_label_map"] = lab.numpy().astype(np.uint8)
    out["chain_refined_pseudo_label"] = rpl.numpy().astype(np.uint8)
    out["chain_affinity_label"] = aff_label.numpy().astype(np.uint8)
    out["chain_affinity_mask"] = amask.numpy()
    m1 = torch.minimum(R.top2_margin(refined["l"], dim=1), R.top2_margin(refined["h"], dim=1))
    for mode, bits in sure_masks(m1, inside, "chain, refined_aff_label").items():
        out[f"chain_aff_sure_{mode}"] = bits
    for mode, bits in sure_masks(bkg_stack_and_margin(rec.outs, H, W)[1], inside, "chain, refined_pseudo_label").items():
        out[f"chain_rpl_sure_{mode}"] = bits

    path = os.path.join(HERE, "camutils_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
