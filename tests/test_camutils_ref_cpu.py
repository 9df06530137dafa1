"""tests/camutils_ref.py (our restatement of the reference's utils/camutils.py, here in float64) reproduces every fixture of
tests/golden/camutils_ref.npz, which holds what the unmodified reference computed in float32: labels exactly outside the
recorded near-ties, maps to the reference's own f32 arithmetic.  The worst figures are printed."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camutils_cases as K  # noqa: E402
import camutils_ref as R  # noqa: E402

PAR_TOL = 3e-5            # tests/test_par_gpu.py, exact mode: the f32 PAR against a wider one, maps in [0, 1.22]


@pytest.fixture(scope="module")
def gold(golden):
    return golden("camutils_ref.npz")


def _d(t):
    return t.double()


def test_inputs_rebuild_bit_for_bit(gold):
    c = K.label_case()
    assert K.check(c["cam"], c["cls"]) == gold["lab_check"][0]
    # (the sigmoid table, the one input that needs exp, is taken from the fixture, never rebuilt: every checksum below is strict)
    for h, w in K.WALK_GRIDS:
        for C in K.WALK_C:
            c = K.walk_case(h, w, C, gold["sigmoid_table"])
            assert K.check(c["aff"], c["cams"], c["cls"]) == gold[f"walk_check_{h * w}_{C}"][0]
    for i in range(len(K.REFINE_SHAPES)):
        c = K.refine_case(i)
        assert K.check(c["images"], c["cams"], c["cls"]) == gold[f"ref{i}_check"][0]
    assert K.check(K.msc_inputs()) == gold["msc_check"][0]
    c = K.chain_case(gold["sigmoid_table"])
    assert K.check(c["images"], c["cams"], c["cls"], c["aff"]) == gold["chain_check"][0]


def test_labels(gold):
    c, cfg = K.label_case(), K.make_cfg()
    nobox = R.cam_to_label(_d(c["cam"]), c["cls"], cfg=cfg)
    assert nobox.dtype == torch.int64 and np.array_equal(nobox.numpy(), gold["lab_nobox"])
    for mid in (0, 1):
        valid, lab = R.cam_to_label(_d(c["cam"]), c["cls"], img_box=c["box"], ignore_mid=bool(mid), cfg=cfg)
        assert np.array_equal(lab.numpy(), gold[f"lab_mid{mid}"])
        assert K.check(valid.float()) == gold[f"lab_valid_check{mid}"][0]
    assert len(np.unique(gold["lab_mid1"])) > 4 and (gold["lab_mid1"] == 255).any() and (gold["lab_mid1"] == 0).any()
    assert np.array_equal(R.ignore_img_box(nobox, c["box"], 255).numpy(), gold["lab_ign_i64"])
    assert np.array_equal(R.ignore_img_box(nobox.float() + 0.25, c["box"], 255).numpy(), gold["lab_ign_f32"])


def walk_ratio(got, ref64, factor=1.0):
    """Worst |got - ref64| / (factor (2^-20 ref64 + 2^-24))."""
    return ((got.double() - ref64).abs() / (factor * (2.0 ** -20 * ref64.abs() + 2.0 ** -24))).max().item()


@pytest.mark.parametrize("hw", K.WALK_GRIDS)
@pytest.mark.parametrize("C", K.WALK_C)
def test_walk(gold, hw, C):
    from weclip_vit_comer_amd.utils.camutils import get_mask_by_radius
    h, w = hw
    n = h * w
    c = K.walk_case(h, w, C, gold["sigmoid_table"])
    for masked in (0, 1):
        mask = get_mask_by_radius(h, w, radius=8).double() if masked else None
        ref = R.propagte_aff_cam_with_bkg(_d(c["cams"]), aff=c["aff"], mask=mask, cls_labels=c["cls"], bkg_score=K.THRE[0]).reshape(3, C + 1, n)
        rec = torch.from_numpy(gold[f"walk_bkg_{n}_{C}_{masked}"])
        r = walk_ratio(rec, ref, 2.0)
        print(f"walk with bkg n={n} C={C} masked={masked}: recorded f32 vs fp64, worst ratio to twice the bound {r:.3f}")
        assert r <= 1.0
        assert (ref[1, :, 5] == 0).all() and (rec[1, :, 5] == 0).all()            # the zeroed column: 0 / (0 + eps)
        assert (rec[0, 1:] == 0).all() and (ref[0, 1:] == 0).all()                # no class present: only the background row
        ref = R.propagte_aff_cam(_d(c["cams"]), aff=c["aff"], mask=mask).reshape(3, C, n)[..., ::K.WALK_STRIDE[n]]
        r = walk_ratio(torch.from_numpy(gold[f"walk_plain_{n}_{C}_{masked}"]), ref, 2.0)
        print(f"walk n={n} C={C} masked={masked}: recorded f32 vs fp64, worst ratio to twice the bound {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("i", range(len(K.REFINE_SHAPES)))
def test_refine(gold, i):
    B, C, H, W = K.REFINE_SHAPES[i]
    c = K.refine_case(i)
    par = R.Par(K.DILATIONS, K.NUM_ITER)
    img, cams = _d(c["images"]), _d(c["cams"])
    maps = R.bkg_refined_maps(par, img, cams, c["cls"], c["cfg"])
    rec = torch.from_numpy(gold[f"ref{i}_bkg_stack"])
    Kmax = rec.shape[1] // 2
    worst = 0.0
    for b, (values, mh, ml) in enumerate(maps):
        for half, m in enumerate((mh, ml)):
            up = F.interpolate(rec[b:b + 1, half * Kmax:half * Kmax + len(values)], size=(H, W), mode="bilinear", align_corners=False)[0]
            worst = max(worst, (up.double() - m).abs().max().item())
    lab = R.refine_cams_with_bkg_v2(par, img, cams, c["cls"], c["cfg"], c["box_bkg"])
    sure = K.unpack(gold[f"ref{i}_bkg_sure_exact"], (B, H, W))
    recl = torch.from_numpy(gold[f"ref{i}_bkg_label"].astype(np.float64))
    out = R.refine_cams_with_cls_label(par, img, c["cls"], cams, c["box_cls"])
    reco = torch.from_numpy(gold[f"ref{i}_cls_out"])
    e_cls = (out - reco.double()).abs().max().item()
    print(f"refine case {i}: bkg_v2 maps |f32 reference - fp64| <= {worst:.2e}; labels differ on {(lab != recl)[sure].sum().item()} sure and "
          f"{(lab != recl)[~sure].sum().item()} of {(~sure).sum().item()} unsure pixels; cls_label maps <= {e_cls:.2e} (CAMs x{K.CAM_SCALE:g})")
    assert worst <= PAR_TOL and e_cls <= PAR_TOL * K.CAM_SCALE
    assert torch.equal(lab[sure], recl[sure]) and (~sure).float().mean().item() <= 0.02
    assert set(np.unique(gold[f"ref{i}_bkg_label"]).tolist()) >= {0, 255} and len(np.unique(gold[f"ref{i}_bkg_label"])) >= 3
    assert ((reco == 0) == (out == 0)).all()                                      # zeros outside the boxes and on absent classes


def test_multi_scale(gold):
    x = K.msc_inputs()
    cam, aff = R.multi_scale_cam_with_aff_mat(K.msc_model, _d(x), K.MSC_SCALES)
    e = (cam - torch.from_numpy(gold["msc_cam"]).double()).abs().max().item()
    ea = (aff - torch.from_numpy(gold["msc_aff"]).double()).abs().max().item()
    print(f"multi-scale: cam |f32 reference - fp64| <= {e:.2e}, affinity <= {ea:.2e}")
    assert e <= 1e-5 and ea <= 1e-5 and tuple(aff.shape) == (4, 12, 12)          # index 2 of the list: the 1.5 run's 3 x 4 grid
    assert torch.equal(R.multi_scale_cam(K.msc_model, _d(x), K.MSC_SCALES), cam)
    with pytest.raises(IndexError):
        R.multi_scale_cam_with_aff_mat(K.msc_model, _d(x), (0.5, 1.0, 1.0, 1.5))


def test_chain(gold):
    from weclip_vit_comer_amd.utils.camutils import cams_to_affinity_label, get_mask_by_radius
    c = K.chain_case(gold["sigmoid_table"])
    c.update(images=_d(c["images"]), cams=_d(c["cams"]))
    B, _, H, W = c["cams"].shape
    mask = get_mask_by_radius(*K.CHAIN_GRID, radius=K.CHAIN_RADIUS)
    amask = torch.from_numpy(gold["chain_affinity_mask"])
    r = K.run_chain(R, R.Par(K.DILATIONS, K.NUM_ITER), c, mask, amask,
                    lambda x, size: F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False), cams_to_affinity_label)
    assert np.array_equal(r["pseudo_label"].numpy(), gold["chain_pseudo_label"])
    s_aff = K.unpack(gold["chain_aff_sure_exact"], (B, H, W))
    s_rpl = K.unpack(gold["chain_rpl_sure_exact"], (B, H, W))
    g_aff = torch.from_numpy(gold["chain_aff_label_map"].astype(np.int64))
    g_rpl = torch.from_numpy(gold["chain_refined_pseudo_label"].astype(np.float64))
    assert torch.equal(r["aff_label_map"][s_aff], g_aff[s_aff]) and torch.equal(r["refined_pseudo_label"][s_rpl], g_rpl[s_rpl])
    pair = K.affinity_sure(s_rpl, H, W)
    assert torch.equal(r["affinity_label"][pair], torch.from_numpy(gold["chain_affinity_label"].astype(np.int64))[pair])
    assert len(np.unique(gold["chain_aff_label_map"])) >= 3 and len(np.unique(gold["chain_affinity_label"])) == 3
