"""utils.camutils on the MI355X (csrc/camlabel.hip) against the fp64 restatement tests/camutils_ref.py and the reference's own
numbers in tests/golden/camutils_ref.npz.

Random walk: per element |out - out64| <= 2^-20 out64 + 2^-24.  The measured f32-input MFMA chain error is ~1.5e-7 of
sum |a b| at K <= 1024; every term is non-negative, so that sum is the value itself; as much again for the column sum in the
denominator and a few ulp of f32 soft-max leave about 3x margin.
The refine_* functions: continuous maps within the PAR tolerance of tests/test_par_gpu.py for the active precision mode (3e-5
exact, 5e-4 fast), labels equal wherever the reference's recorded top-2 margin exceeds twice that tolerance."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camutils_cases as K  # noqa: E402
import camutils_ref as R  # noqa: E402


def _M():
    from weclip_vit_comer_amd.utils import camutils
    return camutils


@pytest.fixture(scope="module")
def gold(golden):
    return golden("camutils_ref.npz")


@pytest.fixture(scope="module")
def par():
    from weclip_vit_comer_amd.WeCLIP_model.PAR import PAR
    return PAR(K.DILATIONS, K.NUM_ITER).cuda()


@pytest.fixture(params=["exact", "fast"])
def mode(request, monkeypatch):
    """The PAR precision modes, switched the way tests/test_par_gpu.py's `tol` fixture does; -> (name, tolerance)."""
    from weclip_vit_comer_amd import config
    monkeypatch.setattr(config, "precision", request.param)
    return request.param, {"exact": 3e-5, "fast": 5e-4}[request.param]


def _ratio(got, ref64):
    return ((got.cpu().double() - ref64).abs() / (2.0 ** -20 * ref64.abs() + 2.0 ** -24)).max().item()


# ---------------------------------------------------------------------------------------------------------------- random walk
@pytest.mark.parametrize("hw", K.WALK_GRIDS)
@pytest.mark.parametrize("C", K.WALK_C)
def test_walk_vs_fp64(gold, hw, C):
    M = _M()
    h, w = hw
    n = h * w
    c = K.walk_case(h, w, C, gold["sigmoid_table"])
    cams, aff, cls = c["cams"].cuda(), c["aff"].cuda(), c["cls"].cuda()
    aff0 = aff.clone()
    for masked in (0, 1):
        mask = M.get_mask_by_radius(h, w, radius=8) if masked else None
        mask_d = mask.cuda() if masked else None
        mask64 = mask.double() if masked else None
        got = M.propagte_aff_cam_with_bkg(cams, aff=aff, mask=mask_d, cls_labels=cls, bkg_score=K.THRE[0])
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, C + 1, h, w)
        ref = R.propagte_aff_cam_with_bkg(c["cams"].double(), aff=c["aff"], mask=mask64, cls_labels=c["cls"], bkg_score=K.THRE[0])
        r1 = _ratio(got, ref)
        rec = torch.from_numpy(gold[f"walk_bkg_{n}_{C}_{masked}"]).reshape(3, C + 1, h, w)
        r_rec = ((got.cpu().double() - rec.double()).abs() / (2 * (2.0 ** -20 * ref.abs() + 2.0 ** -24))).max().item()
        absent = torch.ones(3, C + 1, dtype=torch.bool)
        absent[:, 0] = False
        absent[:, 1:] = c["cls"] == 0
        assert (got.cpu()[absent] == 0).all()                                   # absent-key rows are exactly 0
        assert (got.cpu().reshape(3, C + 1, n)[1, :, 5] == 0).all()             # the zeroed column: 0 / (0 + eps)
        assert torch.equal(got, M.propagte_aff_cam_with_bkg(cams, aff=aff, mask=mask_d, cls_labels=cls, bkg_score=K.THRE[0]))
        got2 = M.propagte_aff_cam(cams, aff=aff, mask=mask_d)
        assert got2.dtype == torch.float32 and tuple(got2.shape) == (3, C, h, w)
        ref2 = R.propagte_aff_cam(c["cams"].double(), aff=c["aff"], mask=mask64)
        r2 = _ratio(got2, ref2)
        st = K.WALK_STRIDE[n]
        rec2 = torch.from_numpy(gold[f"walk_plain_{n}_{C}_{masked}"]).double()
        r_rec2 = ((got2.cpu().double().reshape(3, C, n)[..., ::st] - rec2).abs()
                  / (2 * (2.0 ** -20 * ref2.reshape(3, C, n)[..., ::st].abs() + 2.0 ** -24))).max().item()
        assert torch.equal(got2, M.propagte_aff_cam(cams, aff=aff, mask=mask_d))   # two calls are bit-identical
        # the reference's recorded f32 output is held to twice the bound
        print(f"walk n={n} C={C} masked={masked}: worst |out - out64| / bound: with bkg {r1:.3f}, plain {r2:.3f}; "
              f"against the recorded f32 reference / (2 bound): with bkg {r_rec:.3f}, plain {r_rec2:.3f}")
        assert r1 <= 1.0 and r2 <= 1.0 and r_rec <= 1.0 and r_rec2 <= 1.0
    assert torch.equal(aff, aff0)                                              # the caller's aff is left as it is


def test_walk_more_than_one_wave_pass_and_ragged_columns():
    """n = 1000: sixteen 64-row passes per wave with a ragged last one, a ragged last column block; K = 33 (two MFMA row tiles)."""
    M = _M()
    B, C, h, w = 2, 32, 25, 40
    n = h * w
    aff = torch.from_numpy(K.noise((B, n, n), 71)).float()
    cams = torch.from_numpy(K.noise((B, C, h, w), 72)).float()
    cls = (torch.from_numpy(K.noise((B, C), 73)) > 0.5).float()
    got = M.propagte_aff_cam_with_bkg(cams.cuda(), aff=aff.cuda(), mask=None, cls_labels=cls.cuda(), bkg_score=0.4)
    r = _ratio(got, R.propagte_aff_cam_with_bkg(cams.double(), aff=aff, mask=None, cls_labels=cls, bkg_score=0.4))
    print(f"walk n={n} K={C + 1}: worst |out - out64| / bound {r:.3f}")
    assert r <= 1.0


def test_walk_op(gold):
    import weclip_vit_comer_amd
    weclip_vit_comer_amd.register_torch_ops()
    M = _M()
    c = K.walk_case(7, 9, 5, gold["sigmoid_table"])
    aff, cams, cls = c["aff"].cuda(), c["cams"].cuda().reshape(3, 5, 63), c["cls"].cuda()
    mask = M.get_mask_by_radius(7, 9, radius=3).cuda()
    o = torch.ops.weclip.aff_propagate(aff, cams, mask, cls, 0.35, True)
    assert torch.equal(o.reshape(3, 6, 7, 9), M.propagte_aff_cam_with_bkg(c["cams"].cuda(), aff=aff, mask=mask, cls_labels=cls, bkg_score=0.35))
    torch.library.opcheck(torch.ops.weclip.aff_propagate, (aff, cams, mask, cls, 0.35, True))
    torch.library.opcheck(torch.ops.weclip.aff_propagate, (aff, cams, None, None, 0.0, False))


# ---------------------------------------------------------------------------------------------------------------- labels
def test_labels_equal_the_reference(gold):
    M = _M()
    c, cfg = K.label_case(), K.make_cfg()
    cam, cls = c["cam"].cuda(), c["cls"].cuda()
    nobox = M.cam_to_label(cam, cls, cfg=cfg)
    assert nobox.dtype == torch.int64 and np.array_equal(nobox.cpu().numpy(), gold["lab_nobox"])
    for box in (c["box"], torch.tensor(c["box"]), torch.tensor(c["box"]).cuda()):
        for mid in (0, 1):
            valid, lab = M.cam_to_label(cam, cls, img_box=box, ignore_mid=bool(mid), cfg=cfg)
            assert lab.dtype == torch.int64 and valid.dtype == torch.float32
            assert np.array_equal(lab.cpu().numpy(), gold[f"lab_mid{mid}"])
            assert K.check(valid) == gold[f"lab_valid_check{mid}"][0] and torch.equal(valid.cpu(), c["cls"][:, :, None, None] * c["cam"])
        out = M.ignore_img_box(nobox, box, 255)
        assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), gold["lab_ign_i64"])
        out = M.ignore_img_box(nobox.float() + 0.25, box, 255)
        assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), gold["lab_ign_f32"])
    with pytest.raises(RuntimeError, match="int64 or float32"):
        M.ignore_img_box(nobox.int(), c["box"], 255)
    # H * W a multiple of four: the 128-bit path, against the restatement
    cam4 = c["cam"][:, :, :32, :44].contiguous()
    valid, lab = M.cam_to_label(cam4.cuda(), cls, img_box=c["box"], ignore_mid=True, cfg=cfg)
    rv, rl = R.cam_to_label(cam4.double(), c["cls"], img_box=c["box"], ignore_mid=True, cfg=cfg)
    assert torch.equal(lab.cpu(), rl) and torch.equal(valid.cpu().double(), rv)


# ---------------------------------------------------------------------------------------------------------------- refine_*
@pytest.mark.parametrize("i", range(len(K.REFINE_SHAPES)))
def test_refine_with_bkg(gold, par, mode, i):
    from weclip_vit_comer_amd.resize import bilinear_resize
    M = _M()
    name, tol = mode
    B, C, H, W = K.REFINE_SHAPES[i]
    c = K.refine_case(i)
    img, cams, cls = c["images"].cuda(), c["cams"].cuda(), c["cls"].cuda()
    keys = [list(k) for k in K.REFINE_PRESENT[C]]
    stack, meta, Kmax = M._bkg_refined_stack(par, img, cams, keys, c["cfg"])
    rec = torch.from_numpy(gold[f"ref{i}_bkg_stack"])
    assert tuple(stack.shape) == tuple(rec.shape) and Kmax == rec.shape[1] // 2
    e_stack = (stack.cpu() - rec).abs().max().item()
    up = bilinear_resize(stack, (H, W)).cpu()
    e_up = (up - F.interpolate(rec, size=(H, W), mode="bilinear", align_corners=False)).abs().max().item()
    lab = M.refine_cams_with_bkg_v2(par, img, cams, cls, c["cfg"], c["box_bkg"])
    assert lab.dtype == torch.float32 and tuple(lab.shape) == (B, H, W)
    assert torch.equal(lab, M.refine_cams_with_bkg_v2(par, img, cams, None, c["cfg"], torch.tensor(c["box_bkg"]).cuda(), keys=keys))
    sure = K.unpack(gold[f"ref{i}_bkg_sure_{name}"], (B, H, W))
    recl = torch.from_numpy(gold[f"ref{i}_bkg_label"].astype(np.float32))
    bad = (lab.cpu() != recl)
    print(f"refine_cams_with_bkg_v2 case {i} {name}: refined stack |ours - reference| <= {e_stack:.2e}, after the up-sample <= {e_up:.2e} "
          f"(tolerance {tol:.0e}); labels differ on {bad[sure].sum().item()} sure pixels and {bad[~sure].sum().item()} of "
          f"{(~sure).sum().item()} left out ({(~sure).float().mean().item():.2%} of the pixels)")
    assert e_stack <= tol and e_up <= tol
    assert (~sure).float().mean().item() <= 0.02 and not bad[sure].any()


@pytest.mark.parametrize("i", range(len(K.REFINE_SHAPES)))
def test_refine_with_cls_label(gold, par, mode, i):
    M = _M()
    name, tol = mode
    B, C, H, W = K.REFINE_SHAPES[i]
    c = K.refine_case(i)
    img, cams, cls = c["images"].cuda(), c["cams"].cuda(), c["cls"].cuda()
    out = M.refine_cams_with_cls_label(par, img, cls, cams, c["box_cls"])
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, C, H, W)
    rec = torch.from_numpy(gold[f"ref{i}_cls_out"])
    zero = rec == 0
    e = (out.cpu() - rec).abs().max().item()
    print(f"refine_cams_with_cls_label case {i} {name}: |ours - reference| <= {e:.2e} on maps that reach {rec.max().item():.1f} "
          f"(tolerance {tol:.0e})")
    assert e <= tol
    assert (out.cpu()[zero] == 0).all() and zero.float().mean().item() > 0.5      # zeros outside the boxes, on absent keys: exact
    keys = [list(k) for k in K.REFINE_PRESENT[C]]
    assert torch.equal(out, M.refine_cams_with_cls_label(par, img, None, cams, c["box_cls"], keys=keys))


# ---------------------------------------------------------------------------------------------------------------- multi-scale
def test_multi_scale(gold):
    M = _M()
    x = K.msc_inputs().cuda()
    cam, aff = M.multi_scale_cam_with_aff_mat(K.msc_model, x, K.MSC_SCALES)
    e = (cam.cpu() - torch.from_numpy(gold["msc_cam"])).abs().max().item()
    ea = (aff.cpu() - torch.from_numpy(gold["msc_aff"])).abs().max().item()
    print(f"multi-scale: cam |ours - reference| <= {e:.2e}, affinity <= {ea:.2e}")
    assert cam.dtype == torch.float32 and e <= 1e-5 and ea <= 1e-5 and tuple(aff.shape) == (4, 12, 12)
    assert torch.equal(M.multi_scale_cam(K.msc_model, x, K.MSC_SCALES), cam)
    with pytest.raises(IndexError):
        M.multi_scale_cam_with_aff_mat(K.msc_model, x, (0.5, 1.0, 1.0, 1.5))


# ---------------------------------------------------------------------------------------------------------------- synchronisation
def test_host_synchronisation(gold, par):
    M = _M()
    c = K.refine_case(1)
    cfg, box = c["cfg"], c["box_cls"]
    img, cams, cls = c["images"].cuda(), c["cams"].cuda(), c["cls"].cuda()
    keys = [list(k) for k in K.REFINE_PRESENT[20]]
    w = K.walk_case(7, 9, 5, gold["sigmoid_table"])
    waff, wcams, wcls = w["aff"].cuda(), w["cams"].cuda(), w["cls"].cuda()
    mask = M.get_mask_by_radius(7, 9, radius=3).cuda()
    box_dev = torch.tensor(box).cuda()
    M.refine_cams_with_bkg_v2(par, img, cams, cls, cfg, box, keys=keys)          # warm: nothing lazy is left for the checked runs
    M.refine_cams_with_cls_label(par, img, cls, cams, box, keys=keys)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in (box, box_dev):
            _, lab = M.cam_to_label(cams, cls, img_box=b, ignore_mid=True, cfg=cfg)
            M.ignore_img_box(lab, b, 255)
        M.cam_to_label(cams, cls, cfg=cfg)
        M.propagte_aff_cam(wcams, aff=waff, mask=mask)
        M.propagte_aff_cam_with_bkg(wcams, aff=waff, mask=mask, cls_labels=wcls, bkg_score=0.35)
        M.refine_cams_with_bkg_v2(par, img, cams, cls, cfg, box, keys=keys)
        M.refine_cams_with_bkg_v2(par, img, cams, cls, cfg, box_dev, keys=keys)
        M.refine_cams_with_cls_label(par, img, cls, cams, box, keys=keys)
        torch.cuda.set_sync_debug_mode("warn")
        counts = []
        for call in (lambda: M.refine_cams_with_bkg_v2(par, img, cams, cls, cfg, box),
                     lambda: M.refine_cams_with_bkg_v2(par, img, cams, cls, cfg, box_dev),
                     lambda: M.refine_cams_with_cls_label(par, img, cls, cams, box),
                     lambda: M.refine_cams_with_cls_label(par, img, cls, cams, box_dev)):
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                call()
            # torch words its finding "called a synchronizing CUDA operation" (tests/test_energy_gpu.py)
            counts.append(len([1 for m in caught if "called a synchronizing" in str(m.message)]))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert counts == [1, 1, 1, 1], counts


# ---------------------------------------------------------------------------------------------------------------- the chain
def test_training_step_chain(gold, par, mode):
    """scripts/.ipynb_checkpoints/dist_train_voc-checkpoint.py:310-339 on the (3, 20, 34, 46) case."""
    from weclip_vit_comer_amd.resize import bilinear_resize
    M = _M()
    name, _ = mode
    c = K.chain_case(gold["sigmoid_table"])
    for k in ("images", "cams", "cls", "aff"):
        c[k] = c[k].cuda()
    B, _, H, W = c["cams"].shape
    aff0 = c["aff"].clone()
    mask = M.get_mask_by_radius(*K.CHAIN_GRID, radius=K.CHAIN_RADIUS).cuda()
    amask = torch.from_numpy(gold["chain_affinity_mask"]).cuda()
    r = {k: v.cpu() for k, v in K.run_chain(M, par, c, mask, amask, bilinear_resize, M.cams_to_affinity_label).items()}
    assert torch.equal(c["aff"], aff0)
    assert np.array_equal(r["pseudo_label"].numpy(), gold["chain_pseudo_label"])
    s_aff = K.unpack(gold[f"chain_aff_sure_{name}"], (B, H, W))
    s_rpl = K.unpack(gold[f"chain_rpl_sure_{name}"], (B, H, W))
    g_aff = torch.from_numpy(gold["chain_aff_label_map"].astype(np.int64))
    g_rpl = torch.from_numpy(gold["chain_refined_pseudo_label"].astype(np.float32))
    g_al = torch.from_numpy(gold["chain_affinity_label"].astype(np.int64))
    pair = K.affinity_sure(s_rpl, H, W)
    bad_a, bad_r = r["aff_label_map"] != g_aff, r["refined_pseudo_label"] != g_rpl
    print(f"chain {name}: refined_aff_label differs on {bad_a[s_aff].sum().item()} sure and {bad_a[~s_aff].sum().item()} of "
          f"{(~s_aff).sum().item()} left-out pixels; refined_pseudo_label on {bad_r[s_rpl].sum().item()} and {bad_r[~s_rpl].sum().item()} of "
          f"{(~s_rpl).sum().item()}")
    assert r["aff_label_map"].dtype == torch.int64 and r["refined_pseudo_label"].dtype == torch.float32
    assert (~s_aff).float().mean().item() <= 0.02 and (~s_rpl).float().mean().item() <= 0.02
    assert not bad_a[s_aff].any() and not bad_r[s_rpl].any()
    assert torch.equal(r["affinity_label"][pair], g_al[pair]) and pair.float().mean().item() > 0.5
