"""Dense CRF on the MI355X (csrc/dcrf.hip, utils/dcrf.py) against the fp64 reference tests/dcrf_ref.py.

Every output is NaN-filled before a call, so an element the kernels do not write fails the comparison."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcrf_ref as R  # noqa: E402

EPS = 2.0 ** -10            # include/weclip_hip.h: |M - M64| <= eps M64 + 2^-24
CRF_PROC = dict(iter_max=10, pos_w=3, pos_xy_std=3, bi_w=4, bi_xy_std=64, bi_rgb_std=5)


def _lib():
    from weclip_vit_comer_amd import _lib as L
    return L


def _ws(C, H, W):
    L = _lib()
    n = ctypes.c_long()
    L.lib().wc_dcrf_workspace_floats(C, H, W, ctypes.byref(n))
    return torch.full((n.value,), float("nan"), device="cuda")


def _image(H, W, u8, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    return img if u8 else img.float() + torch.rand(H, W, 3, generator=g) * 0.99


def _q(C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(3 * torch.randn(C, H, W, generator=g, dtype=torch.float64), 0).float()


def _message(img, Q, pos, bxy, brgb):
    L = _lib()
    C, H, W = Q.shape
    mp = torch.full((C, H, W), float("nan"), device="cuda")
    mb, S = mp.clone(), torch.full((2, H, W), float("nan"), device="cuda")
    gi, gq, ws = img.cuda().contiguous(), Q.cuda().contiguous(), _ws(C, H, W)
    L.lib().wc_dcrf_message(L.ptr(gi), 1 if img.dtype == torch.uint8 else 0, L.ptr(gq), L.ptr(mp), L.ptr(mb), L.ptr(S), L.ptr(ws),
                            C, H, W, float(pos), float(bxy), float(brgb), L.stream())
    torch.cuda.synchronize()
    return mp.cpu().double(), mb.cpu().double(), S.cpu().double()


def _check_msg(got, ref, what):
    bad = (got - ref).abs() > EPS * ref + 2.0 ** -24
    worst = ((got - ref).abs() / (ref + 2.0 ** -24 / EPS)).max().item()
    assert not bad.any().item() and torch.isfinite(got).all().item(), f"{what}: worst scaled error {worst:.3e}"
    return worst


CASES = [((1, 1), 1), ((1, 64), 2), ((64, 1), 21), ((37, 53), 81), ((64, 64), 21), ((37, 53), 2), ((64, 64), 81), ((37, 53), 128)]


@pytest.mark.parametrize("hw,C", CASES)
@pytest.mark.parametrize("u8", [True, False])
def test_message_vs_fp64(hw, C, u8):
    H, W = hw
    img, Q = _image(H, W, u8, seed=H * 7 + W + C), _q(C, H, W, seed=C)
    mp, mb, S = _message(img, Q, 3.0, 16.0, 13.0)
    rp, rb, sp, sb = R.messages(img, Q, 3.0, 16.0, 13.0)
    w1 = _check_msg(mp, rp, "gaussian")
    w2 = _check_msg(mb, rb, "bilateral")
    assert ((S[0] - sp).abs() <= EPS * sp).all() and ((S[1] - sb).abs() <= EPS * sb).all()
    print(f"{H}x{W} C={C} u8={u8}: worst |err| / (M64 + 2^-24/eps): gaussian {w1:.2e}, bilateral {w2:.2e}")


@pytest.mark.parametrize("bxy,brgb", [(0.5, 13.0), (1000.0, 13.0), (16.0, 0.1), (1000.0, 0.1)])
@pytest.mark.parametrize("u8", [True, False])
def test_message_extreme_stds(bxy, brgb, u8):
    H, W, C = 37, 53, 21
    img, Q = _image(H, W, u8, seed=5), _q(C, H, W, seed=6)
    mp, mb, S = _message(img, Q, 0.5 if bxy == 0.5 else 3.0, bxy, brgb)
    rp, rb, sp, sb = R.messages(img, Q, 0.5 if bxy == 0.5 else 3.0, bxy, brgb)
    _check_msg(mp, rp, "gaussian")
    _check_msg(mb, rb, "bilateral")
    if brgb == 0.1:             # random colours: the bilateral kernel is nearly the identity, M ~ n^2 Q
        assert (sb - 1).abs().max().item() < 1e-3


@pytest.mark.parametrize("t", [0, 1, 10])
@pytest.mark.parametrize("hw,C", [((37, 53), 21), ((64, 64), 81), ((16, 24), 2)])
def test_inference_vs_fp64(t, hw, C):
    from weclip_vit_comer_amd.utils import dcrf
    H, W = hw
    g = torch.Generator().manual_seed(t + C)
    img = _image(H, W, True, seed=11)
    P = torch.softmax(2 * torch.randn(C, H, W, generator=g), 0)
    Q = dcrf.DenseCRF(t, 3, 3, 4, 16, 5)(img.numpy(), P.numpy())
    assert isinstance(Q, np.ndarray) and Q.dtype == np.float32 and Q.shape == (C, H, W)
    Q64 = R.inference(img, R.unary_from_prob(P), t, 3, 3, 4, 16, 5)
    err = (torch.from_numpy(Q).double() - Q64).abs().max().item()
    top2 = Q64.topk(2, 0).values if C > 1 else None
    sure = (top2[0] - top2[1]) > 1e-2
    agree = (torch.from_numpy(Q).argmax(0) == Q64.argmax(0))
    print(f"t={t} {H}x{W} C={C}: max |Q - Q64| {err:.2e}")
    assert err <= 1e-2 and agree[sure].all().item()


def test_full_size_crf_proc():
    """500x375, C = 21, crf_proc's parameters: the message at 256 pixels against fp64; the inference is normalised, finite
    and bit-identical from call to call."""
    from weclip_vit_comer_amd.utils import dcrf
    H, W, C = 375, 500, 21
    g = torch.Generator().manual_seed(3)
    # smooth colour regions plus noise: a realistic bilateral neighbourhood
    base = torch.rand(3, 6, 8, generator=g) * 255
    img = (F.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
           + 8 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)
    Q = _q(C, H, W, seed=4)
    p = CRF_PROC
    mp, mb, S = _message(img, Q, p["pos_xy_std"], p["bi_xy_std"], p["bi_rgb_std"])
    rows = torch.randint(0, H * W, (256,), generator=g)
    rp, rb, sp, sb = R.messages(img, Q, p["pos_xy_std"], p["bi_xy_std"], p["bi_rgb_std"], rows=rows, S_given=(S[0], S[1]))
    _check_msg(mp.reshape(C, -1)[:, rows], rp, "gaussian")
    w = _check_msg(mb.reshape(C, -1)[:, rows], rb, "bilateral")
    assert ((S[1].reshape(-1)[rows] - sb).abs() <= EPS * sb).all() and ((S[0].reshape(-1)[rows] - sp).abs() <= EPS * sp).all()
    crf = dcrf.DenseCRF(**p)
    P = torch.softmax(2 * torch.randn(C, H, W, generator=g), 0).cuda()
    Q1 = crf(img.cuda(), P)
    Q2 = crf(img.cuda(), P)
    assert Q1.is_cuda and torch.isfinite(Q1).all().item()
    assert (Q1.sum(0) - 1).abs().max().item() < 1e-5
    assert torch.equal(Q1, Q2)
    print(f"500x375 C=21: sampled bilateral worst scaled error {w:.2e}")


def test_crf_labels_flat_regions():
    """Two flat colour regions with noisy probabilities come out labelled as the regions."""
    from weclip_vit_comer_amd.utils import dcrf
    H, W = 48, 64
    img = np.zeros((H, W, 3), np.uint8)
    img[:, :32] = (200, 40, 40)
    img[:, 32:] = (30, 60, 220)
    truth = np.zeros((H, W), np.int64)
    truth[:, 32:] = 1
    rng = np.random.default_rng(0)
    p1 = np.clip(np.where(truth == 1, 0.65, 0.35) + rng.normal(0, 0.25, (H, W)), 0.01, 0.99)
    P = np.stack([1 - p1, p1]).astype(np.float32)
    assert (P.argmax(0) != truth).mean() > 0.1                   # the unary alone is wrong in many pixels
    Q = dcrf.DenseCRF(10, 3, 3, 10, 50, 5)(img, P)
    assert (Q.argmax(0) == truth).all()


def test_numpy_api_equals_torch_api_and_reference_shapes():
    from weclip_vit_comer_amd.utils import dcrf
    H, W, C = 40, 56, 21
    img = _image(H, W, True, seed=9).numpy()
    g = torch.Generator().manual_seed(9)
    P = torch.softmax(torch.randn(C, H, W, generator=g), 0).numpy()
    crf = dcrf.DenseCRF(**CRF_PROC)
    Qn = crf(img, P)
    Qt = crf(torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda())
    assert isinstance(Qn, np.ndarray) and Qt.is_cuda and np.array_equal(Qn, Qt.cpu().numpy())
    import weclip_vit_comer_amd
    weclip_vit_comer_amd.register_torch_ops()
    assert np.array_equal(torch.ops.weclip.dense_crf(torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda(), 10, 3.0, 3.0, 4.0,
                                                     64.0, 5.0).cpu().numpy(), Qn)
    q = dcrf.crf_inference(img, P, t=10, scale_factor=1, labels=21)
    assert isinstance(q, np.ndarray) and q.shape == (C, H, W) and q.dtype == np.float32
    assert np.allclose(q.sum(0), 1, atol=1e-5)
    lab = P.argmax(0)
    pred = dcrf.crf_inference_label(img, lab, t=10, n_labels=21, gt_prob=0.7)
    assert isinstance(pred, np.ndarray) and pred.shape == (H, W) and pred.dtype == np.int64
    assert (pred == lab).mean() > 0.2
    U = dcrf.unary_from_labels(torch.from_numpy(lab).cuda(), 21, 0.7).cpu().double()
    assert torch.allclose(U, R.unary_from_labels(lab, 21, 0.7), rtol=1e-6)


def test_unary_from_logits_is_the_crf_proc_composition():
    from weclip_vit_comer_amd.utils import dcrf
    g = torch.Generator().manual_seed(2)
    lg = 4 * torch.randn(81, 13, 17, generator=g)
    U = dcrf.unary_from_logits(lg.cuda(), (50, 71)).cpu().double()
    ref = R.unary_from_prob(F.softmax(F.interpolate(lg[None].double(), size=(50, 71), mode="bilinear", align_corners=False), 1)[0])
    assert (U - ref).abs().max().item() < 1e-4


def test_add_with_crf_on_tiny_coco():
    from test_msc_flip_gpu import _coco_model
    from make_golden import coco_inputs
    from weclip_vit_comer_amd.msc_flip import MscFlipEvaluator
    from weclip_vit_comer_amd.utils import dcrf, evaluate
    m = _coco_model()
    crf = dcrf.DenseCRF(**CRF_PROC)
    ev = MscFlipEvaluator(m, 81, scales=(1.0, 0.75), resize_long=96, crf=crf)
    plain = MscFlipEvaluator(m, 81, scales=(1.0, 0.75), resize_long=96)
    assert plain.crf is None and not hasattr(plain, "crf_hist")
    hand = torch.zeros(81, 81, dtype=torch.int64, device="cuda")
    mism = 0
    for i, (_, img, lab) in enumerate(coco_inputs()):
        Hl, Wl = lab.shape
        rgb = torch.randint(0, 256, (Hl, Wl, 3), generator=torch.Generator().manual_seed(i), dtype=torch.uint8)
        p, mp_, cp = ev.add_with_crf(img[None].cuda(), lab[None].cuda(), rgb.numpy())
        p2, mp2 = plain.add(img[None].cuda(), lab[None].cuda())
        assert torch.equal(p, p2) and torch.equal(mp_, mp2) and cp.shape == lab.shape
        # by hand: F.interpolate -> softmax -> DenseCRF -> argmax
        _, msc = ev.logits(img[None].cuda())
        prob = F.softmax(F.interpolate(msc[None], size=(Hl, Wl), mode="bilinear", align_corners=False), 1)[0]
        ref = crf(rgb.cuda(), prob.contiguous()).argmax(0)
        mism += int((ref != cp).sum())
        evaluate.confusion_hist(lab.cuda(), ref, 81, out=hand)
    assert torch.equal(ev.hist, plain.hist) and torch.equal(ev.msc_hist, plain.msc_hist)
    n = int(hand.sum())
    # the fused logits unary and torch's interpolate + softmax round differently: only fp near-ties of the argmax may move
    assert (ev.crf_hist - hand).abs().sum().item() <= 2 * max(1, n // 500), (mism, n)
    s = ev.crf_scores()
    assert 0.0 <= s["pAcc"] <= 1.0
    print(f"add_with_crf: {mism} of {n} pixels differ from the by-hand composition")
