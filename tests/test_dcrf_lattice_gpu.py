"""The permutohedral-lattice bilateral term of the dense CRF on the MI355X (csrc/dcrf_lattice.hip, utils/dcrf.py
bilateral="lattice") against the fp64 restatement tests/dcrf_lattice_ref.py.

Every output, the value rows and the workspace are NaN-filled before a call, so an element the kernels do not write fails
the comparison.  Measured on the MI355X (worst scaled error |err| / (M64 + 2^-24 / eps), bound eps = 2^-10 = 9.8e-4): see
DESIGN.md "Dense CRF", "The lattice"."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcrf_lattice_ref as LR  # noqa: E402
import dcrf_ref as R  # noqa: E402
from test_dcrf_gpu import CRF_PROC, EPS, _image, _q  # noqa: E402

NAN = float("nan")


def _mods():
    from weclip_vit_comer_amd import _lib as L
    from weclip_vit_comer_amd.utils import dcrf
    return L, dcrf


def _lattice(img, C, H, W, bxy, brgb):
    L, dcrf = _mods()
    lt = dcrf._Lattice(img.cuda(), C, H, W, bxy, brgb)
    lt.vals.fill_(NAN)
    lt.ws.fill_(NAN)
    return lt


def _filter(lt, V):
    L, _ = _mods()
    C, H, W = V.shape
    out = torch.full((C, H, W), NAN, device="cuda")
    gv = V.float().cuda().contiguous()
    L.lib().wc_dcrf_lattice_filter(L.ptr(lt.lat), L.ptr(gv), L.ptr(out), L.ptr(lt.vals), L.ptr(lt.ws), C, H, W, lt.M, L.stream())
    torch.cuda.synchronize()
    return out.cpu().double()


def _message(lt, Q, pos):
    L, _ = _mods()
    C, H, W = Q.shape
    mp = torch.full((C, H, W), NAN, device="cuda")
    mb, S = mp.clone(), torch.full((2, H, W), NAN, device="cuda")
    gq = Q.cuda().contiguous()
    lt.vals.fill_(NAN)
    lt.ws.fill_(NAN)
    L.lib().wc_dcrf_lattice_message(L.ptr(lt.lat), L.ptr(gq), L.ptr(mp), L.ptr(mb), L.ptr(S), L.ptr(lt.vals), L.ptr(lt.ws), C, H, W,
                                    lt.M, float(pos), L.stream())
    torch.cuda.synchronize()
    return mp.cpu().double(), mb.cpu().double(), S.cpu().double()


def _check(got, ref, what):
    ref = torch.as_tensor(ref)
    bad = (got - ref).abs() > EPS * ref.abs() + 2.0 ** -24
    worst = ((got - ref).abs() / (ref.abs() + 2.0 ** -24 / EPS)).max().item()
    print(f"{what}: worst scaled error {worst:.3e}")
    assert torch.isfinite(got).all().item() and not bad.any().item(), f"{what}: worst scaled error {worst:.3e}"
    return worst


def _values(C, H, W, seed):
    return torch.rand(C, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _filter_and_message(img, H, W, C, bxy, brgb, pos=3.0, gaussian=True):
    ref = LR.build(img, H, W, bxy, brgb)
    lt = _lattice(img, C, H, W, bxy, brgb)
    assert lt.M == ref.M, (lt.M, ref.M)
    V, Q = _values(C, H, W, seed=C + 1), _q(C, H, W, seed=C)
    tag = f"{H}x{W} C={C} {img.dtype} stds=({bxy:g},{brgb:g}) M={lt.M}"
    _check(_filter(lt, V), LR.filter_planes(ref, V), tag + " filter")
    mp, mb, S = _message(lt, Q, pos)
    rb, sb = LR.message(ref, Q)
    _check(mb, rb, tag + " message")
    assert ((S[1] - torch.as_tensor(sb)).abs() <= EPS * torch.as_tensor(sb)).all()
    if gaussian:
        rp, _, sp, _ = R.messages(img, Q, pos, bxy, brgb)
        _check(mp, rp, tag + " gaussian")
        assert ((S[0] - sp).abs() <= EPS * sp).all()


CASES = [((1, 1), 1), ((1, 64), 2), ((64, 1), 21), ((37, 53), 81), ((64, 64), 21), ((37, 53), 128)]


@pytest.mark.parametrize("bxy,brgb", [(16.0, 13.0), (64.0, 5.0)])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("hw,C", CASES)
def test_filter_and_message_vs_fp64(hw, C, u8, bxy, brgb):
    H, W = hw
    _filter_and_message(_image(H, W, u8, seed=H * 7 + W + C), H, W, C, bxy, brgb)


def _smallest_xy_std(H, W, brgb):
    """The smallest bi_xy_std (as an f32) that the a-priori key bound admits at this shape."""
    L, _ = _mods()
    b = ctypes.c_double()

    def ok(xy):
        try:
            L.lib().wc_dcrf_lattice_key_bound(H, W, xy, brgb, ctypes.byref(b))
            return True
        except RuntimeError:
            return False
    lo, hi = 1e-3, 16.0
    assert not ok(lo) and ok(hi)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    xy = float(np.nextafter(np.float32(hi), np.float32(np.inf)))
    assert ok(xy) and not ok(0.99 * xy)
    return xy


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("which", ["wide", "smallest"])
def test_extreme_stds_inside_the_key_bound(which, u8):
    H, W, C = 37, 53, 21
    bxy = 1000.0 if which == "wide" else _smallest_xy_std(H, W, 13.0)
    _filter_and_message(_image(H, W, u8, seed=5), H, W, C, bxy, 13.0, gaussian=False)


def test_stds_outside_the_key_bound_raise_and_write_nothing():
    L, dcrf = _mods()
    H, W, C = 37, 53, 21
    img = _image(H, W, True, seed=5).cuda()
    with pytest.raises(RuntimeError, match="key bound"):
        dcrf.lattice_filter(img, _values(C, H, W, 1).cuda(), 16.0, 0.1)
    with pytest.raises(RuntimeError, match="key bound"):
        dcrf.DenseCRF(10, 3, 3, 4, 16, 0.1, bilateral="lattice")(img, _q(C, H, W, 1).cuda())
    nl, nw = ctypes.c_long(), ctypes.c_long()
    L.lib().wc_dcrf_lattice_workspace_bytes(C, H, W, ctypes.byref(nl), ctypes.byref(nw))
    lat = torch.full((nl.value // 4,), NAN, device="cuda")
    with pytest.raises(RuntimeError, match="key bound"):
        L.lib().wc_dcrf_lattice_build(L.ptr(img), 1, L.ptr(lat), H, W, 16.0, 0.1, L.stream())
    torch.cuda.synchronize()
    assert torch.isnan(lat).all().item()


def test_float_colours_outside_the_range_are_reported():
    _, dcrf = _mods()
    H, W = 16, 24
    img = _image(H, W, False, seed=2)
    img[3, 4, 1] = 300.0
    with pytest.raises(RuntimeError, match="colours"):
        dcrf.lattice_filter(img.cuda(), _values(2, H, W, 1).cuda(), 16.0, 13.0)


@pytest.mark.parametrize("t", [0, 1, 10])
@pytest.mark.parametrize("hw,C", [((37, 53), 21), ((64, 64), 81), ((16, 24), 2)])
def test_inference_vs_fp64(t, hw, C):
    _, dcrf = _mods()
    H, W = hw
    g = torch.Generator().manual_seed(t + C)
    img = _image(H, W, True, seed=11)
    P = torch.softmax(2 * torch.randn(C, H, W, generator=g), 0)
    Q = dcrf.DenseCRF(t, 3, 3, 4, 16, 5, bilateral="lattice")(img.numpy(), P.numpy())
    assert isinstance(Q, np.ndarray) and Q.dtype == np.float32 and Q.shape == (C, H, W)
    Q64 = LR.inference(img, R.unary_from_prob(P), t, 3, 3, 4, 16, 5)
    err = (torch.from_numpy(Q).double() - Q64).abs().max().item()
    top2 = Q64.topk(2, 0).values
    sure = (top2[0] - top2[1]) > 1e-2
    agree = (torch.from_numpy(Q).argmax(0) == Q64.argmax(0))
    print(f"t={t} {H}x{W} C={C}: max |Q - Q64| {err:.2e}")
    assert err <= 1e-2 and agree[sure].all().item()


def test_crf_labels_flat_regions():
    """Two flat colour regions with noisy probabilities come out labelled as the regions."""
    _, dcrf = _mods()
    H, W = 48, 64
    img = np.zeros((H, W, 3), np.uint8)
    img[:, :32] = (200, 40, 40)
    img[:, 32:] = (30, 60, 220)
    truth = np.zeros((H, W), np.int64)
    truth[:, 32:] = 1
    rng = np.random.default_rng(0)
    p1 = np.clip(np.where(truth == 1, 0.65, 0.35) + rng.normal(0, 0.25, (H, W)), 0.01, 0.99)
    P = np.stack([1 - p1, p1]).astype(np.float32)
    assert (P.argmax(0) != truth).mean() > 0.1
    Q = dcrf.DenseCRF(10, 3, 3, 10, 50, 5, bilateral="lattice")(img, P)
    assert (Q.argmax(0) == truth).all()


def test_constant_image_is_one_cell_with_long_segments():
    """64x64 of one colour at (1000, 13): the pixels lie in one or two adjacent simplices, so a handful of vertices own up
    to 4096 entries each and the splat goes through its chunked path (segments of several 256-entry chunks)."""
    H, W, C = 64, 64, 21
    img = torch.full((H, W, 3), 117, dtype=torch.uint8)
    ref = LR.build(img, H, W, 1000.0, 13.0)
    assert ref.M <= 2 * (LR.D + 1) and np.bincount(ref.vert.reshape(-1)).max() > 4 * 256
    _filter_and_message(img, H, W, C, 1000.0, 13.0, gaussian=False)


def test_full_size_crf_proc():
    """500x375, C = 21, crf_proc's parameters: one message against the restatement; the inference is normalised, finite and
    bit-identical from call to call."""
    _, dcrf = _mods()
    H, W, C = 375, 500, 21
    g = torch.Generator().manual_seed(3)
    base = torch.rand(3, 6, 8, generator=g) * 255
    img = (F.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
           + 8 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)
    Q = _q(C, H, W, seed=4)
    p = CRF_PROC
    ref = LR.build(img, H, W, p["bi_xy_std"], p["bi_rgb_std"])
    lt = _lattice(img, C, H, W, p["bi_xy_std"], p["bi_rgb_std"])
    assert lt.M == ref.M
    _, mb, S = _message(lt, Q, p["pos_xy_std"])
    rb, sb = LR.message(ref, Q)
    _check(mb, rb, f"500x375 C=21 M={lt.M} message")
    assert ((S[1] - torch.as_tensor(sb)).abs() <= EPS * torch.as_tensor(sb)).all()
    crf = dcrf.DenseCRF(**p, bilateral="lattice")
    P = torch.softmax(2 * torch.randn(C, H, W, generator=g), 0).cuda()
    Q1 = crf(img.cuda(), P)
    Q2 = crf(img.cuda(), P)
    assert Q1.is_cuda and torch.isfinite(Q1).all().item()
    assert (Q1.sum(0) - 1).abs().max().item() < 1e-5
    assert torch.equal(Q1, Q2)


def test_add_with_crf_on_tiny_coco():
    from test_msc_flip_gpu import _coco_model
    from make_golden import coco_inputs
    from weclip_vit_comer_amd.msc_flip import MscFlipEvaluator
    from weclip_vit_comer_amd.utils import dcrf
    m = _coco_model()
    ev = MscFlipEvaluator(m, 81, scales=(1.0, 0.75), resize_long=96, crf=dcrf.DenseCRF(**CRF_PROC, bilateral="lattice"))
    n = 0
    for i, (_, img, lab) in enumerate(coco_inputs()):
        Hl, Wl = lab.shape
        rgb = torch.randint(0, 256, (Hl, Wl, 3), generator=torch.Generator().manual_seed(i), dtype=torch.uint8)
        _, _, cp = ev.add_with_crf(img[None].cuda(), lab[None].cuda(), rgb.numpy())
        assert cp.shape == lab.shape
        n += int(((lab >= 0) & (lab < 81)).sum())
    assert int(ev.crf_hist.sum()) == n == int(ev.msc_hist.sum())
    assert 0.0 <= ev.crf_scores()["pAcc"] <= 1.0


def test_torch_op_equals_the_python_path():
    import weclip_vit_comer_amd
    _, dcrf = _mods()
    weclip_vit_comer_amd.register_torch_ops()
    H, W, C = 40, 56, 21
    img = _image(H, W, True, seed=9)
    P = torch.softmax(torch.randn(C, H, W, generator=torch.Generator().manual_seed(9)), 0)
    Qp = dcrf.DenseCRF(**CRF_PROC, bilateral="lattice")(img.cuda(), P.cuda())
    Qo = torch.ops.weclip.dense_crf_lattice(img.cuda(), P.cuda(), 10, 3.0, 3.0, 4.0, 64.0, 5.0)
    assert torch.equal(Qp, Qo)
    assert not torch.equal(Qp, dcrf.DenseCRF(**CRF_PROC)(img.cuda(), P.cuda()))          # the exact path is another function
    with pytest.raises(NotImplementedError):
        torch.ops.weclip.dense_crf_lattice(img, P, 10, 3.0, 3.0, 4.0, 64.0, 5.0)
