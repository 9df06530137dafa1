"""GPU tests of csrc/trainlog.hip: `wc_val_pair_hist` against the composition the suite already pins
(`msc_flip.resize_argmax` + `wc_confusion_hist`, twice: integer equality) and against a host restatement in fp64;
`wc_label_match_count` against the torch expression of the reference's pseudo_seg_mAcc, eagerly and inside a captured graph.

Near ties: the fp64 / ATen references round differently from the kernel, so a pixel whose two largest up-sampled logits lie
closer than 1e-4 may legitimately flip.  fp32 bilinear interpolation of O(1) logits carries ~1e-6 of rounding, so 1e-4 is a
hundred times that; such pixels are taken out of BOTH sides (label 255), and each test asserts they are at most 1 %."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TIE = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lds_threshold_nc():
    """Largest nc whose (nc, nc) uint32 histogram the existing confusion_hist_kernel keeps in LDS (read from evalops.hip)."""
    src = open(os.path.join(ROOT, "weclip-vit-comer_amd", "csrc", "evalops.hip")).read()
    kib = int(re.search(r"use_lds = lds <= (\d+) \* 1024", src).group(1))
    return int(np.floor(np.sqrt(kib * 1024 / 4)))


def _reference_hists(seg, cam, gt, nc):
    """resize_argmax + wc_confusion_hist per leg, with a flag of its own (the module-wide one of evaluate stays untouched)."""
    from weclip_vit_comer_amd import _lib as L
    from weclip_vit_comer_amd.msc_flip import resize_argmax
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    hists = []
    for pred in (resize_argmax(seg, tuple(gt.shape)), cam):
        h = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
        if pred is not None:
            L.lib().wc_confusion_hist(L.ptr(gt, torch.int64), L.ptr(pred.contiguous(), torch.int64), L.ptr(h, torch.int64),
                                      L.ptr(flag, torch.int32), gt.numel(), nc, L.stream())
        hists.append(h)
    return hists[0], hists[1], int(flag.item())


def _case(*a, **kw):
    seg, cam, gt = case_host(*a, **kw)
    return seg.cuda(), (None if cam is None else cam.cuda()), gt.cuda()


def case_host(Hs, Ws, Hl, Wl, nc, seed, cam_mode="valid", gt_mode="mixed"):
    g = torch.Generator().manual_seed(seed)
    seg = torch.randn(nc, Hs, Ws, generator=g)
    gt = torch.randint(0, nc, (Hl, Wl), generator=g)
    if gt_mode == "all_ignore":
        gt[:] = 255
    else:
        gt[torch.rand(Hl, Wl, generator=g) < 0.1] = 255
        gt[0, 0] = 0                                                  # at least one counted pixel
    cam = None
    if cam_mode != "none":
        cam = torch.randint(0, nc, (Hl, Wl), generator=g)
        if cam_mode == "out_of_range":
            cam[0, 0] = 255                                            # gt there is a class id: skipped, flag raised
    return seg, cam, gt


CASES = [
    # Hs, Ws, Hl, Wl, nc, cam, gt
    (3, 4, 37, 53, 2, "valid", "mixed"),
    (20, 20, 320, 320, 21, "valid", "mixed"),
    (23, 31, 375, 500, 81, "valid", "mixed"),
    (5, 5, 5, 5, 21, "valid", "mixed"),                                # identity
    (3, 4, 37, 53, "above_lds", "valid", "mixed"),                     # global atomics for both legs
    (20, 20, 320, 320, 100, "valid", "mixed"),                         # two histograms no longer fit in LDS, one would
    (20, 20, 320, 320, 100, "none", "mixed"),                          # ... and does, without the CAM leg
    (23, 31, 375, 500, 21, "none", "mixed"),
    (23, 31, 375, 500, 21, "out_of_range", "mixed"),
    (3, 4, 37, 53, 21, "valid", "all_ignore"),
]


@pytest.mark.parametrize("Hs,Ws,Hl,Wl,nc,cam_mode,gt_mode", CASES)
def test_val_pair_hist_equals_resize_argmax_plus_confusion_hist(Hs, Ws, Hl, Wl, nc, cam_mode, gt_mode):
    from weclip_vit_comer_amd.validate import val_pair_hist
    if nc == "above_lds":
        nc = _lds_threshold_nc() + 2
        assert nc * nc * 4 > 64 * 1024
    seg, cam, gt = _case(Hs, Ws, Hl, Wl, nc, seed=Hs * 1000 + nc, cam_mode=cam_mode, gt_mode=gt_mode)
    ref_seg, ref_cam, ref_flag = _reference_hists(seg, cam, gt, nc)
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    seg_hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
    cam_hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
    val_pair_hist(seg, cam, gt, nc, seg_hist, cam_hist, flag=flag)
    valid = int(((gt >= 0) & (gt < nc)).sum())
    print(f"{(Hs, Ws)}->{(Hl, Wl)} nc {nc} cam {cam_mode} gt {gt_mode}: counted {int(seg_hist.sum())} of {valid} valid pixels, "
          f"seg cells differing {int((seg_hist != ref_seg).sum())}, cam cells differing {int((cam_hist != ref_cam).sum())}, "
          f"flag {int(flag.item())} (reference {ref_flag})")
    assert torch.equal(seg_hist, ref_seg) and torch.equal(cam_hist, ref_cam)
    assert int(flag.item()) == ref_flag == (1 if cam_mode == "out_of_range" else 0)
    assert int(seg_hist.sum()) == valid == (0 if gt_mode == "all_ignore" else valid)
    if cam_mode == "out_of_range":
        assert int(cam_hist.sum()) == valid - 1
    elif cam_mode == "none":
        assert int(cam_hist.sum()) == 0
    # a second call into the same histograms doubles them
    val_pair_hist(seg, cam, gt, nc, seg_hist, cam_hist, flag=flag)
    assert torch.equal(seg_hist, 2 * ref_seg) and torch.equal(cam_hist, 2 * ref_cam)


def _resize_fp64(seg, Hl, Wl):
    """F.interpolate(seg, (Hl, Wl), bilinear, align_corners=False) in numpy fp64 (ATen's source index, size-derived scale)."""
    C, Hs, Ws = seg.shape

    def taps(n_out, n_in):
        s = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        return i0, i1, s - i0
    y0, y1, ly = taps(Hl, Hs)
    x0, x1, lx = taps(Wl, Ws)
    s = seg.astype(np.float64)
    top = s[:, y0][:, :, x0] * (1 - lx) + s[:, y0][:, :, x1] * lx
    bot = s[:, y1][:, :, x0] * (1 - lx) + s[:, y1][:, :, x1] * lx
    return top * (1 - ly)[None, :, None] + bot * ly[None, :, None]


def host_reference(seg, cam, gt, nc):
    """(seg_hist, cam_hist, gt with the near-tie pixels set to 255, their fraction) on the host.  Runs without a GPU."""
    from weclip_vit_comer_amd.utils.evaluate import _fast_hist
    up = _resize_fp64(seg, *gt.shape)
    srt = np.sort(up, axis=0)
    tie = (srt[-1] - srt[-2]) < TIE if nc > 1 else np.zeros(gt.shape, bool)
    gt = np.where(tie, 255, gt)
    return _fast_hist(gt, up.argmax(0), nc), _fast_hist(gt, cam, nc), gt, float(tie.mean())


@pytest.mark.parametrize("Hs,Ws,Hl,Wl,nc,seed", [(3, 4, 37, 53, 2, 5), (23, 31, 375, 500, 21, 6), (20, 20, 320, 320, 81, 7)])
def test_val_pair_hist_equals_fp64_host_restatement(Hs, Ws, Hl, Wl, nc, seed):
    from weclip_vit_comer_amd.validate import val_pair_hist
    seg, cam, gt = _case(Hs, Ws, Hl, Wl, nc, seed=seed)
    ref_seg, ref_cam, gt_kept, tie_frac = host_reference(seg.cpu().numpy(), cam.cpu().numpy(), gt.cpu().numpy(), nc)
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    seg_hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
    cam_hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
    val_pair_hist(seg, cam, torch.from_numpy(gt_kept).cuda(), nc, seg_hist, cam_hist, flag=flag)
    diff = np.abs(seg_hist.cpu().numpy() - ref_seg).sum()
    print(f"{(Hs, Ws)}->{(Hl, Wl)} nc {nc}: near-tie pixels {tie_frac:.4%}, |seg_hist - fp64 reference| summed {diff}")
    assert tie_frac <= 0.01
    assert np.array_equal(seg_hist.cpu().numpy(), ref_seg) and np.array_equal(cam_hist.cpu().numpy(), ref_cam)
    assert int(flag.item()) == 0


def _match_case(B, Hs, Ws, H, W, C=21, seed=0):
    """seg, label (near-tie pixels 255), the torch expression's match count, the near-tie fraction."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    seg = torch.randn(B, C, Hs, Ws, generator=g).cuda()
    up = F.interpolate(seg, size=(H, W), mode="bilinear", align_corners=False)
    top = up.topk(2, dim=1).values
    tie = (top[:, 0] - top[:, 1]) < TIE
    pred = up.argmax(1)
    label = torch.randint(0, C, (B, H, W), generator=g).cuda()
    pick = torch.rand(B, H, W, generator=g).cuda()
    label = torch.where(pick < 0.5, pred, label)                       # half the pixels match by construction
    label = torch.where(pick > 0.9, torch.full_like(label, 255), label)
    label = torch.where(tie, torch.full_like(label, 255), label).contiguous()
    return seg, label, int((pred == label).sum()), float(tie.float().mean()), pred


@pytest.mark.parametrize("B,Hs,Ws,H,W", [(1, 2, 3, 32, 48), (3, 2, 3, 32, 48), (1, 20, 20, 320, 320), (3, 20, 20, 320, 320)])
def test_label_match_count_equals_torch_expression(B, Hs, Ws, H, W):
    from weclip_vit_comer_amd.validate import label_match_count
    seg, label, ref, tie_frac, _ = _match_case(B, Hs, Ws, H, W, seed=B * 100 + Hs)
    counts = torch.full((2,), 12345, device="cuda", dtype=torch.int64)                 # stale values: must be overwritten
    label_match_count(seg, label, counts)
    got = counts.tolist()
    print(f"B {B} {(Hs, Ws)}->{(H, W)}: matches {got[0]} (torch {ref}) of {got[1]}, near-tie pixels {tie_frac:.4%}")
    assert tie_frac <= 0.01
    assert got == [ref, B * H * W] and 0 < ref < B * H * W
    # an all-ignore label: nothing matches; the second call overwrites the first one's count
    label_match_count(seg, torch.full_like(label, 255), counts)
    assert counts.tolist() == [0, B * H * W]
    label_match_count(seg, label, counts)
    assert counts.tolist() == [ref, B * H * W]


def test_label_match_count_in_a_captured_graph_follows_the_label_buffer():
    from weclip_vit_comer_amd.validate import label_match_count
    B, Hs, Ws, H, W = 3, 2, 3, 32, 48
    seg, label_a, ref_a, _, pred = _match_case(B, Hs, Ws, H, W, seed=1)
    label_b = label_a.clone()
    label_b[:, :H // 2] = 255                                                           # (the near-tie pixels stay 255)
    ref_b = int((pred == label_b).sum())
    assert 0 < ref_b < ref_a
    label_match_count(seg, label_b, torch.zeros(2, device="cuda", dtype=torch.int64))   # warms the library up before the capture
    buf, counts = label_a.clone(), torch.zeros(2, device="cuda", dtype=torch.int64)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        label_match_count(seg, buf, counts)
    g.replay()
    assert counts.tolist() == [ref_a, B * H * W]
    buf.copy_(label_b)
    g.replay()
    assert counts.tolist() == [ref_b, B * H * W]
