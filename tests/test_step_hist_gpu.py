"""GPU tests of `wc_step_pair_hist` (csrc/trainlog.hip, validate.step_pair_hist): the batched confusion counts of a supervised
train step against the per-image composition the suite already pins (`msc_flip.resize_argmax` + `wc_confusion_hist`, integer
equality), its accumulate and out-of-range contracts, and an independent fp64 numpy restatement."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (C = nc, (Hs, Ws), (H, W)); the last one's 130 * 130 * 4 bytes exceed 64 KiB of LDS: the global-atomic path
SHAPES = [(3, (4, 4), (16, 16)), (21, (5, 7), (33, 47)), (21, (9, 9), (7, 5)), (81, (4, 4), (32, 32)), (130, (4, 4), (16, 16))]
OUT_OF_RANGE = 200                                                       # >= every nc above, and not the ignore value


def _labels(B, H, W, nc, mode, g):
    """mixed: class ids with 255, one other out-of-range value and a negative one sprinkled in; one_class: a single class
    throughout (every lane of every wave counts into one row of the matrix: the hot-cell case)."""
    if mode == "one_class":
        return torch.full((B, H, W), nc - 1, dtype=torch.int64)
    lab = torch.randint(0, nc, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    lab[r < 0.10] = 255
    lab[(r >= 0.10) & (r < 0.15)] = OUT_OF_RANGE
    lab[(r >= 0.15) & (r < 0.20)] = -1
    lab[:, 0, 0], lab[:, 0, 1], lab[:, 1, 0], lab[:, 1, 1], lab[:, 2, 0] = 255, OUT_OF_RANGE, -7, 0, -1    # each kind in every image
    return lab


def _reference(seg, label, nc):
    """Per image: resize_argmax + wc_confusion_hist, summed over the batch, with a flag of its own (evaluate's stays clean)."""
    from weclip_vit_comer_amd import _lib as L
    from weclip_vit_comer_amd.msc_flip import resize_argmax
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
    for b in range(seg.shape[0]):
        pred = resize_argmax(seg[b].contiguous(), tuple(label.shape[1:]))
        L.lib().wc_confusion_hist(L.ptr(label[b].contiguous(), torch.int64), L.ptr(pred, torch.int64), L.ptr(hist, torch.int64),
                                  L.ptr(flag, torch.int32), pred.numel(), nc, L.stream())
    return hist, int(flag.item())


@pytest.mark.parametrize("mode", ["mixed", "one_class"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nc,hw,HW", SHAPES)
def test_step_pair_hist_equals_resize_argmax_plus_confusion_hist(nc, hw, HW, B, mode):
    from weclip_vit_comer_amd.validate import step_pair_hist
    g = torch.Generator().manual_seed(1000 * nc + 10 * B + HW[0])
    seg = torch.randn(B, nc, *hw, generator=g).cuda()
    label = _labels(B, *HW, nc, mode, g).cuda()
    ref, ref_flag = _reference(seg, label, nc)
    hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    assert step_pair_hist(seg, label, nc, hist, flag) is hist
    valid = int(((label >= 0) & (label < nc)).sum())
    print(f"B {B} nc {nc} {hw}->{HW} {mode}: counted {int(hist.sum())} of {valid} valid pixels, cells differing "
          f"{int((hist != ref).sum())}")
    assert torch.equal(hist, ref)
    assert int(hist.sum()) == valid > 0 and int(flag.item()) == ref_flag == 0
    if mode == "mixed":
        assert valid < label.numel() and all(int((label == v).sum()) > 0 for v in (255, OUT_OF_RANGE, -1, -7))
    else:
        assert int(hist[nc - 1].sum()) == valid == label.numel()
    # the entry adds: a second call doubles the matrix
    step_pair_hist(seg, label, nc, hist, flag)
    assert torch.equal(hist, 2 * ref)


@pytest.mark.parametrize("nc,hw,HW", [(21, (5, 7), (33, 47)), (130, (4, 4), (16, 16))])
def test_step_pair_hist_skips_and_flags_a_prediction_outside_the_matrix(nc, hw, HW):
    """C = nc + 2 logit planes; the two extra classes win in part of the batch: those pixels are absent, the flag is raised,
    every other pixel is counted as the composition counts it."""
    from weclip_vit_comer_amd.validate import step_pair_hist
    B = 3
    g = torch.Generator().manual_seed(nc)
    seg = torch.randn(B, nc + 2, *hw, generator=g)
    seg[0, nc, :2] += 50.0                                               # class nc wins over the top of image 0
    seg[2, nc + 1, :, -1] += 50.0                                        # class nc + 1 over the right edge of image 2
    seg = seg.cuda()
    label = _labels(B, *HW, nc, "mixed", g).cuda()
    ref, ref_flag = _reference(seg, label, nc)
    hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    step_pair_hist(seg, label, nc, hist, flag)
    valid = int(((label >= 0) & (label < nc)).sum())
    print(f"nc {nc}: counted {int(hist.sum())} of {valid} valid pixels, flag {int(flag.item())}")
    assert int(flag.item()) == ref_flag == 1
    assert 0 < int(hist.sum()) < valid
    assert torch.equal(hist, ref)
    # without the boosted planes the flag stays down
    flag.zero_()
    step_pair_hist(seg[:, :nc].contiguous()[1:2], label[1:2].contiguous(), nc, hist, flag)
    assert int(flag.item()) == 0


def test_step_pair_hist_refuses_bad_arguments():
    from weclip_vit_comer_amd.validate import step_pair_hist
    seg = torch.zeros(2, 3, 4, 4, device="cuda")
    label = torch.zeros(2, 8, 8, device="cuda", dtype=torch.int64)
    hist = torch.zeros(3, 3, device="cuda", dtype=torch.int64)
    with pytest.raises(RuntimeError, match="batch size"):
        step_pair_hist(seg, label[:1], 3, hist)
    with pytest.raises(RuntimeError, match="num_classes"):
        step_pair_hist(seg, label, 4, hist)                              # a (3, 3) matrix would be written out of bounds
    with pytest.raises(RuntimeError, match="dtype"):
        step_pair_hist(seg, label.int(), 3, hist)
    with pytest.raises(RuntimeError, match="dtype"):
        step_pair_hist(seg.half(), label, 3, hist)
    assert int(hist.sum()) == 0


# ---------------------------------------------------------------------------------------------- fp64 numpy restatement
MARGIN = 1e-4          # fp32 bilinear interpolation of O(10) logits rounds at ~1e-6 .. 1e-5: a larger fp64 top-2 gap cannot flip
FP64_CASES = [(2, 5, (4, 5), (23, 31), 1), (2, 21, (5, 7), (33, 47), 1), (3, 21, (9, 9), (7, 5), 1)]     # B, nc, hw, HW, seed


def _taps(n_out, n_in):
    """ATen's align_corners=False source index with a size-derived scale, in fp64."""
    s = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, s - i0


def fp64_case(B, nc, hw, HW, seed):
    """Seeded inputs and their reference on the host: (seg f32, label, matrix, smallest top-2 margin over the valid pixels)."""
    rng = np.random.RandomState(seed)
    seg = (rng.standard_normal((B, nc, *hw)) * 8.0).astype(np.float32)
    label = rng.randint(0, nc, (B, *HW)).astype(np.int64)
    r = rng.random_sample((B, *HW))
    label[r < 0.1] = 255
    label[(r >= 0.1) & (r < 0.13)] = -1
    y0, y1, ly = _taps(HW[0], hw[0])
    x0, x1, lx = _taps(HW[1], hw[1])
    s = seg.astype(np.float64)
    top = s[:, :, y0][:, :, :, x0] * (1 - lx) + s[:, :, y0][:, :, :, x1] * lx
    bot = s[:, :, y1][:, :, :, x0] * (1 - lx) + s[:, :, y1][:, :, :, x1] * lx
    up = top * (1 - ly)[None, None, :, None] + bot * ly[None, None, :, None]             # (B, nc, H, W)
    srt = np.sort(up, axis=1)
    valid = (label >= 0) & (label < nc)
    margin = float((srt[:, -1] - srt[:, -2])[valid].min())
    hist = np.zeros((nc, nc), np.int64)
    np.add.at(hist, (label[valid], up.argmax(1)[valid]), 1)
    return seg, label, hist, margin


@pytest.mark.parametrize("B,nc,hw,HW,seed", FP64_CASES)
def test_step_pair_hist_equals_fp64_numpy(B, nc, hw, HW, seed):
    """The seeds were chosen on the CPU so that the margin holds at EVERY valid pixel: no pixel is left out of the comparison."""
    from weclip_vit_comer_amd.validate import step_pair_hist
    seg, label, ref, margin = fp64_case(B, nc, hw, HW, seed)
    print(f"B {B} nc {nc} {hw}->{HW} seed {seed}: smallest fp64 top-2 margin over the valid pixels {margin:.3e}")
    assert margin > MARGIN
    hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    step_pair_hist(torch.from_numpy(seg).cuda(), torch.from_numpy(label).cuda(), nc, hist, flag)
    got = hist.cpu().numpy()
    print(f"  cells differing {int((got != ref).sum())}, counted {int(got.sum())} of {int(ref.sum())}")
    assert np.array_equal(got, ref) and int(flag.item()) == 0
