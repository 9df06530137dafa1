"""Fused segmentation loss (up-sampling + two CE terms) and the bilinear backward vs torch autograd."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import weclip_oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,nc,h,w,scale", [(2, 21, 4, 6, 16), (1, 5, 7, 5, 16), (2, 21, 32, 32, 16),
                                           (1, 4, 5, 7, 9.5), (1, 3, 12, 10, 1), (1, 40, 4, 6, 16),
                                           # the class chunks of the pixel pass: 81 (COCO, three chunks), 32 (one chunk of 32 at
                                           # its upper edge), 33 (one class in the second chunk), 128 (the class limit)
                                           (1, 81, 5, 3, 16), (1, 32, 4, 6, 16), (2, 33, 3, 5, 9.5), (1, 128, 3, 4, 16)])
def test_fused_seg_loss_forward_backward(B, nc, h, w, scale):
    from weclip_vit_comer_amd.utils.losses import get_seg_loss_fused
    g = torch.Generator().manual_seed(h)
    H, W = int(h * scale), int(w * scale)       # 9.5: non-integer ratio; 1: identity resize
    seg = torch.randn(B, nc, h, w, generator=g)
    lab = torch.randint(0, nc, (B, H, W), generator=g)
    lab[:, : H // 3] = 0
    lab[:, -5:, -7:] = 255
    ref_in = seg.double().requires_grad_(True)
    ref = O.seg_loss(F.interpolate(ref_in, size=(H, W), mode="bilinear", align_corners=False), lab)
    ref.backward()
    x = seg.cuda().requires_grad_(True)
    out = get_seg_loss_fused(x, lab.cuda())
    (3.0 * out).backward()
    assert abs(out.item() - ref.item()) < 2e-5 * max(1.0, abs(ref.item()))
    np.testing.assert_allclose(x.grad.cpu().numpy(), 3.0 * ref_in.grad.numpy(), rtol=2e-3, atol=2e-7)
    # without a gradient request the forward-only kernel runs (with one: loss + gradient in one pixel pass)
    with torch.no_grad():
        out_ng = get_seg_loss_fused(seg.cuda(), lab.cuda())
    assert abs(out_ng.item() - out.item()) < 2e-6 * max(1.0, abs(out.item()))


@pytest.mark.parametrize("align", [False, True])
def test_bilinear_upsample_backward(align):
    from weclip_vit_comer_amd.resize import bilinear_upsample
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 5, 7, generator=g)
    gy = torch.randn(2, 3, 40, 61, generator=g)
    xr = x.double().requires_grad_(True)
    (F.interpolate(xr, size=(40, 61), mode="bilinear", align_corners=align) * gy.double()).sum().backward()
    xc = x.cuda().requires_grad_(True)
    (bilinear_upsample(xc, (40, 61), align) * gy.cuda()).sum().backward()
    np.testing.assert_allclose(xc.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("B,h,w,radius", [(2, 4, 6, 8), (1, 32, 32, 8), (2, 10, 7, 2)])
def test_fused_affinity_loss_forward_backward(B, h, w, radius):
    """label -> affinity label (nearest /16, radius mask, ignore) + get_aff_loss, one pass, vs the oracle."""
    from weclip_vit_comer_amd.utils.losses import get_aff_loss_fused
    g = torch.Generator().manual_seed(h * w)
    H, W = 16 * h, 16 * w
    cam = torch.randint(0, 4, (B, H, W), generator=g)
    cam[:, :, : W // 5] = 255                      # ignored stripe
    ap = torch.rand(B, h * w, h * w, generator=g)
    ref_in = ap.double().requires_grad_(True)
    aff_label = O.cams_to_affinity_label(cam, O.radius_mask(h, w, radius), ignore_index=255)
    ref = O.aff_loss(ref_in, aff_label)
    ref = ref[0] if isinstance(ref, tuple) else ref
    ref.backward()
    x = ap.cuda().requires_grad_(True)
    out = get_aff_loss_fused(x, cam.cuda(), radius=radius, ignore_index=255)
    (0.1 * out).backward()
    assert abs(out.item() - ref.item()) < 1e-5
    np.testing.assert_allclose(x.grad.cpu().numpy(), 0.1 * ref_in.grad.numpy(), rtol=1e-4, atol=1e-10)


def test_fused_seg_loss_is_deterministic_and_refuses_bad_arguments():
    from weclip_vit_comer_amd import _lib as L
    from weclip_vit_comer_amd.utils.losses import get_seg_loss_fused
    g = torch.Generator().manual_seed(4)
    seg = torch.randn(4, 81, 8, 8, generator=g).cuda()
    label = torch.randint(0, 81, (4, 128, 128), generator=g).cuda()
    outs = []
    for _ in range(2):
        x = seg.clone().requires_grad_(True)
        loss = get_seg_loss_fused(x, label, 255)
        loss.backward()
        outs.append((loss.detach().clone(), x.grad.clone()))
    assert torch.isfinite(outs[0][0]).item() and outs[0][1].abs().max().item() > 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # the C entry refuses before launching anything: the output buffers stay as they were
    f32 = torch.float32
    cnt, part, sums = torch.empty(2048, device="cuda"), torch.empty(4096, device="cuda"), torch.full((8,), 7.0, device="cuda")
    tmp, grad = torch.empty(2 * 4 * 129 * 8 * 128, device="cuda"), torch.full((4, 129, 8, 8), 7.0, device="cuda")
    with pytest.raises(RuntimeError, match="bad size"):
        L.lib().wc_seg_loss_fwd_bwd(L.ptr(seg, f32), L.ptr(label, torch.int64), L.ptr(cnt), L.ptr(part), L.ptr(sums), L.ptr(tmp),
                                    L.ptr(grad), 4, 129, 8, 8, 128, 128, 255, L.stream())
    with pytest.raises(RuntimeError, match="null"):
        L.lib().wc_seg_loss_fwd_bwd(L.ptr(seg, f32), None, L.ptr(cnt), L.ptr(part), L.ptr(sums), L.ptr(tmp), L.ptr(grad), 4, 81, 8, 8,
                                    128, 128, 255, L.stream())
    torch.cuda.synchronize()
    assert (sums == 7.0).all().item() and (grad == 7.0).all().item()
