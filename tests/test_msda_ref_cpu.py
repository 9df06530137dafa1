"""The fp64 deformable-attention reference of the kernel tests (tests/msda_ref.py) is the definition, not a restatement of the
kernels' assumptions: it equals a per-sample loop written from the Deformable-DETR formula, and its fused form equals the
composition of WeCLIP_model/comer.py::MSDeformAttn.  CPU only."""
import math

import pytest
import torch

from tests import msda_ref as R

F64 = torch.float64


def _naive(value, shapes, loc, attn):
    """out[n,q,m,d] = sum_l sum_p attn * sum over the four neighbours (x0 + i, y0 + j) of the pixel coordinate
    (loc_x W - 0.5, loc_y H - 0.5) of (1 - |x - px|)(1 - |y - py|) value_l[py, px], zero outside the map."""
    N, S, M, D = value.shape
    _, Lq, _, nL, P, _ = loc.shape
    out = [[[None] * M for _ in range(Lq)] for _ in range(N)]
    pairs = torch.zeros(N, S, M, dtype=F64)
    for n in range(N):
        for q in range(Lq):
            for m in range(M):
                acc = torch.zeros(D, dtype=F64)
                start = 0
                for l, (H, W) in enumerate(shapes):
                    for p in range(P):
                        x = loc[n, q, m, l, p, 0] * W - 0.5
                        y = loc[n, q, m, l, p, 1] * H - 0.5
                        x0, y0 = math.floor(x.item()), math.floor(y.item())
                        for py in (y0, y0 + 1):
                            for px in (x0, x0 + 1):
                                if 0 <= px < W and 0 <= py < H:
                                    w = (1 - (x - px).abs()) * (1 - (y - py).abs())
                                    acc = acc + attn[n, q, m, l, p] * w * value[n, start + py * W + px, m]
                                    if w.item() > 0:
                                        pairs[n, start + py * W + px, m] += 1
                    start += H * W
                out[n][q][m] = acc
    o = torch.stack([torch.stack([torch.cat(out[n][q]) for q in range(Lq)]) for n in range(N)])
    return o, pairs


def _border_case():
    shapes = [(3, 4), (1, 5), (2, 1)]
    N, Lq, M, D, P = 2, 3, 2, 3, 6
    S = sum(h * w for h, w in shapes)
    g = torch.Generator().manual_seed(0)
    value = torch.randn(N, S, M, D, generator=g, dtype=F64)
    loc = torch.rand(N, Lq, M, len(shapes), P, 2, generator=g, dtype=F64) * 1.4 - 0.2
    attn = torch.randn(N, Lq, M, len(shapes), P, generator=g, dtype=F64)
    # pixel coordinates exactly -1 and W / H (excluded), just inside them, at pixel centres and far outside
    for l, (H, W) in enumerate(shapes):
        for c, size in ((0, W), (1, H)):
            px = torch.tensor([-1.0, size, -1 + 1e-6, size - 1e-6, 0.0, size - 1.0, -40.0, 3 * size + 7])
            loc[0, 0, 0, l, :, c] = ((px[:P] + 0.5) / size)
            loc[1, 2, 1, l, :, c] = ((px[2:2 + P] + 0.5) / size)
    return shapes, value, loc, attn


def test_reference_is_the_deformable_detr_formula():
    shapes, value, loc, attn = _border_case()
    vr, lr, ar = [t.clone().requires_grad_(True) for t in (value, loc, attn)]
    out = R.msda_fp64(vr, shapes, lr, ar)
    vn, ln_, an = [t.clone().requires_grad_(True) for t in (value, loc, attn)]
    ref, pairs = _naive(vn, shapes, ln_, an)
    torch.testing.assert_close(out, ref, rtol=1e-13, atol=1e-13)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(1), dtype=F64)
    (out * g).sum().backward()
    (ref * g).sum().backward()
    torch.testing.assert_close(vr.grad, vn.grad, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(ar.grad, an.grad, rtol=1e-13, atol=1e-13)
    # location gradients: equal away from the kinks (d/dx has them where x is an integer, the -1 / size borders included)
    far = R.kink_distance(shapes, loc) > 1e-3
    assert far.float().mean() > 0.5
    torch.testing.assert_close(lr.grad[far], ln_.grad[far], rtol=1e-12, atol=1e-12)
    # error-scale helpers against the same loop
    S = value.shape[1]
    torch.testing.assert_close(R.pair_counts(shapes, loc, S), pairs)
    oa, gaa, gva = R.abs_scales(value, shapes, loc, attn, g)
    va, aa = value.abs().requires_grad_(True), attn.abs().requires_grad_(True)
    ra, _ = _naive(va, shapes, loc, aa)
    ra.backward(g.abs())
    torch.testing.assert_close(oa, ra.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(gaa, aa.grad, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(gva, va.grad, rtol=1e-13, atol=1e-13)
    # |terms| of the location gradient bound the gradient itself
    la = R.loc_grad_abs(value, shapes, loc, attn, g)
    assert (lr.grad.abs()[far] <= la[far] * (1 + 1e-12)).all()


def test_fused_reference_is_the_msdeformattn_composition(monkeypatch):
    from weclip_vit_comer_amd.WeCLIP_model import comer as CM
    from oracle import comer_oracle as CO
    shapes = [(6, 5), (3, 4), (2, 2)]
    N, Lq, C, M, P = 2, 7, 64, 4, 4
    nL = len(shapes)
    S = sum(h * w for h, w in shapes)
    torch.manual_seed(0)
    att = CM.MSDeformAttn(d_model=C, n_levels=nL, n_heads=M, n_points=P).double()
    with torch.no_grad():
        for p in att.parameters():
            p.copy_(torch.randn(p.shape, dtype=F64) * 0.3)
    g = torch.Generator().manual_seed(3)
    query = torch.randn(N, Lq, C, generator=g, dtype=F64)
    feat = torch.randn(N, S, C, generator=g, dtype=F64)
    ref1 = torch.rand(Lq, nL, 2, generator=g, dtype=F64)                  # per-level reference points, the same for every image
    seen = {}

    def core(value, shapes_, loc, attn):
        seen.update(loc=loc, attn=attn)
        return CO.ms_deform_attn(value, shapes_, loc, attn)
    monkeypatch.setattr(CM, "ms_deform_attn_core", core)
    out_mod = att(query, ref1.expand(N, Lq, nL, 2), feat, shapes)
    monkeypatch.undo()

    T = nL * P
    ld = 3 * M * T + 8                                                       # with padding columns
    ow = torch.cat([query @ att.sampling_offsets.weight.t(), query @ att.attention_weights.weight.t(),
                    torch.zeros(N, Lq, ld - 3 * M * T, dtype=F64)], -1).reshape(N * Lq, ld)
    value = (feat @ att.value_proj.weight.t() + att.value_proj.bias).reshape(N, S, M, C // M)
    for nl_ref, r in ((nL, ref1), (1, ref1[:, :1])):
        loc, attn, out = R.msda_fused_fp64(value, shapes, ow, ld, att.sampling_offsets.bias, att.attention_weights.bias, r,
                                           nl_ref, M, P)
        if nl_ref == nL:
            torch.testing.assert_close(loc, seen["loc"], rtol=1e-14, atol=1e-14)
            torch.testing.assert_close(attn, seen["attn"], rtol=1e-14, atol=1e-14)
            torch.testing.assert_close(att.output_proj(out), out_mod, rtol=1e-13, atol=1e-13)
        else:                                                                # one point for all levels: broadcast over nL
            l2, _, _ = R.msda_fused_fp64(value, shapes, ow, ld, att.sampling_offsets.bias, att.attention_weights.bias,
                                         r.expand(Lq, nL, 2).contiguous(), nL, M, P)
            torch.testing.assert_close(loc, l2, rtol=0, atol=0)
    # without biases: the bias folded into ow gives the same
    ow_b = ow.clone()
    ow_b[:, :M * T * 2] += att.sampling_offsets.bias
    ow_b[:, M * T * 2:3 * M * T] += att.attention_weights.bias
    loc_b, attn_b, out_b = R.msda_fused_fp64(value, shapes, ow_b, ld, None, None, ref1, nL, M, P)
    torch.testing.assert_close(loc_b, seen["loc"], rtol=1e-14, atol=1e-14)
    torch.testing.assert_close(attn_b, seen["attn"], rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("size", [1, 5, 128])
def test_kink_distance(size):
    loc = torch.tensor([0.0, 1.0, 0.5, 0.25 + 1e-5, 2.0, -0.5], dtype=F64)
    l6 = torch.stack([loc, loc], -1).reshape(1, 1, 1, 1, -1, 2)
    d = R.kink_distance([(size, size)], l6)[0, 0, 0, 0, :, 0]
    px = loc * size - 0.5
    torch.testing.assert_close(d, (px - px.round()).abs())
    assert d[0] == 0.5 and d[1] == 0.5 and d[4] == 0.5
