"""The fp64 restatements of tests/comer_ref.py against stock torch in float64 (nn.Conv2d + autograd, F.gelu, F.unfold,
nn.GroupNorm + autograd), and the input conditions that tests/test_comer_kernels_gpu.py relies on: the share of GroupNorm
elements near the ReLU kink, the partial-row counts of the MRFP filter-gradient reduction, the paths its cases reach."""
import math

import pytest
import torch
import torch.nn.functional as Fn

from tests import comer_ref as R
from tests import test_comer_kernels_gpu as K

F64 = torch.float64
TOL = 1e-12


def _close(a, b, tol=TOL):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= tol * max(1.0, b.abs().max().item() if b.numel() else 1.0), err


def _rnd(*shape, seed):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shapes,N,C", [([(5, 13), (3, 7), (1, 9), (2, 3)], 2, 8), ([(1, 1)], 1, 4), ([(4, 6), (2, 2)], 3, 6)])
def test_mrfp_dwconv_matches_conv2d_and_autograd(shapes, N, C):
    h = C // 2
    S = sum(a * b for a, b in shapes)
    x, dy = _rnd(N, S, C, seed=1), _rnd(N, S, C, seed=2)
    w3, b3, w5, b5 = _rnd(h, 9, seed=3), _rnd(h, seed=4), _rnd(h, 25, seed=5), _rnd(h, seed=6)
    alpha = -0.375
    leaves = [t.clone().requires_grad_(True) for t in (x, w3, b3, w5, b5)]
    xl, w3l, b3l, w5l, b5l = leaves
    outs, s = [], 0
    for H, W in shapes:                                                      # the module form: NCHW maps, two grouped Conv2d
        m = xl[:, s:s + H * W].reshape(N, H, W, C).permute(0, 3, 1, 2)
        a = Fn.conv2d(m[:, :h], w3l.reshape(h, 1, 3, 3), b3l, padding=1, groups=h)
        b = Fn.conv2d(m[:, h:], w5l.reshape(h, 1, 5, 5), b5l, padding=2, groups=h)
        outs.append(torch.cat([a, b], 1).permute(0, 2, 3, 1).reshape(N, H * W, C))
        s += H * W
    y_t = torch.cat(outs, 1)
    y_t.backward(dy)
    y, y_abs = R.mrfp_dwconv(x, w3, b3, w5, b5, shapes)
    _close(y, y_t.detach())
    assert (y_abs >= y.abs() - 1e-12).all()
    _close(R.mrfp_dwconv(x.abs(), w3.abs(), b3.abs(), w5.abs(), b5.abs(), shapes)[0], y_abs)
    _close(R.gelu(y), Fn.gelu(y_t.detach()))
    dx, dx_abs = R.mrfp_dwconv_bwd_data(dy, w3, w5, shapes)
    _close(dx, xl.grad)
    assert (dx_abs >= dx.abs() - 1e-12).all()
    grads, grads_abs = R.mrfp_dwconv_bwd_filters(dy, x, shapes, alpha)
    for got, ab, leaf in zip(grads, grads_abs, (w3l, b3l, w5l, b5l)):
        _close(got, alpha * leaf.grad)
        assert (ab >= got.abs() - 1e-12).all()


def test_gelu_matches_torch():
    y = torch.linspace(-9, 9, 1001, dtype=F64)
    _close(R.gelu(y), Fn.gelu(y), 1e-15)


@pytest.mark.parametrize("N,C,H,W,k", [(2, 3, 5, 7, 3), (1, 2, 2, 3, 7), (2, 2, 4, 4, 1), (1, 3, 6, 5, 5)])
def test_dwconv_nchw_matches_conv2d_and_autograd(N, C, H, W, k):
    x, dy, w, b = _rnd(N, C, H, W, seed=1), _rnd(N, C, H, W, seed=2), _rnd(C, k, k, seed=3), _rnd(C, seed=4)
    xl, wl, bl = [t.clone().requires_grad_(True) for t in (x, w, b)]
    y_t = Fn.conv2d(xl, wl.reshape(C, 1, k, k), bl, padding=k // 2, groups=C)
    y_t.backward(dy)
    _close(R.dwconv_fwd(x, w, b)[0], y_t.detach())
    _close(R.dwconv_fwd(x, w, None)[0], y_t.detach() - b.reshape(1, C, 1, 1))
    (dx, dw, db), (dx_a, dw_a, db_a) = R.dwconv_bwd(x, w, dy)
    _close(dx, xl.grad)
    _close(dw, wl.grad)
    _close(db, bl.grad)
    assert (dx_a >= dx.abs() - 1e-12).all() and (dw_a >= dw.abs() - 1e-12).all() and (db_a >= db.abs() - 1e-12).all()


@pytest.mark.parametrize("N,H,W,C,stride,Kp", [(2, 5, 7, 3, 1, 64), (2, 6, 4, 3, 2, 64), (1, 1, 5, 8, 2, 128), (2, 2, 2, 4, 1, 64),
                                               (1, 7, 7, 2, 2, 64)])
def test_im2col_matches_unfold_and_col2im_is_its_adjoint(N, H, W, C, stride, Kp):
    x = _rnd(N, H, W, C, seed=7)
    Ho, Wo = R.out_size(H, stride), R.out_size(W, stride)
    u = Fn.unfold(x.permute(0, 3, 1, 2), 3, padding=1, stride=stride)             # (N, C*9, L), rows c*9 + ky*3 + kx
    assert u.shape[-1] == Ho * Wo
    u = u.reshape(N, C, 9, Ho, Wo).permute(0, 3, 4, 2, 1).reshape(N, Ho, Wo, 9 * C)      # -> (ky*3 + kx)*C + c
    vals = R.im2col3x3_values(x, stride)
    assert torch.equal(vals, u)
    hi, lo = R.im2col3x3(x.float(), stride, Kp)
    assert hi.shape == (N * Ho * Wo, Kp) and (hi[:, 9 * C:] == 0).all() and (lo[:, 9 * C:] == 0).all()
    v32 = R.im2col3x3_values(x.float(), stride).float().reshape(-1, 9 * C)
    assert torch.equal(hi[:, :9 * C], v32.half()) and torch.equal(lo[:, :9 * C], (v32 - v32.half().float()).half())
    assert ((hi.double() + lo.double())[:, :9 * C] - v32.double()).abs().max() <= 2.0 ** -21 * v32.abs().max()
    # <im2col(x), d> == <x, col2im(d)>, with NaN in the padding columns of d
    d = torch.full((N, Ho, Wo, Kp), float("nan"), dtype=F64)
    d[..., :9 * C] = _rnd(N, Ho, Wo, 9 * C, seed=8)
    dx, dx_abs = R.col2im3x3(d, H, W, C, stride)
    lhs, rhs = (vals * d[..., :9 * C]).sum().item(), (x * dx).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * (vals.abs() * d[..., :9 * C].abs()).sum().item()
    xl = x.clone().requires_grad_(True)                                          # and against autograd through unfold
    ul = Fn.unfold(xl.permute(0, 3, 1, 2), 3, padding=1, stride=stride).reshape(N, C, 9, Ho, Wo).permute(0, 3, 4, 2, 1)
    ul.reshape(N, Ho, Wo, 9 * C).backward(d[..., :9 * C])
    _close(dx, xl.grad)
    assert (dx_abs >= dx.abs() - 1e-12).all()


@pytest.mark.parametrize("N,HW,C,G", [(2, 7, 8, 2), (1, 1, 16, 4), (3, 33, 12, 3)])
def test_groupnorm_relu_matches_torch_through_a_fixed_mask(N, HW, C, G):
    eps = K.EPS
    x, dy = _rnd(N, HW, C, seed=11) + 0.7, _rnd(N, HW, C, seed=12)
    gamma, beta = _rnd(C, seed=13), _rnd(C, seed=14)
    gn = torch.nn.GroupNorm(G, C, eps=eps).double()
    with torch.no_grad():
        gn.weight.copy_(gamma)
        gn.bias.copy_(beta)
    xl = x.clone().requires_grad_(True)
    pre_t = gn(xl.permute(0, 2, 1)).permute(0, 2, 1)                             # (N, C, HW) -> rows
    mean, rstd, m1, m2 = R.gn_stats(x, G, eps)
    xg = x.reshape(N, HW, G, C // G)
    _close(mean, xg.mean((1, 3)))
    _close(rstd, 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False) + eps))
    _close(m1, xg.abs().mean((1, 3)))
    _close(m2, (xg ** 2).mean((1, 3)))
    pre, pre_abs = R.gn_relu_pre(x, mean, rstd, gamma, beta)
    _close(pre, pre_t.detach())
    assert (pre_abs >= pre.abs() - 1e-12).all()
    mask = torch.rand(N, HW, C, generator=torch.Generator().manual_seed(15)) < 0.6      # fixed, independent of the sign of pre
    (pre_t * mask).backward(dy)
    (dx, dg, db), (dx_a, dg_a, db_a) = R.gn_relu_bwd(x, mean, rstd, gamma, dy, mask, G)
    _close(dx, xl.grad, 1e-11)
    _close(dg, gn.weight.grad)
    _close(db, gn.bias.grad)
    assert (dx_a >= dx.abs() - 1e-12).all() and (dg_a >= dg.abs() - 1e-12).all() and (db_a >= db.abs() - 1e-12).all()
    # the mask that ReLU itself gives
    xl.grad = None
    gn.zero_grad()
    torch.relu(gn(xl.permute(0, 2, 1)).permute(0, 2, 1)).backward(dy)
    (dx, dg, db), _ = R.gn_relu_bwd(x, mean, rstd, gamma, dy, pre > 0, G)
    _close(dx, xl.grad, 1e-11)
    _close(dg, gn.weight.grad)


def test_glue_restatements():
    C, Kk = 5, 9
    G, Wop, s, gamma, bop = _rnd(C, Kk, seed=1), _rnd(C, Kk, seed=2), _rnd(C, seed=3), _rnd(C, seed=4), _rnd(C, seed=5)
    # v1 = v + gamma * (o1 Wop^T + bop) through autograd, with G = dv1^T o1 and s = dv1^T 1
    o1, dv1 = _rnd(11, Kk, seed=6), _rnd(11, C, seed=7)
    gl, Wl, bl = [t.clone().requires_grad_(True) for t in (gamma, Wop, bop)]
    (gl * (o1 @ Wl.t() + bl)).backward(dv1)
    (dW, dbop, dgam), _ = R.cti_gate_grads(dv1.t() @ o1, dv1.sum(0), gamma, Wop, bop)
    _close(dW, Wl.grad)
    _close(dbop, bl.grad)
    _close(dgam, gl.grad)
    # strided rows
    B, Rr, Cc, lds, ss, ldd, sd = 3, 5, 7, 9, 48, 11, 57
    src = _rnd(K._span(B, Rr, Cc, lds, ss), seed=8)
    dst = torch.full((K._span(B, Rr, Cc, ldd, sd),), -7.0, dtype=F64)
    out = R.rows_copy(src, dst, B, Rr, Cc, lds, ss, ldd, sd)
    want = dst.clone()
    for b in range(B):
        want[b * sd:b * sd + Rr * ldd + Cc - ldd].as_strided((Rr, Cc), (ldd, 1)).copy_(
            src[b * ss:].as_strided((Rr, Cc), (lds, 1)))
    assert torch.equal(out, want) and int((out == -7.0).sum()) == dst.numel() - B * Rr * Cc
    sdd = Rr * Cc + 5
    acc = _rnd(K._span(B, Rr, Cc, Cc, sdd), seed=9)
    got, got_abs = R.rows_add(src, acc, B, Rr, Cc, lds, ss, sdd, -1.75)
    want = acc.clone()
    for b in range(B):
        want[b * sdd:b * sdd + Rr * Cc] += -1.75 * src[b * ss:].as_strided((Rr, Cc), (lds, 1)).reshape(-1)
    _close(got, want)
    assert (got_abs >= got.abs() - 1e-12).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the conditions the GPU tests rely on

def test_groupnorm_cases_stay_under_the_relu_kink_cap():
    kinds = set()
    for Cc, G, HW, N, kind in K.gn_cases():
        x, gamma, beta, dy = K.gn_inputs(Cc, G, HW, N, kind)
        ref = K.GNRef(x, gamma, beta, G, exact_groups=(1,) if kind == "const" else ())
        assert ref.near_share <= K.KINK_CAP, (Cc, G, HW, N, kind, ref.near_share)
        assert 0.05 < (ref.pre > 0).double().mean() < 0.95                      # both sides of the ReLU are exercised
        kinds.add(kind)
        if kind == "shifted":
            assert ((ref.mean * ref.rstd).abs() > 3.5).all()
        if kind == "const":
            assert abs(ref.rstd[0, 1].item() - 1.0 / math.sqrt(K.EPS)) < 1e-9
    assert kinds == {"plain", "shifted", "const"}
    cfgs = {(c[0], c[1], c[2]) for c in K.gn_cases()}
    assert all((Cc, G, HW) in cfgs for Cc, G in K.GN_CFG for HW in K.GN_HW)
    assert all({c[3] for c in K.gn_cases() if c[0] == Cc} == {1, 3} for Cc, _ in K.GN_CFG)


def test_mrfp_cases_reach_every_path():
    cases = K.mrfp_cases()
    assert {(c[0], c[1], c[2]) for c in cases} == {(Cc, N, n) for Cc in (64, 128, 256) for N in (1, 3) for n in K.LEVELS}
    for Cc in (64, 128, 256):
        mine = [c for c in cases if c[0] == Cc]
        assert {c[4] for c in mine} == {0, 1}                                    # dy as f32 and as f16
        assert {c[3] for c in mine} == {("y", "g16"), ("g16",), ("y",)}
        assert {c[5] for c in mine} == {("dx32", "dx16"), ("dx16",), ("dx32",)}
    assert all(c[6] != 1.0 for c in cases)
    assert len(K.LEVELS["eight"]) == 8
    # a strip count that is no multiple of 256 / C nor of 4 * (256 / C): workgroups straddle a level boundary, the last is ragged
    _, strips = R.mrfp_parts(K.LEVELS["ragged"], 1, 64)
    assert strips == 17 and all(strips % (256 // Cc) and strips % (4 * (256 // Cc)) for Cc in (64, 128))
    assert any(W % 8 for _, W in K.LEVELS["ragged"]) and any(H < 5 and W < 5 for H, W in K.LEVELS["ragged"])
    Cc, N, shapes = K.BIG
    assert R.mrfp_parts(shapes, N, Cc) == (130, 102)
    for name, shapes in K.LEVELS.items():
        for Cc in (64, 128, 256):
            assert K.mrfp_wgrad_depth(shapes, 3, Cc) <= K.C64
    assert K.mrfp_wgrad_depth(K.BIG[2], K.BIG[1], K.BIG[0]) <= K.C64
