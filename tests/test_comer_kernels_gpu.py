"""Every kernel path of the ViT-CoMer insert kernels outside deformable attention -- the MRFP depth-wise convolutions and the
glue kernels of csrc/comer.hip, the gathers and GroupNorm + ReLU of csrc/convstem.hip, csrc/dwconv.hip -- against the fp64
restatements of tests/comer_ref.py, through the C ABI the way the engine calls it.

Every output and workspace is filled with 0xFF bytes (NaN) before a call: an output element the kernels leave unwritten fails,
and so does a write into a gap between destination rows.  Bounds follow the error model of tests/test_msda_kernels_gpu.py, per
element:
  fp32 arithmetic   |got - ref| <= c 2^-24 sum|terms| with c = 64 (sum|terms|: the same evaluation on absolute values);
  fp16 inputs       the reference's inputs are rounded to fp16 first; fp16 outputs: one fp16 ulp of the reference on top;
  gathers           im2col hi / lo and rows_copy are compared bit for bit;
  reductions        c = the number of roundings on the longest path through the summation (each rounding contributes at most
                    2^-24 sum|terms|) where that exceeds 64: the GroupNorm sums (see gn_depth) -- the MRFP filter gradients,
                    dwconv's filter gradients and cti_gate_grads stay below 64, which the tests assert from the shapes.
`_check` prints the worst err / bound of every comparison (pytest -rP shows them)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import comer_ref as R

pytestmark = pytest.mark.gpu

F32, F16, F64 = torch.float32, torch.float16, torch.float64
U = R.U
C64 = 64                      # the c of the fp32 bound
EPS = float(np.float32(1e-5))  # GroupNorm's eps as the kernels receive it


def _L():
    from weclip_vit_comer_amd import _lib as L
    return L


def _nan(n, dtype, skew=0):
    """Device buffer of n elements with every byte 0xFF (NaN for f32 / f16); skew: start that many 4-byte words past a 16-byte
    boundary."""
    extra = skew * 4 // torch.tensor([], dtype=dtype).element_size()
    t = torch.empty(n + extra, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(255)
    return t[extra:]


def _dev(x, dtype, skew=0):
    t = _nan(x.numel(), dtype, skew)
    t.copy_(x.reshape(-1).to(dtype).cuda())
    return t


def _ptr(t):
    return _L().ptr(t)


def _hs(shapes):
    return _L().int_array([v for hw in shapes for v in hw])


def _ulp16(r):
    a = r.abs().clamp(min=2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def _check(name, got, ref, bound):
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} elements not written (still NaN)"
    err = (got - ref).abs()
    bound = bound.expand_as(err)
    ratio = (err / bound.clamp(min=1e-300)).max().item() if err.numel() else 0.0
    print(f"[err/bound] {name}: {ratio:.3g}")
    bad = err > bound
    if bad.any():
        i = int(torch.argmax((err - bound).reshape(-1)))
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst err / bound "
                             f"{ratio:.3g}; e.g. element {idx}: got {got.reshape(-1)[i]:.9g} ref {ref.reshape(-1)[i]:.9g}")


def _untouched(name, t):
    assert (t.view(torch.uint8) == 255).all(), f"{name} was written by a call that was refused"


def _refused(call, *buffers):
    """An argument error: the call returns WC_ERR_ARG (1) and launches nothing."""
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=r"\(code 1\)"):
        call()
    torch.cuda.synchronize()
    for i, t in enumerate(buffers):
        _untouched(f"output {i}", t)


# ---------------------------------------------------------------------------------------------------------------------------
# MRFP depth-wise convolutions (csrc/comer.hip)

LEVELS = {
    "pyr": [(16, 16), (8, 8), (4, 4)],                      # production-like: every W a multiple of 8 or below it
    "ragged": [(5, 13), (3, 7), (1, 9), (2, 3)],            # strip tails, one-strip rows, H = 1, a map smaller than the 5x5 window
    "one": [(1, 1)],
    "eight": [(6, 5), (1, 1), (1, 9), (7, 1), (4, 4), (3, 8), (2, 2), (5, 3)],
}
# (C, N, levels) of the reduction case: 102 strips, 26 chunks of 4 strips per image, 130 partial rows (> 128, not a multiple of
# 16: the unrolled 8 x 16 loop and the tail of mrfp_dwconv_bwd_w_final_kernel both run)
BIG = (256, 5, [(24, 20), (12, 10), (6, 5)])
_FWD_OUTS = [("y", "g16"), ("g16",), ("y",)]
_DX_OUTS = [("dx32", "dx16"), ("dx16",), ("dx32",)]
_ALPHAS = [0.375, 2.5, -0.0625]                              # (exact in fp32)


def mrfp_cases():
    """(C, N, levels, forward outputs, dy is f16, dx outputs, alpha): every C x N x level list; the options cycle so that every C
    meets every one of them (tests/test_comer_ref_cpu.py checks that)."""
    cases = []
    for ci, Cc in enumerate((64, 128, 256)):
        for li, name in enumerate(("pyr", "ragged", "one", "eight")):
            for ni, N in enumerate((1, 3)):
                j = li * 2 + ni
                cases.append((Cc, N, name, _FWD_OUTS[(j + ci) % 3], (j + j // 2) % 2, _DX_OUTS[(2 * j + ci) % 3], _ALPHAS[j % 3]))
    return cases


def mrfp_wgrad_depth(shapes, N, Cc):
    """Roundings on the longest path of a filter / bias gradient sum: the 8 pixels of each of a lane's 4 strips one after the
    other (the bias sum; a tap takes 8 + 4), the 256 / C lanes, ceil(rows / 128) + 1 partial rows per accumulator, the 8
    accumulators (3), the 16 groups, alpha."""
    parts, _ = R.mrfp_parts(shapes, N, Cc)
    return 8 * 4 + 256 // Cc + (parts + 127) // 128 + 1 + 3 + 16 + 1


def _mrfp_inputs(shapes, N, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in shapes)
    h = Cc // 2
    x, dy = torch.randn(N, S, Cc, generator=g), torch.randn(N, S, Cc, generator=g)
    w3, w5 = torch.randn(h, 9, generator=g) * 0.3, torch.randn(h, 25, generator=g) * 0.2       # every tap its own value
    b3, b5 = torch.randn(h, generator=g), torch.randn(h, generator=g)
    return x, dy, w3, b3, w5, b5


def _mrfp_fwd(x, w3, b3, w5, b5, shapes, outs):
    L = _L()
    N, S, Cc = x.shape
    xd, w3d, b3d, w5d, b5d = [_dev(t, F32) for t in (x, w3, b3, w5, b5)]
    y = _nan(x.numel(), F32) if "y" in outs else None
    g16 = _nan(x.numel(), F16) if "g16" in outs else None
    L.lib().wc_mrfp_dwconv_fwd(_ptr(xd), _ptr(w3d), _ptr(b3d), _ptr(w5d), _ptr(b5d), _ptr(y), _ptr(g16), _hs(shapes), len(shapes),
                               N, Cc, L.stream())
    torch.cuda.synchronize()
    return y, g16


def _mrfp_parts(shapes, N, Cc):
    n = ctypes.c_long(-1)
    _L().lib().wc_mrfp_dwconv_parts(_hs(shapes), len(shapes), N, Cc, ctypes.byref(n))
    return n.value


def _mrfp_bwd(dy, dy16, x, w3, w5, shapes, outs, alpha):
    L = _L()
    N, S, Cc = x.shape
    h = Cc // 2
    dyd = _dev(dy, F16 if dy16 else F32)
    xd, w3d, w5d = [_dev(t, F32) for t in (x, w3, w5)]
    dx32 = _nan(x.numel(), F32) if "dx32" in outs else None
    dx16 = _nan(x.numel(), F16) if "dx16" in outs else None
    dw3, db3, dw5, db5 = _nan(h * 9, F32), _nan(h, F32), _nan(h * 25, F32), _nan(h, F32)
    part = _nan(_mrfp_parts(shapes, N, Cc) * Cc * 26, F32)
    L.lib().wc_mrfp_dwconv_bwd(_ptr(dyd), int(dy16), _ptr(xd), _ptr(w3d), _ptr(w5d), _ptr(dx32), _ptr(dx16), _ptr(dw3), _ptr(db3),
                               _ptr(dw5), _ptr(db5), _ptr(part), alpha, _hs(shapes), len(shapes), N, Cc, L.stream())
    torch.cuda.synchronize()
    return dx32, dx16, (dw3, db3, dw5, db5)


def _run_mrfp(Cc, N, shapes, fwd_outs, dy16, dx_outs, alpha, seed):
    tag = f"mrfp C{Cc} N{N} {len(shapes)} levels"
    x, dy, w3, b3, w5, b5 = _mrfp_inputs(shapes, N, Cc, seed)
    parts, strips = R.mrfp_parts(shapes, N, Cc)
    assert _mrfp_parts(shapes, N, Cc) == parts, "wc_mrfp_dwconv_parts disagrees with N * ceil(strips / (4 * 256 / C))"
    # forward
    y_ref, y_abs = R.mrfp_dwconv(x, w3, b3, w5, b5, shapes)
    y, g16 = _mrfp_fwd(x, w3, b3, w5, b5, shapes, fwd_outs)
    if y is not None:
        _check(f"{tag} y", y, y_ref, C64 * U * y_abs)
    if g16 is not None:
        # |d gelu / dy| <= 1.13 carries y's bound over; the erfc polynomial of the kernel (Abramowitz-Stegun 7.1.26, 1.5e-7 on
        # erf = 1.3 2^-24 on Phi) and its fast exp / reciprocal are a few 2^-24 |y| <= 2^-24 y_abs, inside the same c
        _check(f"{tag} g16", g16, R.gelu(y_ref), C64 * U * 1.13 * y_abs + _ulp16(R.gelu(y_ref)))
    # backward
    dyr = dy.half().float() if dy16 else dy
    dx_ref, dx_abs = R.mrfp_dwconv_bwd_data(dyr, w3, w5, shapes)
    dx32, dx16, grads = _mrfp_bwd(dy, dy16, x, w3, w5, shapes, dx_outs, alpha)
    if dx32 is not None:
        _check(f"{tag} dx32 (dy {'f16' if dy16 else 'f32'})", dx32, dx_ref, C64 * U * dx_abs)
    if dx16 is not None:
        _check(f"{tag} dx16 (dy {'f16' if dy16 else 'f32'})", dx16, dx_ref, C64 * U * dx_abs + _ulp16(dx_ref))
    if dx32 is not None and dx16 is not None:
        assert torch.equal(dx16, dx32.half()), f"{tag}: dx16 is not dx32 rounded to fp16"
    assert mrfp_wgrad_depth(shapes, N, Cc) <= C64
    refs, refs_abs = R.mrfp_dwconv_bwd_filters(dyr, x, shapes, alpha)
    for name, got, ref, ab in zip(("dw3", "db3", "dw5", "db5"), grads, refs, refs_abs):
        _check(f"{tag} {name}", got, ref, C64 * U * ab)
    # the summation order is fixed: a second run gives the same bits
    _, _, again = _mrfp_bwd(dy, dy16, x, w3, w5, shapes, dx_outs, alpha)
    for name, a, b in zip(("dw3", "db3", "dw5", "db5"), grads, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{tag}: {name} differs between two runs"
    return strips, parts


@pytest.mark.parametrize("case", mrfp_cases(), ids=lambda c: "C{}-N{}-{}-{}-dy{}-{}".format(c[0], c[1], c[2], "+".join(c[3]),
                                                                                             "16" if c[4] else "32", "+".join(c[5])))
def test_mrfp_dwconv(case):
    Cc, N, name, fwd_outs, dy16, dx_outs, alpha = case
    _run_mrfp(Cc, N, LEVELS[name], fwd_outs, dy16, dx_outs, alpha, seed=Cc + N + len(name))


def test_mrfp_dwconv_reduction_of_130_partial_rows():
    Cc, N, shapes = BIG
    strips, parts = _run_mrfp(Cc, N, shapes, ("y", "g16"), 1, ("dx16",), 0.375, seed=5)
    assert (strips, parts) == (102, 130) and parts > 128 and parts % 16 != 0
    assert _mrfp_parts(shapes, N, Cc) == 130


# ---------------------------------------------------------------------------------------------------------------------------
# conv-stem gathers (csrc/convstem.hip)

_SIZES = [(17, 23), (16, 16), (1, 5), (2, 2)]


def _kp(Cc):
    return (9 * Cc + 63) // 64 * 64


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cc", [3, 8, 64])            # scalar path with K = 27 inside Kp = 64; smallest vector path; Kp = 9C
def test_im2col_bits(Cc, stride):
    L = _L()
    N, Kp = 2, _kp(Cc)
    assert (Cc, Kp) in ((3, 64), (8, 128), (64, 576))
    g = torch.Generator().manual_seed(Cc + stride)
    for H, W in _SIZES:
        x = torch.randn(N, H, W, Cc, generator=g) * torch.exp2(torch.randint(-12, 6, (N, H, W, Cc), generator=g).float())
        hi_ref, lo_ref = R.im2col3x3(x, stride, Kp)
        xd = _dev(x, F32)
        for with_lo in (True, False):
            hi = _nan(hi_ref.numel(), F16)
            lo = _nan(hi_ref.numel(), F16) if with_lo else None
            L.lib().wc_im2col3x3(_ptr(xd), _ptr(hi), _ptr(lo), N, H, W, Cc, stride, Kp, L.stream())
            torch.cuda.synchronize()
            tag = f"im2col C{Cc} s{stride} {H}x{W} lo={with_lo}"
            assert torch.equal(hi.cpu().view(torch.int16), hi_ref.reshape(-1).view(torch.int16)), f"{tag}: hi differs"
            if with_lo:
                assert torch.equal(lo.cpu().view(torch.int16), lo_ref.reshape(-1).view(torch.int16)), f"{tag}: lo differs"
    assert lo_ref.abs().max() > 0


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cc,skew", [(32, 0), (3, 0), (32, 1)])      # 4-wide; 1-wide; 1-wide because dx is off 16-byte alignment
def test_col2im(Cc, skew, stride):
    L = _L()
    N, Kp = 2, _kp(Cc)
    g = torch.Generator().manual_seed(10 * Cc + stride + skew)
    for H, W in [(6, 8), (7, 5), (1, 5), (2, 2), (9, 4)]:      # (even sizes under stride 2: border pixels with fewer taps)
        Ho, Wo = R.out_size(H, stride), R.out_size(W, stride)
        dcols = torch.full((N, Ho, Wo, Kp), float("nan"))     # the padding columns must not be read
        dcols[..., :9 * Cc] = torch.randn(N, Ho, Wo, 9 * Cc, generator=g)
        ref, ref_abs = R.col2im3x3(dcols, H, W, Cc, stride)
        dd = _dev(dcols, F32)
        dx = _nan(N * H * W * Cc, F32, skew)
        L.lib().wc_col2im3x3(_ptr(dd), _ptr(dx), N, H, W, Cc, stride, Kp, L.stream())
        torch.cuda.synchronize()
        _check(f"col2im C{Cc} skew{skew} s{stride} {H}x{W}", dx, ref, C64 * U * ref_abs)


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm + ReLU (csrc/convstem.hip)

GN_CFG = [(16, 4), (32, 8), (64, 8), (128, 8), (256, 8)]
GN_HW = [1, 63, 256, 257, 1000]
KINK_CAP = 1e-3                # share of the elements whose ReLU side may be left to the kernel


def gn_depth(Cc, HW):
    """Roundings on the longest path of a channel's partial sum over a block of 256 rows: a thread owns four channels of every
    (1024 / C)-th row, so ceil(rows / (1024 / C)) sequential additions, then the 1024 / C row lanes in LDS.  (The blocks are
    then added in fp64 in the forward.)"""
    nrl = 1024 // Cc
    return -(-min(HW, 256) // nrl) + nrl


def gn_cases():
    """(C, G, HW, N, kind): every (C, G) with every HW, N alternating; one case with the group means 4 standard deviations from
    0 (the variance is E[x^2] - mean^2 from fp32 partial sums) and one with a group held constant (variance 0)."""
    cases = [(Cc, G, HW, 3 if (i + j) % 2 else 1, "plain") for i, (Cc, G) in enumerate(GN_CFG) for j, HW in enumerate(GN_HW)]
    return cases + [(64, 8, 1000, 3, "shifted"), (32, 8, 257, 1, "shifted"), (64, 8, 257, 3, "const"), (16, 4, 63, 1, "const")]


def gn_inputs(Cc, G, HW, N, kind, seed=0):
    g = torch.Generator().manual_seed(seed + Cc + HW + N)
    x = torch.randn(N, HW, Cc, generator=g)
    if kind == "shifted":
        sign = torch.where(torch.arange(G) % 2 == 0, 1.0, -1.0).repeat_interleave(Cc // G)
        x = x + 4.0 * sign
    if kind == "const":
        x[:, :, Cc // G:2 * (Cc // G)] = 0.5          # group 1 (0.5 and 0.25: every partial sum is exact in fp32)
    gamma = (0.5 + torch.rand(Cc, generator=g)) * torch.where(torch.rand(Cc, generator=g) < 0.25, -1.0, 1.0)
    beta = (0.25 + 0.5 * torch.rand(Cc, generator=g)) * torch.where(torch.rand(Cc, generator=g) < 0.5, -1.0, 1.0)
    dy = torch.randn(N, HW, Cc, generator=g)
    return x, gamma, beta, dy


class GNRef:
    """fp64 statistics and pre-activation of a case, and their bounds.  With d = gn_depth and m1 = E|x|, m2 = E[x^2] of a group
    (count = HW * C / G values; the C / G channel sums of a group are added after the rows):
      mean  : (d + C/G) additions and the final rounding        ->  mean_b = (d + C/G + 1) U m1
      E[x^2]: one product more                                  ->  (d + C/G + 2) U m2
      var   = E[x^2] - mean^2                                   ->  var_b  = (d + C/G + 2) U m2 + 2 |mean| mean_b + mean_b^2
      rstd  = (var + eps)^-1/2: its change over [var - var_b, var + var_b] (no linearisation: var_b may exceed var + eps when
              the variance is 0), one rounding on top.
    A group held constant at a value whose sums are exact in fp32 leaves only the final roundings: 2 U |mean|, 2 U rstd.
      pre = (x - mean) rstd gamma + beta with the kernel's own statistics:
              |gamma| (rstd mean_b + |x - mean| rstd_b + mean_b rstd_b) + c U pre_abs, c = 64."""

    def __init__(self, x, gamma, beta, G, exact_groups=()):
        N, HW, Cc = x.shape
        Cg = Cc // G
        self.mean, self.rstd, m1, m2 = R.gn_stats(x, G, EPS)
        c = gn_depth(Cc, HW) + Cg
        self.mean_b = (c + 1) * U * m1
        var = 1.0 / self.rstd ** 2 - EPS
        var_b = (c + 2) * U * m2 + 2 * self.mean.abs() * self.mean_b + self.mean_b ** 2
        f = lambda v: 1.0 / torch.sqrt(v.clamp(min=0.0) + EPS)
        self.rstd_b = torch.maximum((f(var + var_b) - self.rstd).abs(), (f(var - var_b) - self.rstd).abs()) + U * self.rstd
        for gi in exact_groups:
            self.mean_b[:, gi] = 2 * U * self.mean[:, gi].abs()
            self.rstd_b[:, gi] = 2 * U * self.rstd[:, gi]
        self.pre, pre_abs = R.gn_relu_pre(x, self.mean, self.rstd, gamma, beta)
        mb, rb, r = [R._per_channel(t, Cc) for t in (self.mean_b, self.rstd_b, self.rstd)]
        xm = (x.double() - R._per_channel(self.mean, Cc)).abs()
        self.pre_b = gamma.double().abs() * (r * mb + xm * rb + mb * rb) + C64 * U * pre_abs
        self.near = self.pre.abs() <= self.pre_b           # the reference cannot tell the side of the ReLU there
        self.near_share = self.near.double().mean().item()


def _gn_run(x, gamma, beta, dy, G):
    L = _L()
    N, HW, Cc = x.shape
    nb = -(-HW // 64)                                   # (the header's workspace sizes)
    xd, gd, bd, dyd = [_dev(t, F32) for t in (x, gamma, beta, dy)]
    y, stats, part = _nan(x.numel(), F32), _nan(N * G * 2, F32), _nan(N * nb * G * 2, F32)
    L.lib().wc_groupnorm_relu_fwd(_ptr(xd), _ptr(gd), _ptr(bd), _ptr(y), _ptr(stats), _ptr(part), N, HW, Cc, G, EPS, L.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and torch.isfinite(y).all(), "GroupNorm forward left NaN in stats or y"
    dx, dgamma, dbeta = _nan(x.numel(), F32), _nan(Cc, F32), _nan(Cc, F32)
    gpart, cpart, gsum = _nan(N * nb * G * 2, F32), _nan(N * nb * Cc * 2, F32), _nan(N * G * 2, F32)
    L.lib().wc_groupnorm_relu_bwd(_ptr(xd), _ptr(y), _ptr(dyd), _ptr(stats), _ptr(gd), _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                  _ptr(gpart), _ptr(cpart), _ptr(gsum), N, HW, Cc, G, L.stream())
    torch.cuda.synchronize()
    return y, stats, dx, dgamma, dbeta


@pytest.mark.parametrize("case", gn_cases(), ids=lambda c: "C{}-G{}-HW{}-N{}-{}".format(*c))
def test_groupnorm_relu(case):
    """Forward against the reference from x alone.  Backward with the statistics and y of the forward as its inputs, as in the
    engine: the reference takes the same fp32 statistics, and the kernel's ReLU mask only where the reference's own
    pre-activation is within its bound of 0 (at most 1 element in 1000; elsewhere the masks must agree).
    Bounds of the backward, c = roundings on the longest path (nb = N * ceil(HW / 256) block partials, one per thread, then a
    wave reduction of 6 and the 4 waves):
      dgamma, dbeta : 3 (d xhat) + gn_depth + 1 + 10;   group sums: + gamma + C/G;   dx: + 8 for its own arithmetic."""
    Cc, G, HW, N, kind = case
    tag = "gn C{} G{} HW{} N{} {}".format(*case)
    x, gamma, beta, dy = gn_inputs(Cc, G, HW, N, kind)
    ref = GNRef(x, gamma, beta, G, exact_groups=(1,) if kind == "const" else ())
    assert ref.near_share <= KINK_CAP
    y, stats, dx, dgamma, dbeta = _gn_run(x, gamma, beta, dy, G)
    st = stats.cpu().double().reshape(N, G, 2)
    _check(f"{tag} mean", st[..., 0], ref.mean, ref.mean_b)
    _check(f"{tag} rstd", st[..., 1], ref.rstd, ref.rstd_b)
    if kind == "const":
        assert abs(ref.rstd[0, 1].item() - 1.0 / math.sqrt(EPS)) < 1e-9 and (ref.mean[:, 1] == 0.5).all()
    if kind == "shifted":
        assert ((ref.mean * ref.rstd).abs() > 3.5).all()
    _check(f"{tag} y", y, ref.pre.clamp(min=0.0), ref.pre_b)              # (ReLU is 1-Lipschitz: no exception at the kink)
    mask_k = (y.cpu().reshape(x.shape) > 0)
    mask_r = ref.pre > 0
    assert (mask_k == mask_r)[~ref.near].all(), f"{tag}: ReLU mask differs where the pre-activation is outside its bound of 0"
    mask = torch.where(ref.near, mask_k, mask_r)
    (dx_r, dg_r, db_r), (dx_a, dg_a, db_a) = R.gn_relu_bwd(x, st[..., 0], st[..., 1], gamma, dy, mask, G)
    c_ch = 3 + gn_depth(Cc, HW) + 1 + 10
    c_dx = c_ch + 1 + Cc // G + 8
    _check(f"{tag} dgamma", dgamma, dg_r, max(C64, c_ch) * U * dg_a)
    _check(f"{tag} dbeta", dbeta, db_r, max(C64, c_ch) * U * db_a)
    _check(f"{tag} dx", dx, dx_r, max(C64, c_dx) * U * dx_a)


# ---------------------------------------------------------------------------------------------------------------------------
# NCHW depth-wise convolution (csrc/dwconv.hip)

@pytest.mark.parametrize("N,Cc,H,W,k", [(2, 3, 7, 70, 3), (1, 2, 5, 6, 1), (2, 3, 2, 3, 7), (1, 2, 9, 11, 5), (3, 4, 6, 70, 7)],
                         ids=lambda v: str(v))
def test_dwconv_nchw(N, Cc, H, W, k):
    """W = 70: two column blocks, H no multiple of the 4 rows of a block; k = 1; k = 7 on a map smaller than the filter.  The
    filter gradient: ceil(HW / 256) products per thread, 10 for the block reduction, N images -- below c = 64 (asserted)."""
    L = _L()
    g = torch.Generator().manual_seed(N + Cc + H + W + k)
    x, dy = torch.randn(N, Cc, H, W, generator=g), torch.randn(N, Cc, H, W, generator=g)
    w, b = torch.randn(Cc, k, k, generator=g), torch.randn(Cc, generator=g)
    tag = f"dwconv N{N} C{Cc} {H}x{W} k{k}"
    xd, wd, bd, dyd = [_dev(t, F32) for t in (x, w, b, dy)]
    for bias in (b, None):
        ref, ref_abs = R.dwconv_fwd(x, w, bias)
        y = _nan(x.numel(), F32)
        L.lib().wc_dwconv_fwd(_ptr(xd), _ptr(wd), _ptr(bd) if bias is not None else None, _ptr(y), N, Cc, H, W, k, L.stream())
        torch.cuda.synchronize()
        _check(f"{tag} y bias={bias is not None}", y, ref, C64 * U * ref_abs)
    assert -(-H * W // 256) + 1 + 10 + N <= C64
    (dx_r, dw_r, db_r), (dx_a, dw_a, db_a) = R.dwconv_bwd(x, w, dy)
    for with_db in (True, False):
        dx, dw, db = _nan(x.numel(), F32), _nan(w.numel(), F32), _nan(Cc, F32)
        part = _nan(N * Cc * (k * k + 1), F32)
        L.lib().wc_dwconv_bwd(_ptr(xd), _ptr(wd), _ptr(dyd), _ptr(dx), _ptr(dw), _ptr(db) if with_db else None, _ptr(part),
                              N, Cc, H, W, k, L.stream())
        torch.cuda.synchronize()
        _check(f"{tag} dx db={with_db}", dx, dx_r, C64 * U * dx_a)
        _check(f"{tag} dw db={with_db}", dw, dw_r, C64 * U * dw_a)
        if with_db:
            _check(f"{tag} db", db, db_r, C64 * U * db_a)
        else:
            _untouched("db", db)


# ---------------------------------------------------------------------------------------------------------------------------
# glue (csrc/comer.hip)

@pytest.mark.parametrize("Cc,K", [(5, 300), (3, 1), (8, 256)])
def test_cti_gate_grads(Cc, K):
    """rowsum over K: ceil(K / 256) products per thread + the block reduction (10) + bop * s: below c = 64."""
    L = _L()
    g = torch.Generator().manual_seed(Cc * K)
    G, Wop = torch.randn(Cc, K, generator=g), torch.randn(Cc, K, generator=g)
    s, gamma, bop = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    refs, refs_abs = R.cti_gate_grads(G, s, gamma, Wop, bop)
    ins = [_dev(t, F32) for t in (G, s, gamma, Wop, bop)]
    outs = [_nan(Cc * K, F32), _nan(Cc, F32), _nan(Cc, F32)]
    L.lib().wc_cti_gate_grads(*[_ptr(t) for t in ins + outs], Cc, K, L.stream())
    torch.cuda.synchronize()
    assert -(-K // 256) + 1 + 10 + 2 <= C64
    for name, got, ref, ab in zip(("dWop", "dbop", "dgamma"), outs, refs, refs_abs):
        _check(f"cti_gate_grads C{Cc} K{K} {name}", got, ref, C64 * U * ab)


# (B, R, C, ld_src, s_src, ld_dst, s_dst); the last: more than 4096 workgroups x 1024 elements, the grid-stride loop wraps
_ROWS = [(3, 5, 7, 9, 48, 11, 57), (3, 4, 16, 16, 64, 24, 100), (1, 4100, 1030, 1030, 0, 1032, 0)]


def _span(B, R, Cc, ld, sb):
    return (B - 1) * sb + (R - 1) * ld + Cc


@pytest.mark.parametrize("src_f32", [1, 0])
@pytest.mark.parametrize("geo", _ROWS, ids=lambda g: "B{}-R{}-C{}".format(*g[:3]))
def test_rows_copy_f16_bits(geo, src_f32):
    L = _L()
    B, Rr, Cc, lds, ss, ldd, sd = geo
    assert Rr * Cc > 4096 * 1024 or B > 1
    g = torch.Generator().manual_seed(Rr + src_f32)
    src = torch.randn(_span(B, Rr, Cc, lds, ss), generator=g)
    src = src if src_f32 else src.half()
    dst0 = torch.full((_span(B, Rr, Cc, ldd, sd),), float("nan"), dtype=F16)
    dst0.view(torch.int16).fill_(-1)
    want = R.rows_copy(src.half(), dst0, B, Rr, Cc, lds, ss, ldd, sd)          # (f32 source: torch's own rounding to fp16)
    sd_, dd = _dev(src, F32 if src_f32 else F16), _nan(dst0.numel(), F16)
    L.lib().wc_rows_copy_f16(_ptr(sd_), src_f32, _ptr(dd), B, Rr, Cc, lds, ss, ldd, sd, L.stream())
    torch.cuda.synchronize()
    got = dd.cpu().view(torch.int16)
    same = got == want.view(torch.int16)
    assert same.all(), f"rows_copy_f16: {int((~same).sum())} elements differ (copied values or the gaps between rows)"
    assert int((want.view(torch.int16) == -1).sum()) == dst0.numel() - B * Rr * Cc


@pytest.mark.parametrize("geo", _ROWS, ids=lambda g: "B{}-R{}-C{}".format(*g[:3]))
def test_rows_add_f32(geo):
    L = _L()
    B, Rr, Cc, lds, ss, _, _ = geo
    sd = Rr * Cc + (5 if B > 1 else 0)                                       # dense rows, a gap between the batches
    alpha = -1.75
    g = torch.Generator().manual_seed(Rr)
    src = torch.randn(_span(B, Rr, Cc, lds, ss), generator=g)
    dst0 = torch.full((_span(B, Rr, Cc, Cc, sd),), float("nan"))
    rows = R._row_index(B, Rr, Cc, Cc, sd)
    dst0[rows] = torch.randn(rows.numel(), generator=g)
    ref, ref_abs = R.rows_add(src, dst0, B, Rr, Cc, lds, ss, sd, alpha)
    sd_, dd = _dev(src, F32), _nan(dst0.numel(), F32)
    dd.copy_(dst0.cuda())
    gap = torch.ones(dst0.numel(), dtype=torch.bool)
    gap[rows] = False
    dd.view(torch.int32)[gap.cuda()] = -1
    L.lib().wc_rows_add_f32(_ptr(sd_), _ptr(dd), B, Rr, Cc, lds, ss, sd, alpha, L.stream())
    torch.cuda.synchronize()
    got = dd.cpu()
    _check(f"rows_add B{B} R{Rr} C{Cc}", got[rows], ref[rows], C64 * U * ref_abs[rows])
    assert (got.view(torch.int32)[gap] == -1).all(), "rows_add_f32 wrote into the gap between two batches"
    assert gap.sum() == (B - 1) * 5


# ---------------------------------------------------------------------------------------------------------------------------
# argument errors: refused on the host, nothing launched (every pointer and size here is valid for the call it is given to)

def test_argument_errors_launch_nothing():
    L = _L()
    lib = L.lib()
    # MRFP: C = 96, nine levels
    shapes = [(2, 2)] * 9
    S = 4 * 9
    for Cc, nl in ((96, 3), (64, 9)):
        n = S * 128
        x = _dev(torch.randn(n), F32)
        w = _dev(torch.randn(128 * 25), F32)
        y, g16, dx, part = _nan(n, F32), _nan(n, F16), _nan(n, F32), _nan(64 * 256 * 26, F32)
        dw = [_nan(128 * 25, F32) for _ in range(4)]
        _refused(lambda: lib.wc_mrfp_dwconv_fwd(_ptr(x), _ptr(w), _ptr(w), _ptr(w), _ptr(w), _ptr(y), _ptr(g16), _hs(shapes), nl, 1, Cc,
                                                L.stream()), y, g16)
        _refused(lambda: lib.wc_mrfp_dwconv_bwd(_ptr(x), 0, _ptr(x), _ptr(w), _ptr(w), _ptr(dx), None, *[_ptr(t) for t in dw], _ptr(part),
                                                1.0, _hs(shapes), nl, 1, Cc, L.stream()), dx, part, *dw)
        npart = ctypes.c_long(-7)
        with pytest.raises(RuntimeError, match=r"\(code 1\)"):
            lib.wc_mrfp_dwconv_parts(_hs(shapes), nl, 1, Cc, ctypes.byref(npart))
        assert npart.value == -7
    # conv stem: stride 3, a cols buffer off 16-byte alignment
    N, H, W, Cc, Kp = 1, 6, 6, 8, 128
    x = _dev(torch.randn(N * H * W * Cc), F32)
    hi, lo = _nan(N * H * W * Kp, F16), _nan(N * H * W * Kp, F16)
    _refused(lambda: lib.wc_im2col3x3(_ptr(x), _ptr(hi), _ptr(lo), N, H, W, Cc, 3, Kp, L.stream()), hi, lo)
    hi1 = _nan(N * H * W * Kp, F16, skew=1)
    _refused(lambda: lib.wc_im2col3x3(_ptr(x), _ptr(hi1), _ptr(lo), N, H, W, Cc, 1, Kp, L.stream()), hi1, lo)
    dcols, dx = _dev(torch.randn(N * H * W * Kp), F32), _nan(N * H * W * Cc, F32)
    _refused(lambda: lib.wc_col2im3x3(_ptr(dcols), _ptr(dx), N, H, W, Cc, 3, Kp, L.stream()), dx)
    # GroupNorm: C / G = 2
    Cc, G, HW = 16, 8, 10
    x, gam = _dev(torch.randn(HW * Cc), F32), _dev(torch.randn(Cc), F32)
    y, stats, part = _nan(HW * Cc, F32), _nan(G * 2, F32), _nan(G * 2, F32)
    _refused(lambda: lib.wc_groupnorm_relu_fwd(_ptr(x), _ptr(gam), _ptr(gam), _ptr(y), _ptr(stats), _ptr(part), 1, HW, Cc, G, EPS,
                                               L.stream()), y, stats, part)
    dxg, dg, db, cpart = _nan(HW * Cc, F32), _nan(Cc, F32), _nan(Cc, F32), _nan(Cc * 2, F32)
    _refused(lambda: lib.wc_groupnorm_relu_bwd(_ptr(x), _ptr(x), _ptr(x), _ptr(gam), _ptr(gam), _ptr(dxg), _ptr(dg), _ptr(db),
                                               _ptr(part), _ptr(cpart), _ptr(stats), 1, HW, Cc, G, L.stream()), dxg, dg, db, cpart)
