"""fp64 restatements of the ViT-CoMer insert kernels that have no other statement of what they compute: the MRFP depth-wise
convolutions and the glue kernels of csrc/comer.hip, the conv-stem gathers and GroupNorm + ReLU of csrc/convstem.hip, and the
NCHW depth-wise convolution of csrc/dwconv.hip.  Written from the formulas in those files' header comments, in plain torch
float64 on the CPU; nothing here calls the package.  tests/test_comer_ref_cpu.py checks every function against stock torch.

Where a kernel test needs an error scale, a function returns (value, value_abs): value_abs is the same evaluation on the
absolute values of every operand ("sum |terms|"), the scale of `|got - ref| <= c 2^-24 sum|terms|`."""
import math

import torch

F64 = torch.float64
U = 2.0 ** -24          # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------------------------------------
# depth-wise convolution on maps (N, H, W, Ch) with one k x k filter per channel, zero padding

def _dw(xm, w, k, mode):
    """xm (N,H,W,Ch), w (Ch, k*k) with tap index ky*k + kx.
      mode 'fwd' : out[y, x] = sum_taps w[ky, kx] * xm[y + ky - R, x + kx - R]
      mode 'bwdx': out[y, x] = sum_taps w[ky, kx] * xm[y - ky + R, x - kx + R]          (the transposed convolution)"""
    N, H, W, Ch = xm.shape
    R = k // 2
    xp = torch.zeros(N, H + 2 * R, W + 2 * R, Ch, dtype=F64)
    xp[:, R:R + H, R:R + W] = xm
    out = torch.zeros(N, H, W, Ch, dtype=F64)
    for ky in range(k):
        for kx in range(k):
            oy, ox = (ky, kx) if mode == "fwd" else (2 * R - ky, 2 * R - kx)
            out += w[:, ky * k + kx] * xp[:, oy:oy + H, ox:ox + W]
    return out


def _dw_wgrad(xm, gm, k):
    """dw[c, ky*k + kx] = sum_{n,y,x} gm[n, y, x, c] * xm[n, y + ky - R, x + kx - R, c] -> (Ch, k*k)"""
    N, H, W, Ch = xm.shape
    R = k // 2
    xp = torch.zeros(N, H + 2 * R, W + 2 * R, Ch, dtype=F64)
    xp[:, R:R + H, R:R + W] = xm
    dw = torch.zeros(Ch, k * k, dtype=F64)
    for ky in range(k):
        for kx in range(k):
            dw[:, ky * k + kx] = (gm * xp[:, ky:ky + H, kx:kx + W]).sum((0, 1, 2))
    return dw


def level_starts(shapes):
    """First token row of every level and the total number of rows S."""
    starts, s = [], 0
    for H, W in shapes:
        starts.append(s)
        s += H * W
    return starts, s


def mrfp_parts(shapes, N, C):
    """Partial rows of the two-stage filter-gradient reduction: strips of 8 pixels per map row, 4 * (256 / C) strips per
    workgroup and image."""
    strips = sum(H * ((W + 7) // 8) for H, W in shapes)
    per = 4 * (256 // C)
    return N * ((strips + per - 1) // per), strips


def _mrfp_apply(rows, shapes, fn):
    """rows (N, S, C) -> fn(map (N,H,W,C), level) per level, back to rows."""
    N, S, C = rows.shape
    starts, S2 = level_starts(shapes)
    assert S == S2
    out = torch.empty(N, S, C, dtype=F64)
    for (H, W), s in zip(shapes, starts):
        out[:, s:s + H * W] = fn(rows[:, s:s + H * W].reshape(N, H, W, C)).reshape(N, H * W, C)
    return out


def mrfp_dwconv(x, w3, b3, w5, b5, shapes):
    """x (N,S,C); 3x3 filters w3 (C/2, 9) + b3 on channels [0, C/2), 5x5 filters w5 (C/2, 25) + b5 on [C/2, C); zero padding per
    level -> (y, y_abs)."""
    h = x.shape[-1] // 2

    def one(x, w3, b3, w5, b5):
        return _mrfp_apply(x, shapes, lambda m: torch.cat([_dw(m[..., :h], w3, 3, "fwd") + b3, _dw(m[..., h:], w5, 5, "fwd") + b5], -1))
    x, w3, b3, w5, b5 = [t.double() for t in (x, w3, b3, w5, b5)]
    return one(x, w3, b3, w5, b5), one(x.abs(), w3.abs(), b3.abs(), w5.abs(), b5.abs())


def gelu(y):
    """y * Phi(y) with the exact erf."""
    y = y.double()
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def mrfp_dwconv_bwd_data(dy, w3, w5, shapes):
    """dx[p] = sum_taps w[tap] * dy[p - tap] per level and channel -> (dx, dx_abs)."""
    h = dy.shape[-1] // 2

    def one(dy, w3, w5):
        return _mrfp_apply(dy, shapes, lambda m: torch.cat([_dw(m[..., :h], w3, 3, "bwdx"), _dw(m[..., h:], w5, 5, "bwdx")], -1))
    dy, w3, w5 = [t.double() for t in (dy, w3, w5)]
    return one(dy, w3, w5), one(dy.abs(), w3.abs(), w5.abs())


def mrfp_dwconv_bwd_filters(dy, x, shapes, alpha):
    """alpha * (dw3 (C/2, 9), db3 (C/2), dw5 (C/2, 25), db5 (C/2)), summed over images, levels and pixels -> (tuple, tuple_abs)."""
    N, S, C = x.shape
    h = C // 2
    starts, _ = level_starts(shapes)

    def one(dy, x, a):
        dw3, dw5 = torch.zeros(h, 9, dtype=F64), torch.zeros(h, 25, dtype=F64)
        for (H, W), s in zip(shapes, starts):
            xm, gm = [t[:, s:s + H * W].reshape(N, H, W, C) for t in (x, dy)]
            dw3 += _dw_wgrad(xm[..., :h], gm[..., :h], 3)
            dw5 += _dw_wgrad(xm[..., h:], gm[..., h:], 5)
        db = dy.sum((0, 1))
        return a * dw3, a * db[:h], a * dw5, a * db[h:]
    dy, x = dy.double(), x.double()
    return one(dy, x, alpha), one(dy.abs(), x.abs(), abs(alpha))


# ---------------------------------------------------------------------------------------------------------------------------
# NCHW depth-wise convolution (stride 1, zero "same" padding, odd k <= 7)

def dwconv_fwd(x, w, bias):
    """x (N,C,H,W), w (C,k,k), bias (C) or None -> (y, y_abs)."""
    k = w.shape[-1]

    def one(x, w, b):
        y = _dw(x.permute(0, 2, 3, 1), w.reshape(w.shape[0], -1), k, "fwd")
        return (y if b is None else y + b).permute(0, 3, 1, 2)
    x, w = x.double(), w.double()
    b = None if bias is None else bias.double()
    return one(x, w, b), one(x.abs(), w.abs(), None if b is None else b.abs())


def dwconv_bwd(x, w, dy):
    """-> ((dx, dw (C,k,k), db (C)), the same on absolute values)."""
    k = w.shape[-1]

    def one(x, w, dy):
        dx = _dw(dy.permute(0, 2, 3, 1), w.reshape(w.shape[0], -1), k, "bwdx").permute(0, 3, 1, 2)
        dw = _dw_wgrad(x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1), k).reshape(w.shape)
        return dx, dw, dy.sum((0, 2, 3))
    x, w, dy = x.double(), w.double(), dy.double()
    return one(x, w, dy), one(x.abs(), w.abs(), dy.abs())


# ---------------------------------------------------------------------------------------------------------------------------
# conv-stem gathers: 3x3 / stride s / pad 1 on NHWC rows

def out_size(n, stride):
    return (n + 2 - 3) // stride + 1


def im2col3x3(x, stride, Kp):
    """x (N,H,W,C) float32 -> (hi, lo) (N*Ho*Wo, Kp) float16: column (ky*3 + kx)*C + c of row (n, oy, ox) holds
    x[n, oy*s - 1 + ky, ox*s - 1 + kx, c] (0 outside the map and in the columns [9C, Kp)), hi = fp16(v), lo = fp16(v - hi)."""
    N, H, W, C = x.shape
    assert x.dtype == torch.float32 and Kp >= 9 * C
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float32)
    xp[:, 1:H + 1, 1:W + 1] = x
    cols = torch.zeros(N, Ho, Wo, Kp, dtype=torch.float32)
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            cols[..., t * C:(t + 1) * C] = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
    hi = cols.half()
    lo = (cols - hi.float()).half()          # (the fp32 difference is exact)
    return hi.reshape(-1, Kp), lo.reshape(-1, Kp)


def im2col3x3_values(x, stride):
    """The gathered values before the split, float64 (N, Ho, Wo, 9C): the index map alone."""
    N, H, W, C = x.shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=F64)
    xp[:, 1:H + 1, 1:W + 1] = x.double()
    return torch.cat([xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
                      for ky in range(3) for kx in range(3)], -1)


def col2im3x3(dcols, H, W, C, stride):
    """The adjoint of the index map: dcols (N, Ho, Wo, Kp) -> (dx (N,H,W,C), dx_abs); only the columns [0, 9C) are read."""
    N, Ho, Wo, _ = dcols.shape
    assert (Ho, Wo) == (out_size(H, stride), out_size(W, stride))

    def one(d):
        dxp = torch.zeros(N, H + 2, W + 2, C, dtype=F64)
        for ky in range(3):
            for kx in range(3):
                t = ky * 3 + kx
                dxp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] += d[..., t * C:(t + 1) * C]
        return dxp[:, 1:H + 1, 1:W + 1]
    d = dcols[..., :9 * C].double()
    return one(d), one(d.abs())


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm + ReLU on rows (N, HW, C), G groups of C / G consecutive channels

def _grp(t, G):
    N, HW, C = t.shape
    return t.reshape(N, HW, G, C // G)


def gn_stats(x, G, eps):
    """-> mean (N,G), rstd (N,G) = 1 / sqrt(var + eps) with the biased variance, and E|x|, E[x^2] per (n, g)."""
    xg = _grp(x.double(), G)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    return mean, 1.0 / torch.sqrt(var + eps), xg.abs().mean((1, 3)), (xg ** 2).mean((1, 3))


def _per_channel(s, C):
    """(N, G) -> (N, 1, C)"""
    return s.repeat_interleave(C // s.shape[1], 1)[:, None, :]


def gn_relu_pre(x, mean, rstd, gamma, beta):
    """The pre-activation (x - mean) * rstd * gamma + beta (y = relu of it) -> (pre, pre_abs)."""
    C = x.shape[-1]
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    m, r = _per_channel(mean.double(), C), _per_channel(rstd.double(), C)
    xh = (x - m) * r
    return xh * gamma + beta, xh.abs() * gamma.abs() + beta.abs()


def gn_relu_bwd(x, mean, rstd, gamma, dy, mask, G):
    """Backward of y = relu(GroupNorm(x)) through a given ReLU mask, with d = dy * mask, g = d * gamma, xhat = (x - mean) rstd:
      dgamma[c] = sum_{n,r} d xhat,   dbeta[c] = sum_{n,r} d,   dx = rstd (g - (sum_grp g + xhat sum_grp g xhat) / count)
    -> ((dx, dgamma, dbeta), the same on absolute values)."""
    N, HW, C = x.shape
    count = HW * (C // G)
    x, gamma = x.double(), gamma.double()
    m, r = _per_channel(mean.double(), C), _per_channel(rstd.double(), C)
    xh = (x - m) * r

    def one(d, xh, gam, sign):
        g = d * gam
        sg = _per_channel(_grp(g, G).sum((1, 3)), C)
        sgx = _per_channel(_grp(g * xh, G).sum((1, 3)), C)
        return r * (g + sign * (sg + xh * sgx) / count), (d * xh).sum((0, 1)), d.sum((0, 1))
    d = dy.double() * mask.double()
    return one(d, xh, gamma, -1.0), one(d.abs(), xh.abs(), gamma.abs(), 1.0)      # (on absolute values every term is added)


# ---------------------------------------------------------------------------------------------------------------------------
# glue

def cti_gate_grads(G, s, gamma, Wop, bop):
    """dWop = diag(gamma) G, dbop = gamma * s, dgamma = rowsum(Wop * G) + bop * s -> ((dWop, dbop, dgamma), on absolute values)."""
    def one(G, s, gamma, Wop, bop):
        return gamma[:, None] * G, gamma * s, (Wop * G).sum(1) + bop * s
    a = [t.double() for t in (G, s, gamma, Wop, bop)]
    return one(*a), one(*[t.abs() for t in a])


def _row_index(B, R, C, ld, sb):
    b, r, c = torch.meshgrid(torch.arange(B), torch.arange(R), torch.arange(C), indexing="ij")
    return (b * sb + r * ld + c).reshape(-1)


def rows_copy(src, dst, B, R, C, ld_src, s_src, ld_dst, s_dst):
    """dst[b*s_dst + r*ld_dst + c] = src[b*s_src + r*ld_src + c] on flat buffers; every other element of dst is kept."""
    out = dst.clone()
    out[_row_index(B, R, C, ld_dst, s_dst)] = src[_row_index(B, R, C, ld_src, s_src)].to(dst.dtype)
    return out


def rows_add(src, dst, B, R, C, ld_src, s_src, s_dst, alpha):
    """dst[b*s_dst + r*C + c] += alpha * src[b*s_src + r*ld_src + c] in float64 -> (dst, |dst| + |alpha| |src|)."""
    i_d, i_s = _row_index(B, R, C, C, s_dst), _row_index(B, R, C, ld_src, s_src)
    out, out_abs = dst.double().clone(), dst.double().abs()
    out[i_d] += alpha * src.double()[i_s]
    out_abs[i_d] += abs(alpha) * src.double()[i_s].abs()
    return out, out_abs
