"""fp64 reference of multi-scale deformable attention (MSDA) for the kernel tests of csrc/msdeform.hip and csrc/comer.hip.

The CoMer inserts have no reference code; what pins them is the published definition (Deformable-DETR, as used by the
ViT-CoMer CTI blocks):

  out[n, q, m, :] = sum_l sum_p attn[n, q, m, l, p] * bilinear(value_l[n, :, m, :], loc[n, q, m, l, p] * (W_l, H_l) - 0.5)

with zero padding outside the map (F.grid_sample, align_corners=False, padding_mode='zeros').  Everything here is vectorised
torch float64; the gradients come from autograd through oracle.comer_oracle.ms_deform_attn (grid_sample) in double.

Error-scale helpers give the per-element bounds of the kernel tests (`|got - ref| <= c * 2^-24 * sum|terms|`): the same
evaluation on absolute values, the number of (sample, corner) pairs with a non-zero bilinear weight per value pixel, the sum
of |terms| of the location gradients, and the distance of every sample to the kinks of the location derivative."""
import torch

from oracle import comer_oracle as CO

F64 = torch.float64
U = 2.0 ** -24          # unit roundoff of fp32


def msda_fp64(value, shapes, loc, attn):
    """value (N,S,M,D), shapes [(H,W)...], loc (N,Lq,M,nL,P,2) as (x,y), attn (N,Lq,M,nL,P), all float64 -> out (N,Lq,M*D)."""
    return CO.ms_deform_attn(value, [tuple(s) for s in shapes], loc, attn)


def level_sizes(shapes):
    """(nL, 2) float64 tensor of (W_l, H_l): the normalisation of the sampling offsets."""
    return torch.tensor([[w, h] for h, w in shapes], dtype=F64)


def msda_fused_fp64(value, shapes, ow, ld, b_off, b_aw, ref, nl_ref, M, P):
    """What msda_fwd4f_kernel documents: ow (N*Lq, ld) = [M*T*2 offsets | M*T logits | padding] per query (T = nL*P),
    loc = ref + (off + b_off) / (W_l, H_l), attn = softmax_T(logits + b_aw).  ref (Lq, nl_ref, 2); b_off / b_aw may be None.
    -> (loc (N,Lq,M,nL,P,2), attn (N,Lq,M,nL,P), out (N,Lq,M*D)); autograd through it gives the gradient of the raw rows."""
    N = value.shape[0]
    nL = len(shapes)
    T = nL * P
    Lq = ow.shape[0] // N
    assert ow.shape[1] == ld and ld >= 3 * M * T
    off = ow[:, :M * T * 2].reshape(N, Lq, M, nL, P, 2)
    if b_off is not None:
        off = off + b_off.reshape(M, nL, P, 2)
    logits = ow[:, M * T * 2:3 * M * T].reshape(N, Lq, M, T)
    if b_aw is not None:
        logits = logits + b_aw.reshape(M, T)
    attn = torch.softmax(logits, -1).reshape(N, Lq, M, nL, P)
    r = ref.reshape(1, Lq, 1, nl_ref, 1, 2)
    loc = r + off / level_sizes(shapes).reshape(1, 1, 1, nL, 1, 2)
    return loc, attn, msda_fp64(value, shapes, loc, attn)


def pixel_coords(shapes, loc):
    """(x, y) pixel coordinates (N,Lq,M,nL,P) of the samples in float64: loc * size - 0.5."""
    sz = level_sizes(shapes).reshape(1, 1, 1, -1, 1, 2)
    p = loc.double() * sz - 0.5
    return p[..., 0], p[..., 1]


def corners(shapes, loc):
    """The four bilinear corners of every sample: (idx (N,Lq,M,nL,P,4) int64 pixel index over all levels, -1 where the corner
    or the whole sample lies outside the map; wgt (N,Lq,M,nL,P,4) bilinear weight, 0 there).  Corner order 00, 01, 10, 11
    as (y, x) offsets; a sample counts when -1 < x < W and -1 < y < H (the kernels' test)."""
    x, y = pixel_coords(shapes, loc)
    idx = torch.full(x.shape + (4,), -1, dtype=torch.int64)
    wgt = torch.zeros(x.shape + (4,), dtype=F64)
    start = 0
    for l, (H, W) in enumerate(shapes):
        xl, yl = x[..., l, :], y[..., l, :]
        inside = (xl > -1) & (yl > -1) & (xl < W) & (yl < H)
        x0, y0 = torch.floor(xl), torch.floor(yl)
        fx, fy = xl - x0, yl - y0
        for c, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            px, py = x0 + dx, y0 + dy
            ok = inside & (px >= 0) & (px < W) & (py >= 0) & (py < H)
            w = (fx if dx else 1 - fx) * (fy if dy else 1 - fy)
            pix = (py.clamp(0, H - 1) * W + px.clamp(0, W - 1)).long() + start
            idx[..., l, :, c] = torch.where(ok, pix, torch.full_like(pix, -1))
            wgt[..., l, :, c] = torch.where(ok, w, torch.zeros_like(w))
        start += H * W
    return idx, wgt


def abs_scales(value, shapes, loc, attn, gout):
    """sum |terms| of every output, attention-weight gradient and value gradient element: the same evaluation on |value|,
    |attn| and |gout| (bilinear weights are non-negative) -> (out_abs (N,Lq,M*D), gattn_abs, gvalue_abs)."""
    va = value.detach().double().abs().requires_grad_(True)
    aa = attn.detach().double().abs().requires_grad_(True)
    out = msda_fp64(va, shapes, loc.detach().double(), aa)
    out.backward(gout.detach().double().abs().reshape(out.shape))
    return out.detach(), aa.grad, va.grad


def corner_values(value, shapes, loc):
    """Values at the four corners of every sample, zero outside: (N,Lq,M,nL,P,4,D) float64, and the bilinear weights."""
    N, S, M, D = value.shape
    idx, wgt = corners(shapes, loc)
    Lq, nL, P = idx.shape[1], idx.shape[3], idx.shape[4]
    v = value.detach().double().permute(0, 2, 1, 3)                         # (N, M, S, D)
    ii = idx.clamp(min=0).permute(0, 2, 1, 3, 4, 5).reshape(N, M, -1)     # (N, M, Lq*nL*P*4)
    g = torch.gather(v, 2, ii[..., None].expand(-1, -1, -1, D))
    g = g.reshape(N, M, Lq, nL, P, 4, D).permute(0, 2, 1, 3, 4, 5, 6)
    return g * (idx >= 0)[..., None], wgt


def loc_grad_abs(value, shapes, loc, attn, gout):
    """sum |terms| of the location gradient d out / d loc (N,Lq,M,nL,P,2): per sample |attn| * size * sum_d |gout_d| *
    (hy (|v00| + |v01|) + ly (|v10| + |v11|)) for x, and the same with the roles of x and y swapped for y."""
    cv, wgt = corner_values(value, shapes, loc)
    N, Lq, M = loc.shape[:3]
    D = value.shape[-1]
    ga = gout.detach().double().abs().reshape(N, Lq, M, 1, 1, 1, D)
    s = (cv.abs() * ga).sum(-1)                                             # (N,Lq,M,nL,P,4): sum_d |gout_d| |v_c,d|
    x, y = pixel_coords(shapes, loc)
    fx, fy = x - torch.floor(x), y - torch.floor(y)
    sx = (1 - fy) * (s[..., 0] + s[..., 1]) + fy * (s[..., 2] + s[..., 3])
    sy = (1 - fx) * (s[..., 0] + s[..., 2]) + fx * (s[..., 1] + s[..., 3])
    sz = level_sizes(shapes).reshape(1, 1, 1, -1, 1, 2)
    return torch.stack([sx, sy], -1) * attn.detach().double().abs()[..., None] * sz


def pair_counts(shapes, loc, S):
    """Per value pixel and head: number of (sample, corner) pairs with a non-zero bilinear weight -> (N, S, M) float64."""
    idx, wgt = corners(shapes, loc)
    N, Lq, M = idx.shape[:3]
    cnt = torch.zeros(N, M, S + 1, dtype=F64)
    ii = torch.where(wgt > 0, idx, torch.full_like(idx, S)).permute(0, 2, 1, 3, 4, 5).reshape(N, M, -1)
    cnt.scatter_add_(2, ii, torch.ones_like(ii, dtype=F64))
    return cnt[..., :S].permute(0, 2, 1)


def kink_distance(shapes, loc):
    """Per sample and coordinate (N,Lq,M,nL,P,2): distance of the pixel coordinate to the nearest kink of the location
    derivative (an integer, which includes the -1 / size borders of the map)."""
    x, y = pixel_coords(shapes, loc)
    return torch.stack([(x - torch.round(x)).abs(), (y - torch.round(y)).abs()], -1)
