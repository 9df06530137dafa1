"""fp64 reference and error model of csrc/par.hip (pixel-adaptive refinement), for tests/test_par_ref_cpu.py (no GPU) and
tests/test_par_kernels_gpu.py.  Nothing here imports the oracle or needs a GPU.

Definition (reference WeCLIP_model/PAR.py:64-92): the T = 8 * n_dilations neighbours of a pixel are fetched by index clamping
(== replicate padding), in get_kernel() order per dilation; per colour channel the unbiased std over the T neighbours; e_t =
-mean_c((|nbr_t - centre| / (std_c + 1e-8) / w1)^2); aff_t = softmax_t(e) + pi_t with pi = w2 * softmax(-(pos / (std(pos) +
1e-8) / w1)^2); one sweep is out(p) = sum_t aff_t(p) masks(nbr_t(p)).

Error model.  eps = 2^-24 (half an ulp of fp32 relative to the value).

fp32 affinity, per element:  K * eps * (a_t * (1 + |e_t| + sum_s a_s |e_s|) + 1 / T).
    First order: d a_t = w_t (d e_t - sum_s w_s d e_s) with |d e_s| a few eps of |e_s| (three squares of rounded quotients),
    the exponential and the normalisation a few eps of w_t and the addition of pi_t half an ulp of a_t; 1 / T is the floor
    for the weights below the mean.  (With |e_t - e_max| in place of |e_t| + sum_s a_s |e_s| the fp32 oracle itself is 148
    units out on the noisy images, where e_max is -200 .. -1600: the error of an exponent scales with the exponent, not
    with its distance to the largest one.  In this form all five image kinds measure alike.)  K is MEASURED: the worst
    ratio of the fp32 oracle (oracle.weclip_oracle.par_affinity) to affinity() over all five image kinds at the shapes of the
    GPU module (tests/test_par_ref_cpu.py::test_affinity_bound_admits_the_fp32_oracle prints it), times a margin of 4 for the
    kernel's one reciprocal per channel in place of two divisions (<= 2 ulp on the argument, amplified by |e|) and __expf.

fp32 sweep:  (T + 2) * eps * sum_t |a_t| |m(nbr_t)|  (T fused multiply-adds), plus sum_t bound(a_t) |m(nbr_t)| when the kernel
    computed the weights itself.

Fixed point (H16, `fast` precision), from the code of par_affinity_reg_kernel<6, true, true>: scale q = fl(amax / 65535), the
    weights in tap order are rounded with the remainder carried on: a' = fl(a_t + carry), n = clamp(rint(a' * fl(65535 /
    amax))), carry = a' - n q.  |a' / q - n| <= 1/2 + 65535 * 2 eps (the roundings of a' * rs and of rs), so every carry is
    within q / 2 + 2 eps amax and every stored weight n q within q + 4 eps amax of its fp32 value.  The exact prefix sums of
    stored - fp32 equal minus the carry up to the roundings of a' and n q, at most eps (a' + n q) per tap: a drift of at
    most 2 eps sum_t a_t over a row.  Hence for one sweep
        |err(p)| <= (q (1 + 1e-3) + 4 eps amax) sum_t |m(nbr_t)|  + the fp32 terms,
    and for the all-ones mask, where the output is the row sum,
        |err(p)| <= q / 2 (1 + 1e-3) + 2 eps amax + 2 eps sum_t a_t  + the fp32 terms.
    In the sweep the kernel accumulates integer weights times mask values and scales once: (T + 2) eps sum |a| |m| again; for
    the all-ones mask the products and sums are integers below 2^24, hence exact, and one rounding (the scaling) is left.
    The Abel-summation form of the general bound (h16_bound(..., abel=True)): the error is sum_t d_t m_t with every prefix
    sum of d within c = q / 2 (1 + 1e-3) + 2 eps amax + 2 eps sum a, so |err| <= c (|m_last| + sum_t |m_t - m_{t+1}|).

Where every e_t of a pixel is exactly 0 (its whole neighbourhood has its colour: the constant image, the flat parts of the
piecewise one) the affinity needs no measured constant, see aff_bound: that is what lets the all-ones bound tell error
diffusion from plain rounding, whose row sum is 3 bounds out on the constant image.

Measured on the MI355X (worst err / bound per instantiation, tests/test_par_kernels_gpu.py -s): see RATIOS below.
"""
import math

import torch

F64, F32 = torch.float64, torch.float32
EPS = 2.0 ** -24
W1, W2 = 0.3, 0.01
DIRS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))        # get_kernel() order, PAR.py:10-24
DIL6 = (1, 2, 4, 8, 12, 24)

# worst |fp32 oracle - fp64| / (eps (a (1 + |e_t| + sum_s a_s |e_s|) + 1 / T)) over the five image kinds, SHAPES and the
# dilation sets of the GPU module: K_MEASURED (per kind: const 0.61, piecewise 4.58, piecewise_noise 4.90, ramp_noise 5.03,
# synth 5.01; printed by tests/test_par_ref_cpu.py); K_AFF = 4 x that, rounded up
K_MEASURED = 5.03
K_AFF = 21.0

SHAPES = ((1, 1), (3, 5), (7, 63), (8, 64), (9, 65), (25, 70), (40, 72), (13, 130))
KINDS = ("const", "piecewise", "piecewise_noise", "ramp_noise", "synth")
AFF_DILS = ((1, 2, 4, 8, 12, 24), (1,), (2, 5), (1, 2, 4, 8, 12), (1, 2, 3, 4, 6, 8, 12, 24))
H16_DILS = ((1, 2, 4, 8, 12, 24), (1, 2, 4, 8, 13, 24), (12, 13, 1, 24, 2, 3), (13, 14, 16, 20, 24, 30))

# worst err / bound per kernel instantiation on the MI355X (the H16 sweeps come within 2 % of the bound on the probe masks:
# there the output is one stored weight and the bound its rounding quantum)
RATIOS = {
    "par_affinity_kernel": 0.255, "par_affinity_reg_kernel<6, false>": 0.26,
    "par_iter_kernel<2, false>": 0.296, "par_iter_kernel<3, false>": 0.293, "par_iter_kernel<4, false>": 0.361,
    "par_iter_kernel<2, true>": 0.137, "par_iter_kernel<3, true>": 0.227, "par_iter_kernel<4, true>": 0.178,
    "par_iter_kernel<2, true, true, 8, 12>": 0.969, "par_iter_kernel<3, true, true, 8, 12>": 0.974,
    "par_iter_kernel<4, true, true, 8, 12>": 0.981,
    "par_iter_kernel<2, true, true, 8, 12> (Abel bound)": 0.321, "par_iter_kernel<3, true, true, 8, 12> (Abel bound)": 0.354,
    "par_iter_kernel<4, true, true, 8, 12> (Abel bound)": 0.349,
}


# ---------------------------------------------------------------------------------------------------------------------
# reference

def taps(dilations):
    """-> ([(dy, dx)] in build_taps order, pi (T,) fp64)."""
    offs = [(dy * d, dx * d) for d in dilations for dy, dx in DIRS]
    pos = torch.tensor([d * (math.sqrt(2.0) if dy and dx else 1.0) for d in dilations for dy, dx in DIRS], dtype=F64)
    pe = -((pos / (pos.std() + 1e-8) / W1) ** 2)
    return offs, W2 * torch.softmax(pe, 0)


def shift(x, dy, dx):
    """x(..., H, W) at the clamped neighbour (y + dy, x + dx) of every pixel."""
    H, W = x.shape[-2:]
    yy = (torch.arange(H) + dy).clamp(0, H - 1)
    xx = (torch.arange(W) + dx).clamp(0, W - 1)
    return x[..., yy, :][..., xx]


def affinity(img, dilations):
    """img (3, H, W) -> aff (T, H, W) fp64, amax (H, W) = max_t aff, de (T, H, W) = e_t - max_t e, e (T, H, W)."""
    img = img.to(F64)
    offs, pi = taps(dilations)
    nb = torch.stack([shift(img, dy, dx) for dy, dx in offs], 1)                      # (3, T, H, W)
    std = nb.std(dim=1, keepdim=True)
    e = (-(((nb - img[:, None]).abs() / (std + 1e-8) / W1) ** 2)).mean(0)
    aff = torch.softmax(e, 0) + pi[:, None, None]
    return aff, aff.max(0).values, e - e.max(0, keepdim=True).values, e


def sweep_terms(aff, masks, dilations, wb=None):
    """One sweep of masks (C, H, W) with weights aff (T, H, W), all in the dtype of aff: -> (out, sum_t |a_t| |m(nbr_t)|,
    sum_t |m(nbr_t)|, sum_t wb_t |m(nbr_t)| or None)."""
    offs, _ = taps(dilations)
    masks = masks.to(aff.dtype)
    out = torch.zeros_like(masks)
    s_am, s_m = torch.zeros_like(masks), torch.zeros_like(masks)
    s_b = torch.zeros_like(masks) if wb is not None else None
    for t, (dy, dx) in enumerate(offs):
        m = shift(masks, dy, dx)
        out = out + aff[t] * m
        s_am += aff[t].abs() * m.abs()
        s_m += m.abs()
        if wb is not None:
            s_b += wb[t] * m.abs()
    return out, s_am, s_m, s_b


def sweep(aff, masks, dilations):
    return sweep_terms(aff.to(F64), masks, dilations)[0]


def forward(img, masks, dilations, n):
    """n sweeps of masks (C, H, W) with the affinities of img (3, H, W)."""
    aff = affinity(img, dilations)[0]
    m = masks.to(F64)
    for _ in range(n):
        m = sweep(aff, m, dilations)
    return m


def labels(masks, keys, nch=None):
    """masks (B, C, H, W), keys (B, C) int64, nch (B,) or None -> keys[b, first argmax over the first nch[b] channels]."""
    B, C = masks.shape[:2]
    out = []
    for b in range(B):
        n = C if nch is None else int(nch[b])
        m = masks[b, :n]
        best, bi = m[0].clone(), torch.zeros(m.shape[1:], dtype=torch.int64)
        for c in range(1, n):
            up = m[c] > best
            best = torch.where(up, m[c], best)
            bi[up] = c
        out.append(keys[b][bi])
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------------------------------
# inputs (fp32, at mask resolution, seeded)

def images(kind, B, H, W, seed=0):
    """(B, 3, H, W) fp32.  Noise is never far below the signal on a flat image (the std would be ill-conditioned)."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * H + W)
    col = torch.rand(B, 3, 1, 1, generator=g) * 2 - 1
    x = torch.arange(W, dtype=F32)[None, None, None, :]
    y = torch.arange(H, dtype=F32)[None, None, :, None]
    if kind == "const":
        return col.expand(B, 3, H, W).contiguous()
    if kind in ("piecewise", "piecewise_noise"):
        img = col + 0.75 * (x >= W // 2).float() + torch.zeros(B, 3, H, W)
        img[:, 1] += 0.5 * (y[:, 0] >= H // 2).float()
        if kind == "piecewise_noise":
            img = img + 0.05 * torch.randn(B, 3, H, W, generator=g)
        return img.contiguous()
    if kind == "ramp_noise":
        ramp = col * (x / max(W - 1, 1)) + (1 - col) * (y / max(H - 1, 1))
        return (ramp + 0.1 * torch.randn(B, 3, H, W, generator=g)).contiguous()
    if kind == "synth":
        from oracle import synth            # the input generators only, not the oracle
        return synth.make_images(B, H, W, seed=seed + 100)
    raise ValueError(kind)


def masks(kind, B, C, H, W, seed=0):
    """dense: uniform [0, 1); ones; probes: every channel the indicator of a seeded pixel set of ~1/97 density (never empty)."""
    g = torch.Generator().manual_seed(7000 + 1000 * seed + 31 * C + 17 * H + W)
    if kind == "dense":
        return torch.rand(B, C, H, W, generator=g)
    if kind == "ones":
        return torch.ones(B, C, H, W)
    if kind == "probes":
        m = (torch.rand(B, C, H * W, generator=g) < 1.0 / 97).float()
        first = torch.randint(0, H * W, (B, C, 1), generator=g)
        m.scatter_(2, first, 1.0)
        return m.view(B, C, H, W).contiguous()
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------------
# bounds

def aff_unit(aff, e):
    return EPS * (aff * (1 + e.abs() + (aff * e.abs()).sum(0, keepdim=True)) + 1.0 / aff.shape[0])


def pi_bound(dilations):
    """The host computes pi in fp32 by the same steps (quotient, square, exponential, normalisation): the same model."""
    offs, pi = taps(dilations)
    pos = torch.tensor([math.hypot(dy, dx) for dy, dx in offs], dtype=F64)
    pe = (pos / (pos.std() + 1e-8) / W1) ** 2
    return K_AFF * EPS * (pi * (1 + pe + (pi / W2 * pe).sum()) + W2 / len(offs))


def aff_bound(aff, e, dilations):
    """Per element.  Where the whole neighbourhood of a pixel has the pixel's colour (every e_t == 0 exactly) no measured
    constant is needed: every exponential is 1 and their sum T exactly, which leaves the rounding of 1 / T, that of the
    addition of pi_t (each counted twice: a reciprocal that is 1 ulp off) and the host's fp32 pi."""
    flat = (e == 0).all(0, keepdim=True)
    exact = 2 * EPS * (1.0 / aff.shape[0] + aff) + pi_bound(dilations).view(-1, *([1] * (aff.dim() - 1)))
    return torch.where(flat, exact, K_AFF * aff_unit(aff, e))


def acc_bound(s_am, T):
    return (T + 2) * EPS * s_am


def sweep_bound(aff, masks, dilations, wb=None):
    """fp32 sweep with weights aff (exact when wb is None, else each within wb of aff): bound on |out - sweep(aff, masks)|."""
    _, s_am, _, s_b = sweep_terms(aff.to(F64), masks, dilations, wb)
    b = acc_bound(s_am, aff.shape[0])
    return b if wb is None else b + s_b


def h16_weight_bound(amax):
    """|stored weight - fp32 weight| per tap."""
    return amax / 65535 * (1 + 1e-3) + 4 * EPS * amax


def h16_bound(aff, amax, e, masks, dilations, abel=False):
    """One H16 sweep against sweep(aff, masks): the general bound, or its Abel-summation form."""
    T = aff.shape[0]
    ab = aff_bound(aff, e, dilations)
    _, s_am, s_m, s_b = sweep_terms(aff, masks, dilations, ab)
    fp32 = acc_bound(s_am, T) + s_b
    if not abel:
        return h16_weight_bound(amax) * s_m + fp32
    offs, _ = taps(dilations)
    m = torch.stack([shift(masks.to(F64), dy, dx) for dy, dx in offs])               # (T, C, H, W)
    tv = m[-1].abs() + (m[1:] - m[:-1]).abs().sum(0)
    c = 0.5 * amax / 65535 * (1 + 1e-3) + 2 * EPS * amax + 2 * EPS * aff.sum(0)
    return c * tv + fp32


def h16_ones_bound(aff, amax, e, dilations):
    """One H16 sweep of the all-ones mask against the row sum of aff.  The accumulation is exact (integers below 2^24)."""
    s = aff.sum(0)
    return 0.5 * amax / 65535 * (1 + 1e-3) + 2 * EPS * amax + 2 * EPS * s + aff_bound(aff, e, dilations).sum(0) + 2 * EPS * s


def forward_bound(aff, masks, dilations, n, wb):
    """n sweeps with weights within wb of aff: E_0 = 0, E_{k+1} = sum_t (|a_t| + wb_t) E_k(nbr_t) + the one-sweep bound of
    the fp64 iterate m_k."""
    aff = aff.to(F64)
    m = masks.to(F64)
    E = torch.zeros_like(m)
    for _ in range(n):
        E = sweep_terms(aff.abs() + wb, E, dilations)[0] * (1 + (aff.shape[0] + 2) * EPS) + sweep_bound(aff, m, dilations, wb)
        m = sweep(aff, m, dilations)
    return E
