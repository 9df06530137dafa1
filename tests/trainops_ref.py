"""fp64 reference and error model of csrc/norm.hip and csrc/train_ops.hip (LayerNorm forward and backward, column sums, operand
transposes, sigmoid-Gram backward, column-scale split, weight conversion, AdamW), for tests/test_trainops_ref_cpu.py (no GPU) and
tests/test_trainops_kernels_gpu.py.  Nothing here imports the oracle or needs a GPU.

Definitions (all evaluated in fp64 from the fp32 / fp16 inputs):
    LayerNorm          y = (x - mean x) rstd gamma + beta, rstd = (mean (x - mean x)^2 + eps)^-1/2; hi = fp16(y), lo = fp16(y - hi).
    LayerNorm backward dx = add + rstd (g - mean g - xhat mean(g xhat)), g = sum over the norms of dy gamma (one norm or two
                       norms of one input); dx16 = fp16(out_scale dx); per norm dgamma = alpha sum_rows dy xhat, dbeta = alpha
                       sum_rows dy.
    column sum         out[c] = alpha sum_r src[r, c], optionally rounded through fp16.
    transpose          out[c, b oR + r] = fp16(scale src[b, r, c]) (+ lo).
    sigmoid-Gram       S = scale (z + z^T), z = dAP AP (1 - AP).
    column-scale split y = alpha x cs[row / rpb, col]  (cs may be absent) -> fp32, hi, lo.
    weight conversion  hi = fp16(w), lo = fp16(w - hi), row-major and transposed.
    AdamW              p *= 1 - lr wd;  m += (1 - b1) (g - m);  v = v b2 + (1 - b2) g g;
                       p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)      (the order csrc/train_ops.hip documents).

Error model.  EPS = 2^-24 (half an ulp of fp32 relative to the value).  Every fp32 output has the per-element bound
        K * EPS * A
where A is the absolute-value companion of the output's formula in fp64: the same expression with every term replaced by its
magnitude (dx: |add| + rstd (G + mean G + X mean(G X)) with G = sum |dy| |gamma|; a column sum: sum |src|; and so on, see
the functions below).  K is MEASURED, not chosen: the worst |fp32 - fp64| / (EPS A) of a plain fp32 torch evaluation of the same
formula (LayerNorm: F.layer_norm and its autograd in fp32) over the shapes and inputs of the GPU module -- K_MEASURED below, printed
by tests/test_trainops_ref_cpu.py::test_bounds_admit_the_fp32_emulation -- times a margin of 4 for rsqrtf in place of a square root
and a division, the kernels' different but fixed summation order and FMA contraction (the margin of tests/par_ref.py, for the
same reason), rounded up to the next integer: K below.

The LayerNorm inputs have rows with a mean offset of several standard deviations (offset 0.5, scales 0.1 .. 10): there x - mean
cancels and xhat carries an error of EPS (|x| + |mean|) rstd, which for an element next to the mean is thousands of times
EPS |xhat|.  So the replacement by magnitudes goes down to the inputs: the companion of xhat = (x - mean x) rstd is
X = (|x| + mean |x|) rstd, and X stands wherever the formula of y, dx or dgamma has xhat.  (With |xhat| itself the fp32 autograd of
F.layer_norm measures K = 38 for dx and K = 10 072 for dgamma, both set by single elements next to their row mean; with X, 4.3
and 2.9.)

An output rounded to fp16 adds one fp16 rounding: 2^-11 |v|, with the fp16 subnormal spacing 2^-24 as a floor (h_bound).  A hi / lo
pair is checked as hi + lo against v with 2^-22 |v| plus that floor (hl_bound).

Bit-exact outputs (no bound): the weight conversion; every transpose of the GPU module (fp16(scale x) is one rounding for an
fp32 source, and the scales used, 1 and 0.25, are powers of two, so that the product is exact for an fp16 source as well); hi and
lo of the column-scale split without cs and with alpha == 1.  Their reference is x.half() and (x - x.half().float()).half() in
fp32 (split16).

Measured on the MI355X (worst err / bound per path, tests/test_trainops_kernels_gpu.py -s): see RATIOS below.
"""
import torch

F64, F32, F16 = torch.float64, torch.float32, torch.float16
EPS = 2.0 ** -24
H_EPS, H_SUB = 2.0 ** -11, 2.0 ** -24
LN_EPS = 1e-5
LN_ALPHA, LN_OUT_SCALE = 0.75, 0.3          # alpha and out_scale of the LayerNorm backward cases (no powers of two: the product
                                            # is one more fp32 rounding, and scaling before or after a rounding differs)

# worst |fp32 torch - fp64| / (EPS A) per output over the shapes below (printed by tests/test_trainops_ref_cpu.py); K = 4 x that,
# rounded up to the next integer
K_MEASURED = {
    "ln_y": 3.88, "ln_dx": 4.26, "ln_dgamma": 2.93, "ln_dbeta": 1.11, "colsum": 2.52, "gram": 2.31, "colscale": 0.99,
    "adamw_p": 3.67, "adamw_m": 2.59, "adamw_v": 3.10,
}
K = {
    "ln_y": 16.0, "ln_dx": 18.0, "ln_dgamma": 12.0, "ln_dbeta": 5.0, "colsum": 11.0, "gram": 10.0, "colscale": 4.0,
    "adamw_p": 15.0, "adamw_m": 11.0, "adamw_v": 13.0,
}

# shapes of the GPU module (the smallest that reach each path; the dispatch rules are mirrored in its docstring)
LN_FWD_SHAPES = ((1, 4), (5, 4), (7, 252), (7, 256), (6, 260), (6, 768), (6, 1024), (3, 1028), (3, 4096))       # (rows, D)
LN_GRID_ROWS = 768 * 16 + 37
LN_BWD_ROWS = (1, 15, 16, 17, 333)
LN_BWD_D = (4, 64, 252, 256, 260, 320, 768, 1024)
LN_BWD_GRID = ((LN_GRID_ROWS, 8), (LN_GRID_ROWS, 260))
LN_BWD2_D = (4, 192, 256)
COLSUM_SHAPES = ((1, 1, 1), (257, 300, 304), (256 * 49 + 3, 70, 70), (256 * 130, 64, 64))                         # (R, C, ld)
TRANSPOSE_SHAPES = ((1, 1, 1), (64, 64, 1), (65, 63, 1), (75, 130, 2))                                            # (R, C, batch)
GRAM_N = (1, 4, 63, 64, 68, 128, 130, 196)
COLSCALE_SHAPES = ((1, 1, 1, 0), (80, 64, 40, 0), (9, 6, 3, 0), (80, 64, 40, 1))                    # (rows, C, rpb, float offset)
ADAMW_SIZES = (4, 65536, 2 * 65536 + 148, 2 * 16384 + 5, 4096)      # the last one: grad a view at a 4-byte offset
ADAMW_GROUPS = (dict(lr=2e-3, weight_decay=0.01), dict(lr=5e-4, weight_decay=0.3))
ADAMW_BETAS, ADAMW_EPS = (0.9, 0.999), 1e-8

# worst err / bound per path on the MI355X.  The fp32 outputs sit at 0.12 .. 0.29: a quarter of the bound is the margin of 4 (five
# AdamW steps against the carried drift bound: 0.10 .. 0.24).  A
# value rounded to fp16 comes within 1 % of its bound (2^-11 |v| is the rounding's own worst case), hi + lo within a half (the
# remainder is below half an ulp of hi, which is 2^-12 .. 2^-11 of |v|).  The bit-equal paths have no bound: 0.
RATIOS = {
    "PolyWarmupAdamW five steps, adamw_multi_kernel (scalar) m": 0.164,
    "PolyWarmupAdamW five steps, adamw_multi_kernel (scalar) p": 0.103,
    "PolyWarmupAdamW five steps, adamw_multi_kernel (scalar) v": 0.219,
    "PolyWarmupAdamW five steps, adamw_multi_kernel (vector) m": 0.216,
    "PolyWarmupAdamW five steps, adamw_multi_kernel (vector) p": 0.114,
    "PolyWarmupAdamW five steps, adamw_multi_kernel (vector) v": 0.24, "adamw_multi_kernel (scalar) m": 0.249,
    "adamw_multi_kernel (scalar) p": 0.245, "adamw_multi_kernel (scalar) v": 0.265, "adamw_multi_kernel (vector) m": 0.25,
    "adamw_multi_kernel (vector) p": 0.22, "adamw_multi_kernel (vector) v": 0.276, "colscale_split_kernel<1>": 0.245,
    "colscale_split_kernel<1> fp16": 0.988, "colscale_split_kernel<1> hi+lo": 0.5, "colscale_split_kernel<4>": 0.245,
    "colscale_split_kernel<4> fp16": 0.988, "colscale_split_kernel<4> hi+lo": 0.5, "colsum_partial_kernel<__half>": 0.291,
    "colsum_partial_kernel<__half> round16": 0.991, "colsum_partial_kernel<float>": 0.291,
    "colsum_partial_kernel<float> round16": 0.991, "convert_weights_kernel (bit-equal)": 0, "layernorm_kernel<16>": 0.153,
    "layernorm_kernel<16> fp16": 0.99, "layernorm_kernel<16> hi+lo": 0.203, "layernorm_kernel<1>": 0.118,
    "layernorm_kernel<1> fp16": 0.993, "layernorm_kernel<1> hi+lo": 0.145, "layernorm_kernel<4>": 0.205,
    "layernorm_kernel<4> fp16": 0.994, "layernorm_kernel<4> hi+lo": 0.309, "ln_bwd_kernel<16> dbeta": 0.221,
    "ln_bwd_kernel<16> dgamma": 0.194, "ln_bwd_kernel<16> dx": 0.183, "ln_bwd_kernel<16> dx fp16": 0.994,
    "ln_bwd_kernel<4, true> dbeta": 0.186, "ln_bwd_kernel<4, true> dgamma": 0.128, "ln_bwd_kernel<4, true> dx": 0.204,
    "ln_bwd_kernel<4, true> dx fp16": 0.995, "ln_bwd_kernel<4> dbeta": 0.186, "ln_bwd_kernel<4> dgamma": 0.126,
    "ln_bwd_kernel<4> dx": 0.17, "ln_bwd_kernel<4> dx fp16": 0.994, "sigmoid_gram_bwd_kernel (element-wise) fp16": 0.968,
    "sigmoid_gram_bwd_kernel (element-wise) hi+lo": 0.496,
    "sigmoid_gram_bwd_kernel (element-wise, off-diagonal tiles) fp16": 0.989,
    "sigmoid_gram_bwd_kernel (element-wise, off-diagonal tiles) hi+lo": 0.494, "sigmoid_gram_bwd_kernel (vector) fp16": 0.971,
    "sigmoid_gram_bwd_kernel (vector) hi+lo": 0.478, "sigmoid_gram_bwd_kernel (vector, off-diagonal tiles) fp16": 0.993,
    "sigmoid_gram_bwd_kernel (vector, off-diagonal tiles) hi+lo": 0.499, "transpose_f16_kernel<__half> (bit-equal)": 0,
    "transpose_f16_kernel<float> (bit-equal)": 0,
}


# ---------------------------------------------------------------------------------------------------------------------
# fp16 helpers

def split16(x):
    """fp32 -> (hi, lo) fp16 as the kernels form them: hi = fp16(x), lo = fp16(x - hi) with the difference taken in fp32."""
    x = x.to(F32)
    hi = x.half()
    return hi, (x - hi.float()).half()


def h_bound(v, b32=0.0):
    """Bound of fp16(v') against v for an fp32 value v' within b32 of v."""
    return b32 * (1 + H_EPS) + torch.clamp(H_EPS * v.abs(), min=H_SUB)


def dx16_bound(dx, b32, out_scale=LN_OUT_SCALE):
    """Bound of fp16(fl32(out_scale dx')) against out_scale dx for an fp32 dx' within b32 of dx: the product is one more fp32
    rounding (EPS of its value), then the fp16 rounding."""
    v = out_scale * dx
    return h_bound(v, abs(out_scale) * b32 + EPS * (v.abs() + abs(out_scale) * b32))


def hl_bound(v, b32=0.0):
    """Bound of hi + lo against v for hi, lo = split16(v'), v' within b32 of v."""
    return b32 * (1 + 2.0 ** -22) + torch.clamp(2.0 ** -22 * v.abs(), min=H_SUB)


# ---------------------------------------------------------------------------------------------------------------------
# inputs (seeded; fp32 unless said otherwise)

def _gen(*key):
    s = 12345
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def ln_inputs(rows, D, seed=0):
    """x: rows with a mean offset of 0.5 and a per-row scale spread over two decades (0.1 .. 10); dy, dyb: fp16-representable, the
    last row and the last four columns four times as large as the rest; gammas sign-mixed; add."""
    g = _gen(rows, D, seed)
    scale = 10.0 ** (torch.rand(rows, 1, generator=g) * 2 - 1)
    if rows > 1:
        scale[0], scale[-1] = 0.1, 10.0
    x = 0.5 + scale * torch.randn(rows, D, generator=g)
    out = {"x": x.contiguous()}
    for name in ("dy", "dyb"):
        dy = torch.randn(rows, D, generator=g)
        dy[-1] *= 4
        dy[:, -4:] *= 4
        out[name] = dy.half().float()
    for name in ("w", "wb", "b"):
        out[name] = torch.randn(D, generator=g) * (1 + torch.arange(D) % 3)
    out["add"] = torch.randn(rows, D, generator=g)
    return out


def colsum_input(R, C, ld, seed=0):
    """(R, ld) fp32, fp16-representable, mostly positive (the sum is then of the size of sum |src|); columns [C, ld) are NaN."""
    g = _gen(R, C, ld, seed)
    src = torch.full((R, ld), float("nan"))
    src[:, :C] = (torch.randn(R, C, generator=g) + 1.0) * (1 + (torch.arange(C) % 5)[None, :])
    src[-1, :C] *= 8
    return src.half().float()


def colsum_cases(R):
    """(alpha, round16) of the column-sum cases: the sums rounded through fp16 are scaled to stay below the fp16 maximum."""
    s = 1.0 if R < 1000 else 2.0 ** -8
    return ((1.0, 0), (-0.3, 0), (s, 1), (-0.3 * s, 1))


def gram_inputs(B, n, seed=0):
    """AP in [0, 1] with exact 0, 1 and 0.5 planted (the corners included), dAP sign-mixed with a large last row and column."""
    g = _gen(B, n, seed)
    AP = torch.sigmoid(torch.randn(B, n, n, generator=g) * 3)
    flat = AP.view(B, -1)
    m = flat.shape[1]
    for k, v in enumerate((0.0, 1.0, 0.5)):
        flat[:, (torch.arange(m) % 7) == 2 * k + 1] = v
    flat[:, m - 1] = 0.5
    dAP = torch.randn(B, n, n, generator=g)
    dAP[:, -1, :] *= 8
    dAP[:, :, -1] *= 8
    return dAP.contiguous(), AP.contiguous()


def weight_values(shape, seed=0):
    """Magnitudes 1e-7 .. 1e3 (log-uniform: fp16 subnormals, underflow to zero and a lo of zero all occur), signs mixed, +0, -0."""
    g = _gen(*shape, seed)
    w = 10.0 ** (torch.rand(shape, generator=g) * 10 - 7) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    flat = w.view(-1)
    flat[0] = 0.0
    flat[-1] = -0.0
    return w


def colscale_inputs(rows, C, rpb, seed=0):
    """x (rows, C) over ten decades, cs (ceil(rows / rpb), C) in [0.5, 1.5)."""
    return weight_values((rows, C), seed=seed + 2), torch.rand((rows + rpb - 1) // rpb, C, generator=_gen(rows, C, rpb, seed)) + 0.5


def adamw_inputs(n, seed=0):
    """p, g, m, v fp32 with independent non-zero values; every 7th g and every 5th v zero (both at once every 35th)."""
    gen = _gen(n, seed)
    p, g, m = (torch.randn(n, generator=gen) for _ in range(3))
    m *= 0.1
    v = torch.rand(n, generator=gen) * 0.01
    g[::7] = 0.0
    v[::5] = 0.0
    return p, g, m, v


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm

def ln_stats(x, eps=LN_EPS):
    x = x.to(F64)
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return mean, rstd, (x - mean) * rstd


def ln_fwd(x, w, b, eps=LN_EPS):
    """-> y (rows, D) fp64, A."""
    _, rstd, xhat = ln_stats(x, eps)
    w, b = w.to(F64), b.to(F64)
    ax = x.to(F64).abs()
    return xhat * w + b, (ax + ax.mean(-1, keepdim=True)) * rstd * w.abs() + b.abs()


def ln_bwd(dys, ws, x, add=None, eps=LN_EPS, alpha=1.0):
    """dys, ws: one (rows, D) gradient and one gamma per norm (one or two norms of the same x).
    -> dict dx, A_dx, dgamma [per norm], dbeta, A_dgamma, A_dbeta."""
    _, rstd, xhat = ln_stats(x, eps)
    dys, ws = [d.to(F64) for d in dys], [w.to(F64) for w in ws]
    g = sum(d * w for d, w in zip(dys, ws))
    G = sum(d.abs() * w.abs() for d, w in zip(dys, ws))
    a = torch.zeros_like(g) if add is None else add.to(F64)
    m = lambda t: t.mean(-1, keepdim=True)
    X = rstd * (x.to(F64).abs() + m(x.to(F64).abs()))               # the companion of xhat = (x - mean x) rstd
    return {
        "dx": a + rstd * (g - m(g) - xhat * m(g * xhat)),
        "A_dx": a.abs() + rstd * (G + m(G) + X * m(G * X)),
        "dgamma": [alpha * (d * xhat).sum(0) for d in dys], "A_dgamma": [abs(alpha) * (d.abs() * X).sum(0) for d in dys],
        "dbeta": [alpha * d.sum(0) for d in dys], "A_dbeta": [abs(alpha) * d.abs().sum(0) for d in dys],
    }


# ---------------------------------------------------------------------------------------------------------------------
# column sum, transpose, sigmoid-Gram, column-scale split, weight conversion

def colsum(src, alpha=1.0):
    """src (R, C) -> out (C,) fp64 (before the optional fp16 rounding), A."""
    s = src.to(F64)
    return alpha * s.sum(0), abs(alpha) * s.abs().sum(0)


def transpose(src, oR, scale=1.0):
    """src (batch, R, C) fp32 or fp16 -> (hi, lo) fp16 (C, (batch - 1) oR + R): out[c, b oR + r] = split16(scale src[b, r, c]),
    zero between the batches.  One rounding: the fp32 product is exact for the scales in use (see the module docstring)."""
    batch, R, C = src.shape
    hi, lo = (torch.zeros(C, (batch - 1) * oR + R, dtype=F16) for _ in range(2))
    for b in range(batch):
        h, l = split16(src[b].float() * torch.tensor(scale, dtype=F32))
        hi[:, b * oR:b * oR + R], lo[:, b * oR:b * oR + R] = h.t(), l.t()
    return hi, lo


def gram(dAP, AP, scale=1.0):
    """-> S (B, n, n) fp64, A."""
    d, a = dAP.to(F64), AP.to(F64)
    z, az = d * a * (1 - a), d.abs() * a.abs() * (1 + a.abs())
    return scale * (z + z.transpose(1, 2)), abs(scale) * (az + az.transpose(1, 2))


def colscale(x, cs, rpb, alpha=1.0):
    """x (rows, C), cs (rows / rpb, C) or None -> y fp64, A."""
    y = alpha * x.to(F64)
    if cs is not None:
        y = y * cs.to(F64).repeat_interleave(rpb, 0)[:x.shape[0]]
    return y, y.abs()


def convert_weights(ws):
    """ws: the fp32 matrices of one operand (stacked along the rows) -> (hi, lo) (R, C) and (hiT, loT) (C, ceil64(R)), zero padded."""
    w = torch.cat(list(ws), 0)
    R, C = w.shape
    hi, lo = split16(w)
    ldT = (R + 63) // 64 * 64
    hiT, loT = torch.zeros(C, ldT, dtype=F16), torch.zeros(C, ldT, dtype=F16)
    hiT[:, :R], loT[:, :R] = hi.t(), lo.t()
    return hi, lo, hiT, loT


# ---------------------------------------------------------------------------------------------------------------------
# AdamW

def adamw(p, g, m, v, step, lr, weight_decay, betas=ADAMW_BETAS, eps=ADAMW_EPS, dt=F64):
    """One step (`step` = the number of this step, from 1) in dtype dt, the derived scalars formed in double and rounded to dt
    once, as the host does.  -> p, m, v, A_p, A_m, A_v."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    sc = lambda val: torch.tensor(val, dtype=F64).to(dt)
    decay, w1, w2, ss, bs, e, b2_ = sc(1.0 - lr * weight_decay), sc(1.0 - b1), sc(1.0 - b2), sc(lr / bc1), sc(bc2 ** 0.5), sc(eps), sc(b2)
    p, g, m, v = (t.to(dt) for t in (p, g, m, v))
    pd = p * decay
    mo = m + w1 * (g - m)
    vo = v * b2_ + (w2 * g) * g
    denom = vo.sqrt() / bs + e
    po = pd - ss * (mo / denom)
    A_m = m.abs() + w1 * (g.abs() + m.abs())
    return po, mo, vo, p.abs() * decay.abs() + ss * (A_m / denom), A_m, vo.abs()


def adamw_drift(E, state, g, step, lr, weight_decay, betas=ADAMW_BETAS, eps=ADAMW_EPS):
    """One step of the fp64 trajectory and of the bound of an fp32 trajectory against it.  state = (p, m, v) fp64 before the step,
    E = (E_p, E_m, E_v) with |fp32 state - state| <= E.  -> (p, m, v) after, E after.
    The fp32 step from the fp32 state is within the one-step bound K EPS A of the exact step from that same state, A taken at
    the fp32 state: A_m <= A_m(ref) + 2 E_m, A_v <= A_v(ref) + E_v, |p| <= |p_ref| + E_p.  The exact step maps the state errors
    to b1 E_m, b2 E_v, and for p to decay E_p + ss |m'/den' - m/den| <= decay E_p + ss (b1 E_m / den' + |m| dden / (den den')),
    where dden = b2 E_v / (sqrt(v) bs) bounds the change of the denominator (|sqrt a - sqrt b| <= |a - b| / sqrt b; an element
    with v == 0 never saw a gradient on either side, E_v == 0) and den' >= max(den - dden, eps) is the fp32 side's denominator."""
    p, m, v = state
    Ep, Em, Ev = E
    po, mo, vo, Ap, Am, Av = adamw(p, g, m, v, step, lr, weight_decay, betas, eps)
    b1, b2 = betas
    decay, ss, bs = abs(1.0 - lr * weight_decay), lr / (1.0 - b1 ** step), (1.0 - b2 ** step) ** 0.5
    Em2 = b1 * Em + K["adamw_m"] * EPS * (Am + 2 * Em)
    Ev2 = b2 * Ev + K["adamw_v"] * EPS * (Av + Ev)
    den = vo.sqrt() / bs + eps
    dden = torch.where(Ev > 0, b2 * Ev / (vo.sqrt().clamp(min=1e-300) * bs), torch.zeros_like(Ev))
    den_lo = (den - dden).clamp(min=eps * (1 - 1e-6))
    local = K["adamw_p"] * EPS * ((p.abs() + Ep) * decay + ss * (Am + 2 * Em) / den_lo)
    Ep2 = decay * Ep + ss * (b1 * Em / den_lo + mo.abs() * dden / (den * den_lo)) + local
    return (po, mo, vo), (Ep2, Em2, Ev2)


def poly_lr_mult(step, warmup_iter, warmup_ratio, max_iter, power):
    """utils/optimizer.py PolyWarmupAdamW._lr_mult at global step `step` (from 0)."""
    if step < warmup_iter:
        return 1 - (1 - step / warmup_iter) * (1 - warmup_ratio)
    return (1 - step / max_iter) ** power
