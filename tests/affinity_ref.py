"""fp64 reference and error model of csrc/affinity.hip (affinity weight, layer selection, Sinkhorn scale vectors, T_sym products,
materialised T_sym, min-max + bilinear up-sampling with the background score), for tests/test_affinity_ref_cpu.py (no GPU) and
tests/test_affinity_kernels_gpu.py.  Nothing here imports the oracle or needs a GPU.

Definitions (all evaluated in fp64 from the fp32 inputs, stage by stage; a stage gets its inputs, not another stage's output):
    affinity weight    W[b,i,j] = (sum_l wgt[b,l] maps_l[b,1+i,1+j]) seg[b,i,j]          (seg may be absent)
    layer selection    rowsum[b,l,i] = sum_j maps_l[b,1+i,1+j], A_l = sum_i rowsum, diff = -A, keep_l = [A_l >= mean_l A],
                       wgt = keep / (sum keep + fp32(1e-5))
    wc_matvec          v[b,j,k] = sum_i M[b,j,i] sin[b,i] X[b,i,k], M = W (transpose = 0) or W^T (transpose = 1);
                       out = 1 / v (recip) or alpha v sout[b,j] + add[b,j,k]
    column scale       c1 = 1 / colsum(W) = wc_matvec(X = 1, transpose, recip)
    Sinkhorn step      r = 1 / (W c), c_next = 1 / (W^T r); three rounds from c1 give (r, c) with T = diag(r) W diag(c)
    T_sym X            y1 = r (W (c X)), y2 = c (W^T (r X)), out = (y1 + y2) / 2
    T_sym              T[i,j] = (r_i W_ij c_j + c_i W_ji r_j) / 2;  trans_mat = T_sym T_sym;  refine = T_sym (T_sym V)
    up-sampling        stats = (min, max - min) per map; z = (R - min) / (fp32(1e-7) + (max - min)); half-pixel bilinear of z with
                       the taps and weights of csrc/resample.h (wc_bil_src: the source coordinate is fp32 arithmetic and is taken
                       as such, it decides the taps; wc_lerp4); bg = 1 - max_{k < nk[b]}; channels nk[b] <= k < C - 1 are zero.

Error model.  EPS = 2^-24.  Every fp32 output has the per-element bound
        K * EPS * (A + P) + P
A is the absolute-value companion of the output's formula in fp64, the same expression with every term replaced by its magnitude:
v: Av = sum |M| |sin| |X|; the linear form: |alpha| Av |sout| + |add|; a reciprocal 1 / v: Av / v^2 (sum |W||c| times the
reciprocal's magnitude: d(1/v) = dv / v^2); T_sym X: (|r| |W| (|c||X|) + |c| |W^T| (|r||X|)) / 2; the min-max: (|R| + |min|) / den,
carried through the four-tap lerp; bg: 1 + max_k A_k.
P is what the errors of a stage's inputs do to its output, for the composites whose inputs are themselves fp32 results with a
bound d (the Sinkhorn chain, T_sym (T_sym V), trans_mat): with every input replaced by |.| + d the companion grows by exactly
        Pv = sum (|M| + dM)(|sin| + dsin)(|X| + dX) - sum |M||sin||X|,
which bounds the change of v rigorously (no first-order truncation); for the linear form P = |alpha| (Pv (|sout| + dsout) +
Av dsout) + dadd, for a reciprocal P = Pv / (|v| (|v| - Pv)).  P is zero for a stage tested on its own.
K is MEASURED, not chosen: the worst |fp32 - fp64| / (EPS A) of a plain fp32 torch evaluation of the same stage over the shapes
and inputs of the GPU module, the larger of two emulations -- torch.matmul / torch.sum in fp32, and an explicit Python loop of fp32
vector additions along the reduced axis (one serial chain per output; the kernels' own serial chains run up to 128 FMAs in
matvec_cols_kernel, hw / 16 per thread) -- K_MEASURED below, printed by
tests/test_affinity_ref_cpu.py::test_bounds_admit_the_fp32_emulation, times the margin of 4 of tests/par_ref.py and
tests/trainops_ref.py, for the same reason: a fixed but different summation order, FMA contraction, 1.0f / x; rounded up: K below.
The serial loop sets K_MEASURED of every reduction (a chain of 2052 additions drifts further than any tree): the kernels, whose
chains are 16 times shorter and end in trees, are expected well below a quarter of the bound, see RATIOS.

Bit-exact outputs (no bound): the masks, boxes and V of box_masks; the zero fill; keep; stats' minimum; W of wc_aff_weight_c1
against W of wc_aff_weight.

Inputs.  W and the maps are positive and non-symmetric: uniform in [0.1, 1.1), not softmax rows, so that row and column sums are
not all near 1.  Dominant entries (3, 10, 30, 100 times their own value, i.e. a few times to 100 times the row mean) are planted
in the first and last row and column, on both sides of every 8-row block edge (aff_weight_colpart_kernel; every fourth of them is
a 32-row block edge of the sweeps), on both sides of the 4-row group edge, in columns 1023 / 1024 (the chunk seam) and on both
sides of the 4-column piece edges of threads 0, 1, 63, 64 (a wave edge) and 255: a dropped, doubled or misplaced element there
moves an output by far more than the bound.  X is sign-mixed for wc_matvec and T_sym X, and >= 0 (a box-masked CAM) for refine.

Measured on the MI355X (worst err / bound per path and output, tests/test_affinity_kernels_gpu.py -s): see RATIOS below.
"""
import torch

F64, F32, I32 = torch.float64, torch.float32, torch.int32
EPS = 2.0 ** -24
GUARD = float(torch.tensor(1e-7, dtype=F32))          # the 1e-7f of the min-max
KEEP_EPS = float(torch.tensor(1e-5, dtype=F32))       # the 1e-5f of the layer weights

# worst |fp32 torch - fp64| / (EPS A) per stage over the shapes below (printed by tests/test_affinity_ref_cpu.py); K = 4 x that,
# rounded up to the next integer
K_MEASURED = {"weight": 4.41, "rowsum": 16.78, "recip": 40.82, "matvec": 26.74, "tsym": 2.35, "stats": 0.64, "upsample": 3.48}
K = {"weight": 18.0, "rowsum": 68.0, "recip": 164.0, "matvec": 107.0, "tsym": 10.0, "stats": 3.0, "upsample": 14.0}

# shapes of the GPU module (the smallest that reach each path; the dispatch rules are mirrored in its docstring)
FUSED_HW = (4, 36, 64, 1024, 1028, 2048)
MATVEC_HW = (1, 3, 35, 113, 259, 2052)
BIG = 1024                                             # from here on: B = 1 and at most 2 maps
NMAPS = (1, 5, 6, 8, 10, 12)
MATVEC_K = (1, 4, 5, 9)
SEG_NMAPS, SEG_HW = (1, 6, 10), (35, 300)
TSYM_HW = (35, 68)
REFINE_CASES = ((5, 7, 3), (6, 8, 5), (32, 40, 3))     # (h, w, classes): hw = 35, 48, 1280
UPSAMPLE_SHAPES = ((3, 4, 37, 53), (4, 6, 64, 96), (5, 7, 5, 7), (8, 8, 3, 5), (1, 1, 9, 9))        # (h, w, H, W)
UPSAMPLE_K = (1, 3, 5)

# worst err / bound per path and output on the MI355X.  The element-wise outputs (W, T_sym, the up-sampled channels, the range) sit
# at 0.2 .. 0.27, the margin's quarter.  Every reduction sits at 0.02 .. 0.05, an eighth of that: its K_MEASURED is set by the serial
# loop emulation (one chain of up to 2052 additions, ratio 16 .. 41), while the kernels' chains are at most 128 long and end in
# trees -- against the torch.matmul emulation alone (ratio about 3) they would sit near a quarter as well.  The composites (three
# Sinkhorn rounds, T_sym T_sym, T_sym (T_sym V)) sit at 0.001 .. 0.006: their bound adds up every step's worst case, although the
# normalisation damps a scale error from step to step; the per-step rows above them are the sharp checks.  Bit-equal paths: 0.
RATIOS = {
    "aff_keep_kernel diff": 0.0269, "aff_keep_kernel keep (bit-equal)": 0, "aff_rowsum_kernel rowsum": 0.0401,
    "aff_sweep_kernel<0, 1> c_next": 0.0216, "aff_sweep_kernel<0, 1> c_next (from c)": 0.0112,
    "aff_sweep_kernel<0, 1> r": 0.0181, "aff_sweep_kernel<1, 1> r": 0.0181, "aff_sweep_kernel<2, 1> T_sym X": 0.0294,
    "aff_sweep_kernel<2, 1> y1": 0.0214, "aff_sweep_kernel<2, 2> T_sym X": 0.045, "aff_sweep_kernel<2, 2> y1": 0.0243,
    "aff_sweep_kernel<2, 3> T_sym X": 0.0298, "aff_sweep_kernel<2, 3> y1": 0.0357, "aff_sweep_kernel<2, 4> T_sym X": 0.0421,
    "aff_sweep_kernel<2, 4> y1": 0.031, "aff_weight_colpart_kernel W against aff_weight_kernel (bit-equal)": 0,
    "aff_weight_colpart_kernel c1": 0.0371, "aff_weight_colpart_kernel c1 (from the maps)": 0.0333,
    "aff_weight_kernel W": 0.27, "affinity_weight W": 0.205, "affinity_weight(seg_trans) W": 0.127,
    "affinity_weight(seg_trans) c1": 0.0165, "affinity_weight(seg_trans, keep) W": 0.168,
    "box_mask_kernel 80 x 85 (bit-equal)": 0, "box_mask_kernel slot -1, nroot > maxbox (bit-equal)": 0,
    "cam_upsample_kernel bg": 0.0981, "cam_upsample_kernel classes": 0.249, "matvec_cols_kernel K = 1": 0.0293,
    "matvec_cols_kernel K = 4": 0.0408, "matvec_cols_kernel K = 5": 0.0473, "matvec_cols_kernel K = 9": 0.0385,
    "matvec_cols_kernel recip K = 1": 0.0382, "matvec_cols_kernel recip K = 5": 0.0345, "matvec_cols_kernel recip c1": 0.0356,
    "matvec_rows_kernel K = 1": 0.0253, "matvec_rows_kernel K = 4": 0.0281, "matvec_rows_kernel K = 5": 0.0311,
    "matvec_rows_kernel K = 9": 0.0359, "matvec_rows_kernel recip K = 1": 0.0184, "matvec_rows_kernel recip K = 5": 0.0234,
    "refine hw = 1280": 0.00101, "refine hw = 1280 with c1": 0.00101, "refine hw = 35": 0.000811, "refine hw = 48": 0.00102,
    "refine hw = 48 with c1": 0.00102, "refined_minmax_kernel min (bit-equal)": 0, "refined_minmax_kernel range": 0.213,
    "sinkhorn_scales (fused) c": 0.00525, "sinkhorn_scales (fused) r": 0.00358, "sinkhorn_scales (wc_matvec) c": 0.00562,
    "sinkhorn_scales (wc_matvec) r": 0.0029, "trans_mat": 0.00157, "tsym_apply (fused) K = 5": 0.0326,
    "tsym_apply (fused) K = 8": 0.0438, "tsym_apply (fused) K = 9": 0.0403, "tsym_apply (wc_matvec) K = 3": 0.035,
    "tsym_apply (wc_matvec) K = 9": 0.0361, "tsym_kernel T_sym": 0.235,
    "upsample_with_bg against wc_cam_upsample (bit-equal)": 0,
}


def bound(name, A, P=None):
    """K EPS (A + P) + P."""
    if P is None:
        return K[name] * EPS * A
    return K[name] * EPS * (A + P) + P


# ---------------------------------------------------------------------------------------------------------------------
# inputs (seeded; fp32)

def _gen(*key):
    s = 24680
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def edge_rows(hw):
    """First and last row, both sides of the 4-row group edge and of every 8-row block edge (every fourth: a 32-row one)."""
    rows = {0, hw - 1, 3, 4}
    for e in range(8, hw, 8):
        rows.update((e - 1, e))
    return sorted(r for r in rows if 0 <= r < hw)


def edge_cols(hw):
    """First and last column, the chunk seam 1023 / 1024, both sides of the piece edges of threads 0, 1, 63, 64, 255."""
    cols = {0, hw - 1, 1023, 1024}
    for t in (1, 2, 63, 64, 65, 255, 256):
        cols.update((4 * t - 1, 4 * t, 1024 + 4 * t - 1, 1024 + 4 * t))
    return sorted(c for c in cols if 0 <= c < hw)


_FACTORS = (3.0, 10.0, 30.0, 100.0)


def plant(M, shift=0):
    """Multiplies one entry of every edge row (in an edge column) and one of every edge column (in an edge row) of M (B, n, n) by
    3, 10, 30 or 100, in place; `shift` moves the pairing, so that layers and images differ."""
    B, n, _ = M.shape
    rows, cols = edge_rows(n), edge_cols(n)
    for b in range(B):
        hit = set()
        for q, i in enumerate(rows):
            hit.add((i, cols[(q + b + shift) % len(cols)], _FACTORS[(q + shift) % 4]))
        for q, j in enumerate(cols):
            hit.add((rows[(7 * q + 3 + b + shift) % len(rows)], j, _FACTORS[(q + b + 1) % 4]))
        seen = set()
        for i, j, f in sorted(hit):
            if (i, j) not in seen:
                seen.add((i, j))
                M[b, i, j] *= f
    return M


def matrix_input(B, hw, seed=0):
    """W (B, hw, hw): positive, non-symmetric, planted."""
    return plant(torch.rand(B, hw, hw, generator=_gen(B, hw, seed)) + 0.1, shift=seed).contiguous()


# share of a row's mass that a layer leaves in the CLS column, low and high in turn (image b takes the list from entry b on, so that
# the images keep different layers): the interiors A_l = sum maps_l[1:,1:] of the two groups lie some 25 % to either side of their
# mean, several times what the planted entries move them (asserted by tests/test_affinity_ref_cpu.py)
CLS_MASS = (0.03, 0.45, 0.08, 0.40, 0.05, 0.48, 0.10, 0.42, 0.06, 0.46, 0.09, 0.44)


def maps_input(B, hw, nmaps, seed=0):
    """nmaps head-mean maps (B, L, L), L = hw + 1: a planted positive interior scaled by 1 - mass, a CLS row of 7 .. 8 and a CLS
    column that holds the layer's share (large against the interior: a kernel that reads row or column 0 is far off)."""
    maps = []
    for l in range(nmaps):
        g = _gen(B, hw, nmaps, l, seed)
        mass = torch.tensor([CLS_MASS[(l + b) % 12] for b in range(B)])[:, None, None]
        m = torch.empty(B, hw + 1, hw + 1)
        m[:, 1:, 1:] = plant(torch.rand(B, hw, hw, generator=g) + 0.1, shift=l + seed) * (1.0 - mass)
        m[:, 0, :] = 7.0 + torch.rand(B, hw + 1, generator=g)
        m[:, 1:, 0] = mass[:, :, 0] * hw * (0.5 + torch.rand(B, hw, generator=g))
        maps.append(m.contiguous())
    return maps


def seg_input(B, hw, seed=0):
    return (torch.rand(B, hw, hw, generator=_gen(B, hw, seed, 77)) * 0.95 + 0.05).contiguous()


def wgt_input(B, nmaps, seed=0):
    """Positive layer weights that are no powers of two and differ per image and layer."""
    return (torch.rand(B, nmaps, generator=_gen(B, nmaps, seed, 5)) * 0.3 + 0.02).contiguous()


def vec_input(B, hw, seed=0, lo=0.2, hi=3.0):
    """A positive scale vector (B, hw) over a decade."""
    return (torch.rand(B, hw, generator=_gen(B, hw, seed, 11)) * (hi - lo) + lo).contiguous()


def x_input(B, hw, Kc, seed=0):
    """Sign-mixed X (B, hw, K), every class different, the edge rows four times as large."""
    X = torch.randn(B, hw, Kc, generator=_gen(B, hw, Kc, seed, 13)) * (1.0 + torch.arange(Kc, dtype=F32))
    X[:, edge_rows(hw)] *= 4.0
    return X.contiguous()


def cams_input(P, h, w, seed=0):
    """P GradCAM-like maps in [0, 1] (P, h*w): a few bright blobs on a dim floor, each with maximum 1."""
    g = _gen(P, h, w, seed, 17)
    c = torch.rand(P, h, w, generator=g) * 0.3
    for p in range(P):
        for q in range(1 + p % 3):
            y, x = int(torch.randint(0, h, (1,), generator=g)), int(torch.randint(0, w, (1,), generator=g))
            c[p, max(y - 1, 0):y + 2, max(x - 2, 0):x + 2] = 0.6 + 0.4 * torch.rand(1, generator=g)
        c[p] /= c[p].max()
    return c.reshape(P, h * w).contiguous()


def refined_input(B, hw, Kc, seed=0):
    """R (B, hw, K) like refined CAMs (small positive values, a different offset and range per map); map 0 of the last image is
    constant (range 0: the 1e-7 guard decides), map K-1 of the first has one non-zero pixel."""
    g = _gen(B, hw, Kc, seed, 19)
    R = torch.rand(B, hw, Kc, generator=g) * (0.01 * (1.0 + torch.arange(Kc, dtype=F32))) + 0.003 * torch.rand(B, 1, Kc, generator=g)
    R[B - 1, :, 0] = 0.0123
    R[0, :, Kc - 1] = 0.0
    R[0, (2 * hw) // 3, Kc - 1] = 0.5
    return R.contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# affinity weight and layer selection

def aff_weight(maps, wgt, seg=None):
    """-> W (B, hw, hw) fp64, A."""
    wgt = wgt.to(F64)
    W = sum(wgt[:, l, None, None] * m[:, 1:, 1:].to(F64) for l, m in enumerate(maps))
    A = sum(wgt[:, l, None, None].abs() * m[:, 1:, 1:].to(F64).abs() for l, m in enumerate(maps))
    if seg is not None:
        W, A = W * seg.to(F64), A * seg.to(F64).abs()
    return W, A


def uniform_wgt(B, nmaps):
    """The normal branch's weights: fp32(1 / nmaps)."""
    return torch.full((B, nmaps), 1.0 / nmaps, dtype=F32)


def seg_weights(maps):
    """-> dict rowsum (B, nmaps, hw), A_rowsum, A_l (B, nmaps), A_A, diff, keep (bool), wgt (fp64 from the fp32 constant)."""
    inner = torch.stack([m[:, 1:, 1:].to(F64) for m in maps], 1)
    rowsum, A_rowsum = inner.sum(-1), inner.abs().sum(-1)
    A_l, A_A = rowsum.sum(-1), A_rowsum.sum(-1)
    keep = A_l >= A_l.mean(1, keepdim=True)
    n = keep.sum(1, keepdim=True).to(F64)
    return {"rowsum": rowsum, "A_rowsum": A_rowsum, "A_l": A_l, "A_A": A_A, "diff": -A_l, "keep": keep,
            "wgt": keep.to(F64) / (n + KEEP_EPS)}


def keep_separation(maps):
    """min_l |A_l - mean A| / bound(A_l): how far the layer decision is from ambiguity (inf for a single layer, where the mean
    is A_0 itself in any arithmetic)."""
    s = seg_weights(maps)
    if len(maps) == 1:
        return float("inf")
    mean = s["A_l"].mean(1, keepdim=True)
    # the mean's own error is at most the mean of the layers' bounds
    b = bound("rowsum", s["A_A"]) + bound("rowsum", s["A_A"]).mean(1, keepdim=True)
    return ((s["A_l"] - mean).abs() / b).min().item()


# ---------------------------------------------------------------------------------------------------------------------
# wc_matvec and what is built from it

def _z(t):
    return None if t is None else t.to(F64)


def matvec(W, X, sin=None, sout=None, add=None, alpha=1.0, recip=False, transpose=False,
           dW=None, dX=None, dsin=None, dsout=None, dadd=None):
    """W (B, hw, hw), X (B, hw, K), sin / sout (B, hw), add (B, hw, K); d*: bounds of the errors of these inputs (None: exact).
    -> out (B, hw, K) fp64, A, P."""
    W, X, sin, sout, add = _z(W), _z(X), _z(sin), _z(sout), _z(add)
    M = W.transpose(1, 2) if transpose else W
    aM, aX = M.abs(), X.abs()
    xs = X if sin is None else X * sin[:, :, None]
    axs = aX if sin is None else aX * sin.abs()[:, :, None]
    v, Av = M @ xs, aM @ axs
    if dW is None and dX is None and dsin is None:
        Pv = torch.zeros_like(v)
    else:
        pM = aM if dW is None else aM + (_z(dW).transpose(1, 2) if transpose else _z(dW))
        pX = aX if dX is None else aX + _z(dX)
        if sin is not None:
            pX = pX * (sin.abs() if dsin is None else sin.abs() + _z(dsin))[:, :, None]
        Pv = (pM @ pX - Av).clamp(min=0.0)
    if recip:
        room = v.abs() - Pv
        P = torch.where(room > 0, Pv / (v.abs() * room.clamp(min=1e-300)), torch.full_like(v, float("inf")))
        return 1.0 / v, Av / (v * v), P
    so = torch.ones_like(v[:, :, :1]) if sout is None else sout[:, :, None]
    dso = torch.zeros_like(so) if dsout is None else _z(dsout)[:, :, None]
    out, A = alpha * v * so, abs(alpha) * Av * so.abs()
    P = abs(alpha) * (Pv * (so.abs() + dso) + Av * dso)
    if add is not None:
        out, A = out + add, A + add.abs()
        if dadd is not None:
            P = P + _z(dadd)
    return out, A, P


def col_scale(W, dW=None):
    """c1 = 1 / colsum(W) -> c (B, hw), A, P."""
    B, hw, _ = W.shape
    c, A, P = matvec(W, torch.ones(B, hw, 1, dtype=F64), recip=True, transpose=True, dW=dW)
    return c[:, :, 0], A[:, :, 0], P[:, :, 0]


def row_scale(W, c, dc=None, dW=None):
    """r = 1 / (W c) -> r (B, hw), A, P."""
    r, A, P = matvec(W, c[:, :, None], recip=True, dX=None if dc is None else dc[:, :, None], dW=dW)
    return r[:, :, 0], A[:, :, 0], P[:, :, 0]


def col_scale_next(W, r, dr=None, dW=None):
    """c_next = 1 / (W^T r) -> c (B, hw), A, P."""
    c, A, P = matvec(W, r[:, :, None], recip=True, transpose=True, dX=None if dr is None else dr[:, :, None], dW=dW)
    return c[:, :, 0], A[:, :, 0], P[:, :, 0]


def sinkhorn(W, rounds=3, c1=None, dc1=None):
    """The fp64 chain c1, r1, c2, r2, c3, r3 from the fp32 W -> (r, c, dr, dc): the scale vectors of T = diag(r) W diag(c) and
    their composed bounds (every step: its own K EPS A plus what the previous step's bound does to it).  c1 / dc1: a first
    column scale and its bound from elsewhere (wc_aff_weight_c1)."""
    if c1 is None:
        c, A, P = col_scale(W)
        dc = bound("recip", A, P)
    else:
        c, dc = c1.to(F64), dc1
    r = dr = None
    for it in range(rounds):
        r, A, P = row_scale(W, c, dc)
        dr = bound("recip", A, P)
        if it < rounds - 1:
            c, A, P = col_scale_next(W, r, dr)
            dc = bound("recip", A, P)
    return r, c, dr, dc


def tsym_apply(W, r, c, X, dr=None, dc=None, dX=None):
    """-> dict out, A, P, y1, A_y1, P_y1 (y1 = r (W (c X)), the fused sweep's first half)."""
    y1, A1, P1 = matvec(W, X, sin=c, sout=r, dsin=dc, dsout=dr, dX=dX)
    y2, A2, P2 = matvec(W, X, sin=r, sout=c, dsin=dr, dsout=dc, dX=dX, transpose=True)
    return {"out": 0.5 * (y1 + y2), "A": 0.5 * (A1 + A2), "P": 0.5 * (P1 + P2), "y1": y1, "A_y1": A1, "P_y1": P1}


def tsym_mat(W, r, c, dr=None, dc=None):
    """-> T (B, hw, hw) fp64, A, P."""
    W, r, c = _z(W), _z(r), _z(c)
    T = 0.5 * (r[:, :, None] * W * c[:, None, :] + c[:, :, None] * W.transpose(1, 2) * r[:, None, :])
    ar, ac, aW = r.abs(), c.abs(), W.abs()
    A = 0.5 * (ar[:, :, None] * aW * ac[:, None, :] + ac[:, :, None] * aW.transpose(1, 2) * ar[:, None, :])
    if dr is None and dc is None:
        return T, A, torch.zeros_like(T)
    pr, pc = ar + (0 if dr is None else dr), ac + (0 if dc is None else dc)
    P = 0.5 * (pr[:, :, None] * aW * pc[:, None, :] + pc[:, :, None] * aW.transpose(1, 2) * pr[:, None, :]) - A
    return T, A, P.clamp(min=0.0)


def trans_mat(W):
    """T_sym T_sym from the fp32 W -> out (B, hw, hw) fp64, its composed bound."""
    r, c, dr, dc = sinkhorn(W)
    T, A, P = tsym_mat(W, r, c, dr, dc)
    dT = bound("tsym", A, P)
    out, A, P = matvec(T, T, dW=dT, dX=dT)
    return out, bound("matvec", A, P)


def refine(W, V, c1=None, dc1=None):
    """T_sym (T_sym V) from the fp32 W and V (B, hw, K) -> out fp64, its composed bound."""
    r, c, dr, dc = sinkhorn(W, c1=c1, dc1=dc1)
    a = tsym_apply(W, r, c, V, dr, dc)
    b = tsym_apply(W, r, c, a["out"], dr, dc, dX=bound("matvec", a["A"], a["P"]))
    return b["out"], bound("matvec", b["A"], b["P"])


# ---------------------------------------------------------------------------------------------------------------------
# up-sampling

def bil_taps(out_n, in_n, half=0.5):
    """wc_bil_src of csrc/resample.h for every destination index: the source coordinate max(scale (d + 0.5) - 0.5, 0) in fp32 with
    scale = fp32(in) / fp32(out), each operation rounded on its own.  -> i0, i1 (long), l1 (fp64 of the fp32 weight).
    `half`: the half-pixel offset (0.5; 0 is the planted fault)."""
    scale = torch.tensor(float(in_n), dtype=F32) / torch.tensor(float(out_n), dtype=F32)
    d = torch.arange(out_n, dtype=F32)
    s = (scale * (d + half) - half).clamp(min=0.0)
    i0 = s.to(torch.int64).clamp(max=in_n - 1)
    i1 = i0 + (i0 < in_n - 1).to(torch.int64)
    return i0, i1, (s - i0.to(F32)).to(F64)


def minmax(R, guard=GUARD):
    """R (B, hw, K) -> stats (B, K, 2) fp64 = (min, max - min), A_stats, z (B, hw, K) = (R - min) / (guard + range), A_z."""
    R = R.to(F64)
    mn, mx = R.min(1).values, R.max(1).values
    stats = torch.stack([mn, mx - mn], -1)
    A_stats = torch.stack([torch.zeros_like(mn), mx.abs() + mn.abs()], -1)
    den = guard + (mx - mn)
    return stats, A_stats, (R - mn[:, None]) / den[:, None], (R.abs() + mn.abs()[:, None]) / den[:, None]


def upsample(R, nk, h, w, H, Wd, C=None, guard=GUARD, half=0.5, bg_all=False):
    """-> dict stats, A_stats, cams (B, C, H, W) fp64, A (same shape; 0 where the output is the exact zero fill), zero (bool mask
    of the zero fill).  guard / half / bg_all: the planted faults (guard 0, no half-pixel offset, bg over all K maps)."""
    B, hw, Kc = R.shape
    C = Kc + 1 if C is None else C
    stats, A_stats, z, Az = minmax(R, guard)
    y0, y1, ly = bil_taps(H, h, half)
    x0, x1, lx = bil_taps(Wd, w, half)
    z, Az = z.reshape(B, h, w, Kc), Az.reshape(B, h, w, Kc)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]

    def lerp(t):
        a, b_, c_, d = t[:, y0][:, :, x0], t[:, y0][:, :, x1], t[:, y1][:, :, x0], t[:, y1][:, :, x1]
        return (1 - ly) * ((1 - lx) * a + lx * b_) + ly * ((1 - lx) * c_ + lx * d)

    up, Aup = lerp(z).permute(0, 3, 1, 2), lerp(Az).permute(0, 3, 1, 2)          # (B, K, H, W)
    cams, A = torch.zeros(B, C, H, Wd, dtype=F64), torch.zeros(B, C, H, Wd, dtype=F64)
    zero = torch.zeros(B, C, H, Wd, dtype=torch.bool)
    for b in range(B):
        n = int(nk[b])
        cams[b, 1:1 + n], A[b, 1:1 + n] = up[b, :n], Aup[b, :n]
        zero[b, 1 + n:] = True
        m = Kc if bg_all else n
        cams[b, 0], A[b, 0] = 1.0 - up[b, :m].max(0).values, 1.0 + Aup[b, :m].max(0).values
    return {"stats": stats, "A_stats": A_stats, "cams": cams, "A": A, "zero": zero}


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulations (K_MEASURED): mode "matmul" = torch.matmul / torch.sum in fp32, "loop" = a serial chain of fp32 vector additions
# along the reduced axis

def _sum32(terms, mode):
    """Sum over dim 0 of an fp32 tensor."""
    if mode == "matmul":
        return terms.sum(0)
    acc = torch.zeros_like(terms[0])
    for t in terms:
        acc = acc + t
    return acc


def aff_weight32(maps, wgt, seg, mode):
    W = _sum32(torch.stack([wgt[:, l, None, None] * m[:, 1:, 1:] for l, m in enumerate(maps)]), mode)
    return W if seg is None else W * seg


def seg_weights32(maps, mode):
    """-> rowsum (B, nmaps, hw), A_l (B, nmaps) in fp32."""
    inner = torch.stack([m[:, 1:, 1:] for m in maps], 1)                      # (B, nmaps, hw, hw)
    rowsum = _sum32(inner.permute(3, 0, 1, 2).contiguous(), mode)
    return rowsum, _sum32(rowsum.permute(2, 0, 1).contiguous(), mode)


def matvec32(W, X, sin=None, sout=None, add=None, alpha=1.0, recip=False, transpose=False, mode="matmul"):
    M = W.transpose(1, 2) if transpose else W
    xs = X if sin is None else X * sin[:, :, None]
    if mode == "matmul":
        v = M @ xs
    else:
        Mc = M.transpose(1, 2).contiguous()              # Mc[:, i] = column i of M: one vector addition per reduced index
        v = torch.zeros_like(xs)
        for i in range(M.shape[2]):
            v = v + Mc[:, i, :, None] * xs[:, i, None, :]
    if recip:
        return 1.0 / v
    v = v * torch.tensor(alpha, dtype=F32)
    if sout is not None:
        v = v * sout[:, :, None]
    return v if add is None else v + add


def tsym_apply32(W, r, c, X, mode):
    y1 = matvec32(W, X, sin=c, sout=r, mode=mode)
    return 0.5 * (y1 + matvec32(W, X, sin=r, sout=c, transpose=True, mode=mode)), y1


def tsym_mat32(W, r, c):
    return 0.5 * (r[:, :, None] * W * c[:, None, :] + c[:, :, None] * W.transpose(1, 2) * r[:, None, :])


def upsample32(R, nk, h, w, H, Wd, C=None):
    """-> stats (B, K, 2), cams (B, C, H, W) in fp32, the formulas of cam_upsample_kernel and wc_lerp4."""
    B, hw, Kc = R.shape
    C = Kc + 1 if C is None else C
    mn, mx = R.min(1).values, R.max(1).values
    rng = mx - mn
    z = ((R - mn[:, None]) / (torch.tensor(GUARD, dtype=F32) + rng)[:, None]).reshape(B, h, w, Kc)
    y0, y1, ly = bil_taps(H, h)
    x0, x1, lx = bil_taps(Wd, w)
    ly, lx = ly.to(F32)[None, :, None, None], lx.to(F32)[None, None, :, None]
    a, b_, c_, d = z[:, y0][:, :, x0], z[:, y0][:, :, x1], z[:, y1][:, :, x0], z[:, y1][:, :, x1]
    hy, hx = 1.0 - ly, 1.0 - lx
    up = (hy * (hx * a + lx * b_) + ly * (hx * c_ + lx * d)).permute(0, 3, 1, 2)
    cams = torch.zeros(B, C, H, Wd, dtype=F32)
    for b in range(B):
        n = int(nk[b])
        cams[b, 1:1 + n] = up[b, :n]
        cams[b, 0] = 1.0 - up[b, :n].max(0).values
    return torch.stack([mn, rng], -1), cams


def nk_input(B, Kc, C):
    """Class counts 1 .. min(K, C - 1), mixed within the batch, the first image with the most."""
    top = min(Kc, C - 1)
    return torch.tensor([top - b % top for b in range(B)], dtype=I32)
