"""fp64 reference of multi-head self-attention for the kernel tests of csrc/attention.hip, csrc/attention_bwd.hip and the
GradCAM column sums of csrc/gradcam.hip.

Conventions are the kernels': packed qkv (B*L, 3E) fp16, E = H*DH, q pre-scaled by log2(e)/sqrt(DH), so the scores
s = q k^T are in the exp2 domain, P = exp2(s - lse) with lse the base-2 log-sum-exp of a score row.  dO (B*L, E) fp16,
o32 (B*L, E) f32, lse (B, H, L) f32.  Gradients are w.r.t. the UNSCALED in-projection output:
    dS = P * (dP - delta),  dP = dO v^T,  delta = rowsum(dO * O)
    dq = dS k / sqrt(DH),   dk = dS^T q_s / log2(e),   dv = P^T dO        (q_s: the pre-scaled q)
Everything is torch float64, one (b, h) at a time, on a subset of rows so that the large shapes stay cheap.

Error model (per element; U = 2^-24 the fp32 unit roundoff, U16 = 2^-11 the fp16 one):
  exponent   eps = (DH + 8) U (sum_d |q_d k_d| + |c|) + 2^-22      (log2 units; c = the row max or lse subtracted)
             A dot product of DH fp16 x fp16 products (exact in fp32) and the subtracted constant takes at most DH + 1
             roundings of a partial sum bounded by sum|terms| + |c|; the forward's separate subtraction s - m, the mean
             kernel's two-part lse and the product roundings of the delta kernel add at most 7 more.  v_exp_f32 is
             accurate to 1 ulp: a relative 2^-23, i.e. log2(1 + 2^-23) < 2^-22 in the exponent.  A perturbation eps of
             the exponent moves p by p ln2 eps.
  fp16 P/dS  P (forward, dv) and dS (dq, dk) are fp16 MFMA operands: 2^-11 relative per term, plus 2^-25 absolute for
             fp16 subnormals (half their spacing 2^-24).  In the forward p is relative to the running maximum and later
             scaled by exp2(m_t - m) <= 1, and the denominator l = sum exp2(s - m) >= 1, so the absolute part stays
             <= 2^-25 |v| / l per term of the normalised output.
  accumulate a sum of n terms in fp32 in any order (MFMA chains, partial sums, the online rescale of every 64-key tile)
             errs by at most (n - 1) U sum|terms| (first-order gamma_n).  n = L keys plus one rescale per 64-key tile plus
             <= 64 partials of the row path plus the final products: n = L + ceil(L / 64) + 80 in the forward, n = L + 8
             for the backward / column-sum chains.  The forward pays it twice: numerator and denominator.
  lse        lse = m + log2(l): the exponent errors weighted by P, the relative error of l (n U, i.e. n U log2(e) in
             log2 units), the final add and log2f (2 U (|lse| + |m|) + 2^-22).
  mean       the kernel folds -lse into one MFMA step as fp16 hi + lo: |lse - hi - lo| <= 2^-22 |lse| + 2^-25; the
             H-head sum and the 1/H scale add (H + 3) U relative.
  fp16 out   one fp16 ulp of the reference on top (ulp16)."""
import math

import torch

F64 = torch.float64
U = 2.0 ** -24
U16 = 2.0 ** -11
SUB16 = 2.0 ** -25
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
EDGE_MAX = 8            # ATT_EDGE_MAX of csrc/attention.hip


def qscale(DH):
    return LOG2E / math.sqrt(DH)


def origin(L):
    """First tiled query row of the forward / mean (attn_origin): a remainder L % 128 in [1, 8] is done off the tiles."""
    r = L % 128
    return r if (L >= 128 and 0 < r <= EDGE_MAX) else 0


def ulp16(r):
    a = r.abs().clamp(min=2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def acc_n_fwd(L):
    return L + (L + 63) // 64 + 80


def acc_n_bwd(L):
    return L + 8


# ---------------------------------------------------------------------------------------------------------------------
# inputs

def edge_keys(L):
    """Keys where a kernel that mishandles its tiles goes wrong: 0, L-1, the first L % 64 (the 8-wave forward's VALU keys),
    and both sides of every 64-key tile edge counted from 0 and from L % 64."""
    ks = {0, L - 1} | set(range(min(L % 64, EDGE_MAX)))
    for o in {0, L % 64}:
        for e in range(o + 64, L, 64):
            ks |= {e - 1, e}
    return sorted(k for k in ks if 0 <= k < L)


def check_rows(L, n_rand=24, seed=0):
    """Rows to check: every row below the tile origin, both sides of every 64 / 128 boundary (from 0 and from the
    origin), the last 40 rows and a seeded random sample."""
    rs = set(range(origin(L))) | set(range(L % 64 if L % 64 <= EDGE_MAX else 0))
    for o in {0, origin(L), L % 64}:
        for e in range(o + 64, L, 64):
            rs |= {e - 1, e}
    rs |= set(range(max(0, L - 40), L))
    g = torch.Generator().manual_seed(seed)
    rs |= set(torch.randint(0, L, (n_rand,), generator=g).tolist())
    return torch.tensor(sorted(rs), dtype=torch.long)


def planted_rows(L):
    """The rows of check_rows that make_inputs gives a dominant key (all but the random sample)."""
    return check_rows(L, n_rand=0)


def make_inputs(B, L, H, DH, seed=0, plant=True, dscale=1.0, cls_zero=False):
    """qkv (B*L, 3E) fp16 with q pre-scaled, dO (B*L, E) fp16.  With `plant`, the keys of edge_keys(L) get 4x the norm and
    every row of planted_rows(L) is aimed at one of them (cycling) with a score gap of log2(L) + 4: that key then carries
    ~90 % of the row's probability, so dropping it or counting it twice moves O by O(|v|), not O(|v| / L).  dscale scales
    dO (GradCAM carries gradients up to 2^12 larger); cls_zero zeroes dO of token 0 (the colsum precondition)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, L, DH, generator=g, dtype=F64) * qscale(DH)
    k = torch.randn(B, H, L, DH, generator=g, dtype=F64)
    v = torch.randn(B, H, L, DH, generator=g, dtype=F64)
    if plant:
        keys = edge_keys(L)
        k[:, :, keys] *= 4.0
        gap = math.log2(L) + 4.0
        for n, i in enumerate(planted_rows(L).tolist()):
            j = keys[(n + 1) % len(keys)]
            kj = k[:, :, j]
            q[:, :, i] = gap * kj / (kj * kj).sum(-1, keepdim=True)
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H * DH).half()
    dO = torch.randn(B * L, H * DH, generator=g, dtype=F64) * dscale
    if cls_zero:
        dO.view(B, L, -1)[:, 0] = 0
    return qkv, dO.half()


def heads(qkv, B, L, H, DH):
    """(q_s, k, v) each (B, H, L, DH) float64 from the packed fp16 qkv."""
    x = qkv.double().reshape(B, L, 3, H, DH).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def per_head(t, B, L, H, DH):
    """(B*L, E) -> (B, H, L, DH) float64."""
    return t.double().reshape(B, L, H, DH).permute(0, 2, 1, 3)


def _eps(qs, k, c, DH):
    """exponent error (log2 units) of exp2(q_s k^T - c): rows of qs x rows of k, c per row of qs."""
    return (DH + 8) * U * (qs.abs() @ k.abs().T + c.abs()[:, None]) + 2.0 ** -22


# ---------------------------------------------------------------------------------------------------------------------
# forward

def fwd_head(qs, k, v, rows, DH):
    """One head: O (R, DH), lse (R,), P (R, L), and the bounds of O and lse, for the query rows `rows`."""
    L = k.shape[0]
    s = qs[rows] @ k.T
    m = s.max(1).values
    p = torch.exp2(s - m[:, None])
    l = p.sum(1)
    P = p / l[:, None]
    O = P @ v
    lse = m + torch.log2(l)
    eps = _eps(qs[rows], k, m, DH)
    n = acc_n_fwd(L)
    va = v.abs()
    bO = ((U16 + 2 * n * U) * P) @ va + LN2 * ((P * eps) @ va + (P * eps).sum(1, keepdim=True) * O.abs()) \
        + (SUB16 / l)[:, None] * va.sum(0)[None]
    blse = (P * eps).sum(1) + n * U * LOG2E + 2 * U * (lse.abs() + m.abs()) + 2.0 ** -22
    return O, lse, P, bO, blse


def fwd(qkv, B, L, H, DH, rows=None, bh=None):
    """-> O (n, R, DH), lse (n, R), bO, blse for the (b, h) pairs `bh` (default all) and query rows `rows` (default all)."""
    qs, k, v = heads(qkv, B, L, H, DH)
    rows = torch.arange(L) if rows is None else rows
    bh = [(b, h) for b in range(B) for h in range(H)] if bh is None else bh
    outs = [fwd_head(qs[b, h], k[b, h], v[b, h], rows, DH) for b, h in bh]
    return tuple(torch.stack([o[i] for o in outs]) for i in (0, 1, 3, 4))


def mean(qkv, B, L, H, DH, imgs, rows):
    """Head-mean of the probabilities, (len(imgs), R, L), and its bound; uses the exact lse (the bound includes the
    forward's lse error)."""
    qs, k, v = heads(qkv, B, L, H, DH)
    M = torch.zeros(len(imgs), len(rows), L, dtype=F64)
    bM = torch.zeros_like(M)
    for i, b in enumerate(imgs):
        for h in range(H):
            _, lse, P, _, blse = fwd_head(qs[b, h], k[b, h], v[b, h], rows, DH)
            eps = _eps(qs[b, h, rows], k[b, h], lse, DH)
            M[i] += P
            bM[i] += P * LN2 * (eps + (blse + 2.0 ** -22 * lse.abs() + SUB16)[:, None])
    M /= H
    bM = bM / H + (H + 3) * U * M
    return M, bM


def fwd_exact(qkv, B, L, H, DH):
    """Exact O (B*L, E) and lse (B, H, L) in float64."""
    qs, k, v = heads(qkv, B, L, H, DH)
    P = torch.softmax((qs @ k.transpose(-1, -2)) * LN2, -1)
    lse = torch.logsumexp((qs @ k.transpose(-1, -2)) * LN2, -1) * LOG2E
    O = (P @ v).permute(0, 2, 1, 3).reshape(B * L, H * DH)
    return O, lse


# ---------------------------------------------------------------------------------------------------------------------
# backward

def _blocks(qs, k, v, dO, o, lse, qi, kj, DH, fp16_ds, fe=None):
    """P, dS and the error bound of each dS entry on queries qi x keys kj of one head (kernel's own lse / O).  fe: the
    forward's (bO, blse) on every query, when o / lse are the exact ones and the kernel was fed its own forward: the lse
    error enters the exponent, the O error delta (|d delta| <= sum_d |dO_d| bO_d)."""
    s = qs[qi] @ k[kj].T
    P = torch.exp2(s - lse[qi, None])
    dP = dO[qi] @ v[kj].T
    delta = (dO[qi] * o[qi]).sum(1)
    dS = P * (dP - delta[:, None])
    eps = _eps(qs[qi], k[kj], lse[qi], DH)
    G = dO[qi].abs() @ v[kj].abs().T
    D = (dO[qi] * o[qi]).abs().sum(1)
    if fe is not None:
        eps = eps + fe[1][qi, None]
        D = D + (dO[qi].abs() * fe[0][qi]).sum(1) / ((DH + 8) * U)
    edS = P * (LN2 * eps * (dP - delta[:, None]).abs() + (DH + 8) * U * (G + 2 * D[:, None]))
    edS = edS + ((U16 + 2 * U) * dS.abs() + SUB16 if fp16_ds else 2 * U * dS.abs())
    return P, dS, eps, edS


def bwd_head(qs, k, v, dO, o, lse, rows, DH, fe=None):
    """One head: dq, dk, dv (R, DH) on `rows` (as queries for dq, as keys for dk / dv) and their bounds."""
    L = k.shape[0]
    n = acc_n_bwd(L)
    a = torch.arange(L)
    sq = 1.0 / math.sqrt(DH)
    P, dS, eps, edS = _blocks(qs, k, v, dO, o, lse, rows, a, DH, True, fe)
    dq = dS @ k * sq
    bdq = sq * (edS @ k.abs() + n * U * dS.abs() @ k.abs()) + 3 * U * dq.abs()
    P, dS, eps, edS = _blocks(qs, k, v, dO, o, lse, a, rows, DH, True, fe)
    dk = dS.T @ qs * LN2
    bdk = LN2 * (edS.T @ qs.abs() + n * U * dS.abs().T @ qs.abs()) + 3 * U * dk.abs()
    dv = P.T @ dO
    bdv = ((U16 + n * U + LN2 * eps) * P + SUB16).T @ dO.abs() + 3 * U * dv.abs()
    return dq, dk, dv, bdq, bdk, bdv


def bwd(qkv, dO, o32, lse, B, L, H, DH, rows=None, bh=None, exact=False, fwd_err=False):
    """-> dq, dk, dv (n, R, DH) and their bounds for the (b, h) pairs `bh` on `rows`.  o32 / lse are the kernel's own
    forward outputs; exact=True uses the exact fp64 O and lse instead (o32 / lse may then be None), and with fwd_err the
    bounds also cover a kernel fed by the forward kernel's o32 / lse (their bounds propagated through delta and P)."""
    qs, k, v = heads(qkv, B, L, H, DH)
    if exact:
        o32, lse = fwd_exact(qkv, B, L, H, DH)
    o = per_head(o32, B, L, H, DH)
    do = per_head(dO, B, L, H, DH)
    lse = lse.double().reshape(B, H, L)
    rows = torch.arange(L) if rows is None else rows
    bh = [(b, h) for b in range(B) for h in range(H)] if bh is None else bh
    a = torch.arange(L)
    fe = [fwd_head(qs[b, h], k[b, h], v[b, h], a, DH)[3:] if fwd_err else None for b, h in bh]
    outs = [bwd_head(qs[b, h], k[b, h], v[b, h], do[b, h], o[b, h], lse[b, h], rows, DH, f) for (b, h), f in zip(bh, fe)]
    return tuple(torch.stack([x[i] for x in outs]) for i in range(6))


def colsum(qkv, dO, o32, lse, pair_img, L, H, DH, exact=False):
    """GradCAM column sums c (P, 3E) = sums over patch tokens l >= 1 of (dq, dk, dv) for pair p on image pair_img[p], and
    their bound.  dO (P*L, E) with a zero CLS row.  Evaluated as the kernel does (rows of P sum to one, rows of dS to
    zero):  cq = sum_l u_l k_l / sqrt(DH), u_l = sum_q dS[q,l];  ck = -sum_q dS[q,0] q_s,q / log2(e);
    cv = sum_q (1 - P[q,0]) dO_q; with the exact forward this IS the column sum."""
    B = int(max(pair_img)) + 1
    qs, k, v = heads(qkv, B, L, H, DH)
    if exact:
        o32, lse = fwd_exact(qkv, B, L, H, DH)
    o = per_head(o32, B, L, H, DH)
    lse = lse.double().reshape(B, H, L)
    Pn = len(pair_img)
    do = per_head(dO, Pn, L, H, DH)
    E = H * DH
    c = torch.zeros(Pn, 3, H, DH, dtype=F64)
    bc = torch.zeros_like(c)
    a = torch.arange(L)
    n = acc_n_bwd(L)
    sq = 1.0 / math.sqrt(DH)
    for p, b in enumerate(pair_img):
        for h in range(H):
            P, dS, eps, edS = _blocks(qs[b, h], k[b, h], v[b, h], do[p, h], o[b, h], lse[b, h], a, a, DH, False)
            u = dS.sum(0)
            eu = edS.sum(0) + n * U * dS.abs().sum(0)
            cq = sq * (u @ k[b, h])
            c[p, 0, h] = cq
            bc[p, 0, h] = sq * (eu @ k[b, h].abs() + n * U * (u.abs() @ k[b, h].abs())) + 3 * U * cq.abs()
            ck = -LN2 * (dS[:, 0] @ qs[b, h])
            c[p, 1, h] = ck
            bc[p, 1, h] = LN2 * (edS[:, 0] @ qs[b, h].abs() + n * U * (dS[:, 0].abs() @ qs[b, h].abs())) + 3 * U * ck.abs()
            w = 1.0 - P[:, 0]
            cv = w @ do[p, h]
            c[p, 2, h] = cv
            bc[p, 2, h] = (P[:, 0] * LN2 * eps[:, 0] + U) @ do[p, h].abs() + n * U * (w.abs() @ do[p, h].abs())
    return c.reshape(Pn, 3 * E), bc.reshape(Pn, 3 * E)


def colsum_direct(qkv, dO, o32, lse, pair_img, L, H, DH, exact=False):
    """The literal column sums over tokens l >= 1 of the full fp64 backward (dq, dk, dv) of every pair: (P, 3E)."""
    qkv_p = qkv.reshape(-1, L, qkv.shape[1])[list(pair_img)].reshape(-1, qkv.shape[1])
    Pn = len(pair_img)
    if not exact:
        o32 = o32.reshape(-1, L, o32.shape[1])[list(pair_img)].reshape(-1, o32.shape[1])
        lse = lse.reshape(-1, H, L)[list(pair_img)]
    dq, dk, dv = bwd(qkv_p, dO, o32, lse, Pn, L, H, DH, exact=exact)[:3]
    return torch.stack([x.reshape(Pn, H, L, DH)[:, :, 1:].sum(2) for x in (dq, dk, dv)], 1).reshape(Pn, 3 * H * DH)
