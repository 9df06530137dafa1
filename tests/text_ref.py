"""fp64 restatement of the CLIP text tower (reference clip/model.py:392-405) and of causal attention, for the tests of
csrc/text.hip and CLIP.encode_text.

encode_text(ids, sd): token_embedding[ids] + positional_embedding, `layers` causal residual blocks, ln_final, the EOT row
(first argmax of the ids), @ text_projection.  Everything in float64 except the reference's own fp16 rounding point: the
attention output, the out-projection weight / bias and its result are fp16 (clip/myAtt.py:321 `F.linear(o.half(), ...)`),
as in oracle/weclip_oracle.attention.

Causal attention (kernel conventions of tests/attn_ref.py: packed fp16 qkv, q pre-scaled by log2(e)/sqrt(DH), base-2
scores).  Query i sees keys j <= i; the masked probabilities are exactly 0.  Error model per element, with U = 2^-24,
U16 = 2^-11 (derivation as in attn_ref.py; only the key count changes):
  exponent  eps = (DH + 8) U (sum_d |q_d k_d| + |m|) + 2^-22: a DH-term fp32 dot product of exact fp16 x fp16 products,
            the subtraction of the row maximum m, and v_exp_f32's 1-ulp error.  p moves by p ln2 eps.
  fp16 P    P is the fp16 B operand of the O^T = V^T P^T MFMA: 2^-11 relative per term plus 2^-25 absolute (subnormal
            spacing / 2); p <= 1 and l = sum p >= 1 (the maximum contributes 1), so the absolute part is <= 2^-25 |v| / l.
  sums      n = L + 8 fp32 accumulations (MFMA chain of at most L keys, the cross-lane add, the final products), numerator
            and denominator: 2 n U of sum |terms|.
  => |O - O64| <= sum_j P_j |v_j| (U16 + 2 n U + ln2 eps_j) + ln2 |O| sum_j P_j eps_j + 2^-25 sum_j |v_j| / l.
  lse       = m + log2 l: sum_j P_j eps_j + n U log2(e) + 2 U (|lse| + |m|) + 2^-22.
  map       the kernel adds p_j / l per head (exp2, the sum and one product): P_j (ln2 eps_j + (n + 3) U) per head, then the
            H-head sum and 1/H: + (H + 3) U M.  Above the diagonal the map is exactly 0.
The fp16 output o16 adds one fp16 ulp of the reference (attn_ref.ulp16).
"""
import math

import torch

from attn_ref import LN2, LOG2E, SUB16, U, U16, heads, qscale, ulp16  # noqa: F401

F64 = torch.float64


def causal_fwd(qkv, B, L, H, DH):
    """-> O (B*L, E), lse (B, H, L), mean (B, L, L) and their bounds bO, blse, bM (same shapes), float64."""
    qs, k, v = heads(qkv, B, L, H, DH)
    s = qs @ k.transpose(-1, -2)                                    # (B, H, L, L)
    mask = torch.ones(L, L, dtype=torch.bool).triu(1)
    s = s.masked_fill(mask, float("-inf"))
    m = s.max(-1).values
    p = torch.exp2(s - m[..., None])
    l = p.sum(-1)
    P = p / l[..., None]
    O = P @ v
    lse = m + torch.log2(l)
    n = L + 8
    prod = (qs.abs() @ k.abs().transpose(-1, -2)).masked_fill(mask, 0.0)
    eps = (DH + 8) * U * (prod + m.abs()[..., None]) + 2.0 ** -22
    va = v.abs()
    vsum = (~mask).to(F64) @ va                                     # sum of |v_j| over the keys each query sees
    Pe = P * eps
    bO = ((U16 + 2 * n * U) * P) @ va + LN2 * (Pe @ va + Pe.sum(-1, keepdim=True) * O.abs()) + (SUB16 / l)[..., None] * vsum
    blse = Pe.sum(-1) + n * U * LOG2E + 2 * U * (lse.abs() + m.abs()) + 2.0 ** -22
    M = P.sum(1) / H
    bM = (P * (LN2 * eps + (n + 3) * U)).sum(1) / H + (H + 3) * U * M
    E = H * DH
    O = O.permute(0, 2, 1, 3).reshape(B * L, E)
    bO = bO.permute(0, 2, 1, 3).reshape(B * L, E)
    return O, lse, M, bO, blse, bM


def make_causal_inputs(B, L, H, DH, seed=0):
    """qkv (B*L, 3E) fp16, q pre-scaled.  Every query i < L - 1 gets a large score (gap log2(L) + 6) on key i + 1, the key
    just above the diagonal, and on key L - 1: a kernel that lets a query see either moves O by O(|v|).  Query L - 1 is
    aimed at key 0 so that the last row also has a dominant key to get right."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, L, DH, generator=g, dtype=F64) * qscale(DH)
    k = torch.randn(B, H, L, DH, generator=g, dtype=F64)
    v = torch.randn(B, H, L, DH, generator=g, dtype=F64)
    gap = math.log2(L) + 6.0 if L > 1 else 0.0
    for i in range(L):
        targets = {min(i + 1, L - 1), L - 1} if i < L - 1 else {0}
        for j in targets:
            kj = k[:, :, j]
            q[:, :, i] += gap * kj / (kj * kj).sum(-1, keepdim=True)
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H * DH).half()


# ---------------------------------------------------------------------------------------------------------------------
# the whole tower

def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _d(t):
    return torch.as_tensor(t).double()


def text_layers(sd):
    return len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})


def block(x, sd, p, heads_):
    """x (N, L, W) float64 -> causal residual block (clip/model.py:210-214 with the text mask)."""
    N, L, W = x.shape
    DH = W // heads_
    a = _ln(x, _d(sd[p + "ln_1.weight"]), _d(sd[p + "ln_1.bias"]))
    qkv = a @ _d(sd[p + "attn.in_proj_weight"]).T + _d(sd[p + "attn.in_proj_bias"])
    q, k, v = qkv.split(W, -1)
    sh = lambda t: t.reshape(N, L, heads_, DH).transpose(1, 2)
    s = (sh(q) / math.sqrt(DH)) @ sh(k).transpose(-1, -2)
    s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    o = (torch.softmax(s, -1) @ sh(v)).transpose(1, 2).reshape(N, L, W)
    h = lambda t: t.half().double()
    o = h(h(o) @ h(_d(sd[p + "attn.out_proj.weight"])).T + h(_d(sd[p + "attn.out_proj.bias"])))     # forced fp16
    x1 = x + o
    z = _ln(x1, _d(sd[p + "ln_2.weight"]), _d(sd[p + "ln_2.bias"])) @ _d(sd[p + "mlp.c_fc.weight"]).T + _d(sd[p + "mlp.c_fc.bias"])
    z = z * torch.sigmoid(1.702 * z)
    return x1 + z @ _d(sd[p + "mlp.c_proj.weight"]).T + _d(sd[p + "mlp.c_proj.bias"])


def encode_text(ids, sd, L_used=None):
    """ids (N, Lctx) -> (N, Ed) float64.  L_used: positions run (default all; max(eot) + 1 gives the same result)."""
    ids = torch.as_tensor(ids).long()
    N, Lctx = ids.shape
    Lu = Lctx if L_used is None else L_used
    W = sd["ln_final.weight"].shape[0]
    H = max(W // 64, 1)
    x = _d(sd["token_embedding.weight"])[ids[:, :Lu]] + _d(sd["positional_embedding"])[:Lu]
    for i in range(text_layers(sd)):
        x = block(x, sd, f"transformer.resblocks.{i}.", H)
    x = _ln(x, _d(sd["ln_final.weight"]), _d(sd["ln_final.bias"]))
    eot = ids.argmax(-1)
    return x[torch.arange(N), eot] @ _d(sd["text_projection"])


def zeroshot(feat, C, T):
    """zeroshot_classifier after encode_text: (C*T, Ed) -> (C, Ed)."""
    f = _d(feat)
    f = f / f.norm(dim=-1, keepdim=True)
    m = f.view(C, T, -1).mean(1)
    return m / m.norm(dim=-1, keepdim=True)


def fwd_exact_nomask(qkv, B, L, H, DH):
    """Bidirectional attention output (B*L, E) of the same inputs (what a kernel without the mask would return)."""
    qs, k, v = heads(qkv, B, L, H, DH)
    P = torch.softmax((qs @ k.transpose(-1, -2)) * LN2, -1)
    return (P @ v).permute(0, 2, 1, 3).reshape(B * L, H * DH)
