"""The fp64 attention reference of the kernel tests (tests/attn_ref.py) without a GPU: it is the definition (fp64 autograd of
softmax(q k^T / sqrt(d)) v), its bounds admit an fp32 / fp16-operand evaluation of the same formulas and reject the faults a
tiled kernel makes (at the shapes of tests/test_attention_kernels_gpu.py), and every C-ABI limit of the attention entry
points, alignment included, is refused before any launch."""
import ctypes
import math
import os

import pytest
import torch

from tests import attn_ref as R

F64 = torch.float64
WC_ERR_ARG = 1


def _autograd(qkv, dO, B, L, H, DH):
    """O, lse and the gradients w.r.t. the unscaled (q, k, v) of softmax(q k^T / sqrt(DH)) v by fp64 autograd."""
    qs, k, v = R.heads(qkv, B, L, H, DH)
    q = (qs / R.qscale(DH)).requires_grad_(True)
    k = k.clone().requires_grad_(True)
    v = v.clone().requires_grad_(True)
    s = q @ k.transpose(-1, -2) / math.sqrt(DH)
    O = torch.softmax(s, -1) @ v
    O.backward(R.per_head(dO, B, L, H, DH))
    lse = torch.logsumexp(s, -1) / math.log(2.0)
    return O.detach(), lse.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("B,L,H,DH", [(2, 37, 2, 32), (1, 130, 3, 64)])
def test_reference_is_fp64_autograd(B, L, H, DH):
    qkv, dO = R.make_inputs(B, L, H, DH, seed=1)
    O, lse, gq, gk, gv = _autograd(qkv, dO, B, L, H, DH)
    rows = R.check_rows(L)
    o, l, _, _ = R.fwd(qkv, B, L, H, DH, rows=rows)
    assert torch.allclose(o, O[:, :, rows].reshape(B * H, len(rows), DH), rtol=0, atol=1e-12)
    assert torch.allclose(l, lse[:, :, rows].reshape(B * H, -1), rtol=0, atol=1e-12)
    dq, dk, dv = R.bwd(qkv, dO, None, None, B, L, H, DH, rows=rows, exact=True)[:3]
    for got, want in ((dq, gq), (dk, gk), (dv, gv)):
        want = want[:, :, rows].reshape(B * H, len(rows), DH)
        assert torch.allclose(got, want, rtol=0, atol=1e-11 * want.abs().max().item())
    M, _ = R.mean(qkv, B, L, H, DH, list(range(B)), rows)
    qs, k, _ = R.heads(qkv, B, L, H, DH)
    Pm = torch.softmax(qs @ k.transpose(-1, -2) * math.log(2.0), -1).mean(1)
    assert torch.allclose(M, Pm[:, rows], rtol=0, atol=1e-14)


@pytest.mark.parametrize("L,H,DH", [(50, 2, 64), (137, 3, 32)])
def test_colsum_is_the_patch_token_column_sum(L, H, DH):
    pair_img = [2, 0, 2, 1]
    qkv, _ = R.make_inputs(3, L, H, DH, seed=2)
    _, dO = R.make_inputs(len(pair_img), L, H, DH, seed=3, plant=False, cls_zero=True)
    c, _ = R.colsum(qkv, dO, None, None, pair_img, L, H, DH, exact=True)
    direct = R.colsum_direct(qkv, dO, None, None, pair_img, L, H, DH, exact=True)
    assert torch.allclose(c, direct, rtol=0, atol=1e-11 * direct.abs().max().item())
    qkv_p = qkv.reshape(3, L, -1)[pair_img].reshape(-1, qkv.shape[1])
    _, _, gq, gk, gv = _autograd(qkv_p, dO, len(pair_img), L, H, DH)
    auto = torch.stack([g[:, :, 1:].sum(2).reshape(len(pair_img), -1) for g in (gq, gk, gv)], 1).reshape(len(pair_img), -1)
    assert torch.allclose(c, auto, rtol=0, atol=1e-11 * auto.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------
# the bounds: an fp32 evaluation with fp16 P / dS operands passes them; the faults fail them

def _fp32_fwd(qs, k, v, rows, drop=0, dup_last=False):
    """O and lse the way the kernels round: fp32 scores and sums, P rounded to fp16 before P V.  drop: leave out the first
    `drop` keys; dup_last: count key L-1 twice (the clamp-to-L-1 loads without the mask)."""
    s = qs[rows].float() @ k.float().T
    if drop:
        s[:, :drop] = -float("inf")
    vv = v.float()
    if dup_last:
        s = torch.cat([s, s[:, -1:]], 1)
        vv = torch.cat([vv, vv[-1:]], 0)
    m = s.max(1).values
    p = torch.exp2(s - m[:, None])
    l = p.sum(1)
    return ((p.half().float() @ vv) / l[:, None]).double(), (m + torch.log2(l)).double()


def _exceeds(got, ref, bound):
    return int(((got - ref).abs() > bound).sum())


FWD_SHAPES = [  # (B, L, H, DH, kr): forward geometries of the GPU file (kr = keys of the 8-wave VALU loop)
    (1, 65, 2, 64, 1), (1, 72, 2, 64, 8), (1, 257, 2, 64, 1), (1, 1032, 2, 64, 8), (1, 1025, 2, 64, 1),
    (1, 1025, 2, 32, 0), (1, 137, 2, 32, 0), (1, 4609, 2, 64, 1),
]


@pytest.mark.parametrize("B,L,H,DH,kr", FWD_SHAPES)
def test_forward_bounds_admit_fp32_and_reject_faults(B, L, H, DH, kr):
    qkv, _ = R.make_inputs(B, L, H, DH, seed=L)
    qs, k, v = R.heads(qkv, B, L, H, DH)
    rows = R.check_rows(L)
    O, lse, P, bO, blse = R.fwd_head(qs[0, 0], k[0, 0], v[0, 0], rows, DH)
    o32, l32 = _fp32_fwd(qs[0, 0], k[0, 0], v[0, 0], rows)
    assert _exceeds(o32, O, bO) == 0 and _exceeds(l32, lse, blse) == 0
    od, _ = _fp32_fwd(qs[0, 0], k[0, 0], v[0, 0], rows, dup_last=True)
    assert _exceeds(od, O, bO) > 0, "key L-1 counted twice passes the O bound"
    if kr:
        ok, _ = _fp32_fwd(qs[0, 0], k[0, 0], v[0, 0], rows, drop=kr)
        assert _exceeds(ok, O, bO) > 0, "dropping the first kr keys passes the O bound"
    # one query row with its neighbour's output
    O_all = R.fwd_head(qs[0, 0], k[0, 0], v[0, 0], torch.arange(L), DH)[0]
    i = len(rows) // 2
    shifted = O.clone()
    shifted[i] = O_all[(rows[i] + 1) % L]
    assert _exceeds(shifted, O, bO) > 0, "a neighbour row's output passes the O bound"
    # lse of heads 0 and 1 swapped: the lse bound and the mean map built on it
    lse1 = R.fwd_head(qs[0, 1], k[0, 1], v[0, 1], rows, DH)[1]
    assert _exceeds(lse1, lse, blse) > 0, "swapped heads pass the lse bound"
    M, bM = R.mean(qkv, B, L, H, DH, [0], rows)
    Pswap = sum(torch.exp2(qs[0, h, rows] @ k[0, h].T - R.fwd_head(qs[0, 1 - h], k[0, 1 - h], v[0, 1 - h], rows, DH)[1][:, None])
                for h in range(2)) / H
    assert _exceeds(Pswap, M[0], bM[0]) > 0, "swapped heads pass the mean-map bound"


BWD_SHAPES = [(1, 65, 2, 32), (1, 1025, 1, 64), (1, 128, 2, 64), (1, 1024, 1, 32)]


@pytest.mark.parametrize("B,L,H,DH", BWD_SHAPES)
def test_backward_bounds_admit_fp32_and_reject_delta_from_fp16_O(B, L, H, DH):
    qkv, dO = R.make_inputs(B, L, H, DH, seed=L + 7)
    O, lse = R.fwd_exact(qkv, B, L, H, DH)
    o32, lse32 = O.float(), lse.float()
    rows = R.check_rows(L)
    dq, dk, dv, bdq, bdk, bdv = R.bwd(qkv, dO, o32, lse32, B, L, H, DH, rows=rows, bh=[(0, 0)])
    # fp32 evaluation with fp16 P / dS operands
    qs, k, v = [x[0, 0].float() for x in R.heads(qkv, B, L, H, DH)]
    do = R.per_head(dO, B, L, H, DH)[0, 0].float()
    o = R.per_head(o32, B, L, H, DH)[0, 0].float()
    P = torch.exp2(qs @ k.T - lse32[0, 0][:, None])
    dS = P * (do @ v.T - (do * o).sum(1)[:, None])
    dq32 = (dS.half().float() @ k) * (1.0 / math.sqrt(DH))
    dk32 = (dS.half().float().T @ qs) * R.LN2
    dv32 = P.half().float().T @ do
    for got, ref, b in ((dq32[rows], dq[0], bdq[0]), (dk32[rows], dk[0], bdk[0]), (dv32[rows], dv[0], bdv[0])):
        assert _exceeds(got.double(), ref, b) == 0
    # delta from the fp16 O (the fp16 out-projection input instead of o32)
    dqf, dkf = R.bwd(qkv, dO, o32.half(), lse32, B, L, H, DH, rows=rows, bh=[(0, 0)])[:2]
    assert _exceeds(dqf[0], dq[0], bdq[0]) + _exceeds(dkf[0], dk[0], bdk[0]) > 0, "delta from fp16 O passes the bounds"


@pytest.mark.parametrize("L,H,DH,dscale", [(137, 2, 64, 1.0), (197, 2, 32, 4096.0), (1025, 1, 64, 1.0)])
def test_colsum_bound_admits_fp32_and_rejects_the_cls_row(L, H, DH, dscale):
    pair_img = [1, 0, 1]
    qkv, _ = R.make_inputs(2, L, H, DH, seed=L)
    _, dO = R.make_inputs(len(pair_img), L, H, DH, seed=L + 1, plant=False, dscale=dscale, cls_zero=True)
    O, lse = R.fwd_exact(qkv, 2, L, H, DH)
    o32, lse32 = O.float(), lse.float()
    c, bc = R.colsum(qkv, dO, o32, lse32, pair_img, L, H, DH)
    # fp32 evaluation of the kernel's formulas
    E = H * DH
    qs, k, v = [x.float() for x in R.heads(qkv, 2, L, H, DH)]
    o, do = R.per_head(o32, 2, L, H, DH).float(), R.per_head(dO, len(pair_img), L, H, DH).float()
    c32 = torch.zeros(len(pair_img), 3, H, DH)
    for p, b in enumerate(pair_img):
        for h in range(H):
            P = torch.exp2(qs[b, h] @ k[b, h].T - lse32[b, h][:, None])
            dS = P * (do[p, h] @ v[b, h].T - (do[p, h] * o[b, h]).sum(1)[:, None])
            c32[p, 0, h] = dS.sum(0) @ k[b, h] / math.sqrt(DH)
            c32[p, 1, h] = -(dS[:, 0] @ qs[b, h]) * R.LN2
            c32[p, 2, h] = (1 - P[:, 0]) @ do[p, h]
    assert _exceeds(c32.reshape(len(pair_img), 3 * E).double(), c, bc) == 0
    # the CLS row (token 0) included in the column sums
    qkv_p = qkv.reshape(2, L, -1)[pair_img].reshape(-1, qkv.shape[1])
    o_p = o32.reshape(2, L, -1)[pair_img].reshape(-1, E)
    dq, dk, dv = R.bwd(qkv_p, dO, o_p, lse32[pair_img], len(pair_img), L, H, DH)[:3]
    full = torch.stack([x.reshape(len(pair_img), H, L, DH).sum(2) for x in (dq, dk, dv)], 1).reshape(len(pair_img), -1)
    assert _exceeds(full, c, bc) > 0, "column sums with the CLS row pass the bound"


# ---------------------------------------------------------------------------------------------------------------------
# C ABI: refused before any launch

@pytest.fixture(scope="module")
def so():
    from weclip_vit_comer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, _, args in _lib.parse_header():
        if name.startswith("wc_attn"):
            getattr(so, name).argtypes = [t for t, _ in args]
    return so


P = ctypes.c_void_p(256)            # never dereferenced: every call below is refused before any launch
M8 = ctypes.c_void_p(256 + 8)       # 8-byte aligned, not 16
M2 = ctypes.c_void_p(256 + 2)       # 2-byte aligned


def _fwd(so, **kw):
    a = dict(qkv=P, out=P, out32=P, lse=P, B=2, L=197, H=12, DH=64)
    assert set(kw) <= set(a), kw          # an unknown key would leave a valid call that launches
    a.update(kw)
    return so.wc_attn_fwd(a["qkv"], a["out"], a["out32"], a["lse"], a["B"], a["L"], a["H"], a["DH"], None)


def _mean(so, **kw):
    a = dict(qkv=P, lse=P, mean=P, B=2, L=197, H=12, DH=64)
    assert set(kw) <= set(a), kw          # an unknown key would leave a valid call that launches
    a.update(kw)
    return so.wc_attn_mean(a["qkv"], a["lse"], a["mean"], a["B"], a["L"], a["H"], a["DH"], None)


def _bwd(so, **kw):
    a = dict(qkv=P, dO=P, o32=P, lse=P, qt=P, kt=P, dot=P, delta=P, hi=P, lo=P, B=2, L=197, Lp=256, H=8, DH=32)
    assert set(kw) <= set(a), kw          # an unknown key would leave a valid call that launches
    a.update(kw)
    return so.wc_attn_bwd(a["qkv"], a["dO"], a["o32"], a["lse"], a["qt"], a["kt"], a["dot"], a["delta"], a["hi"], a["lo"],
                          a["B"], a["L"], a["Lp"], a["H"], a["DH"], None)


def _colsum(so, **kw):
    a = dict(qkv=P, dO=P, o32=P, lse=P, pair_img=P, delta=P, u=P, dS0=P, P0=P, c=P, P=5, L=197, H=12, DH=64)
    assert set(kw) <= set(a), kw          # an unknown key would leave a valid call that launches
    a.update(kw)
    return so.wc_attn_bwd_colsum(a["qkv"], a["dO"], a["o32"], a["lse"], a["pair_img"], a["delta"], a["u"], a["dS0"], a["P0"],
                                 a["c"], a["P"], a["L"], a["H"], a["DH"], None)


_COMMON = [dict(DH=16), dict(DH=48), dict(DH=128), dict(DH=0), dict(B=0), dict(B=-1), dict(L=0), dict(L=-5), dict(H=0),
           dict(H=-1)]


@pytest.mark.parametrize("kw", _COMMON + [dict(qkv=None), dict(out=None), dict(lse=None), dict(qkv=M8), dict(qkv=M2),
                                          dict(out=M8), dict(out32=M8), dict(H=65536), dict(B=65536)])
def test_attn_fwd_refusals(so, kw):
    assert _fwd(so, **kw) == WC_ERR_ARG


@pytest.mark.parametrize("kw", _COMMON + [dict(qkv=None), dict(lse=None), dict(mean=None), dict(qkv=M8), dict(qkv=M2)])
def test_attn_mean_refusals(so, kw):
    assert _mean(so, **kw) == WC_ERR_ARG


@pytest.mark.parametrize("kw", _COMMON + [
    dict(Lp=200), dict(Lp=192), dict(Lp=0), dict(L=257, Lp=256), dict(H=1, DH=32), dict(H=3, DH=32),
    dict(qkv=None), dict(dO=None), dict(o32=None), dict(lse=None), dict(qt=None), dict(kt=None), dict(dot=None),
    dict(delta=None), dict(hi=None), dict(qkv=M8), dict(dO=M8), dict(o32=M8), dict(qt=M8), dict(kt=M8), dict(dot=M8),
    dict(hi=M2), dict(lo=M2)])
def test_attn_bwd_refusals(so, kw):
    assert _bwd(so, **kw) == WC_ERR_ARG


@pytest.mark.parametrize("kw", [k for k in _COMMON if "B" not in k] + [
    dict(P=0), dict(P=-2), dict(P=65536), dict(H=65536), dict(qkv=None), dict(dO=None), dict(o32=None), dict(lse=None),
    dict(pair_img=None), dict(delta=None), dict(u=None), dict(dS0=None), dict(P0=None), dict(c=None), dict(qkv=M8),
    dict(dO=M8), dict(o32=M8), dict(qkv=M2)])
def test_attn_bwd_colsum_refusals(so, kw):
    assert _colsum(so, **kw) == WC_ERR_ARG


def test_refusal_message_names_the_alignment(so):
    from weclip_vit_comer_amd import _lib
    for call in (lambda: _lib.lib().wc_attn_fwd(M8, P, None, P, 2, 197, 12, 64, None),
                 lambda: _lib.lib().wc_attn_mean(M8, P, P, 2, 197, 12, 64, None),
                 lambda: _lib.lib().wc_attn_bwd_colsum(P, M8, P, P, P, P, P, P, P, P, 5, 197, 12, 64, None)):
        with pytest.raises(RuntimeError, match="aligned"):
            call()
