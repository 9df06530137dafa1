"""The fp64 affinity-refinement reference of the kernel tests (tests/affinity_ref.py) without a GPU: it agrees with the fp32 oracle
and the reference golden at their own precision, its bounds admit two fp32 evaluations of the same formulas (K_MEASURED is printed)
and reject the faults a blocked kernel makes, at every shape of tests/test_affinity_kernels_gpu.py; the layer-selection inputs are
far from ambiguity; every C-ABI limit of the affinity entry points is refused before any launch; and the host's size rules are the
library's."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import affinity_ref as R

F64, F32, I32 = torch.float64, torch.float32, torch.int32
WC_ERR_ARG = 1
ALL_HW = R.FUSED_HW + R.MATVEC_HW


def _exceeds(got, ref, b):
    """Elements outside the bound (NaN and inf count)."""
    return int((~((got.to(F64) - ref).abs() <= b)).sum())


def _nb(hw):
    return 1 if hw >= R.BIG else 2


# ---------------------------------------------------------------------------------------------------------------------
# the reference against the oracle and the golden

@pytest.mark.parametrize("seg_trans,n_last", [(False, 6), (True, 6), (True, 10)])
def test_reference_matches_the_oracle_chain(seg_trans, n_last):
    from oracle import weclip_oracle as O
    h, w, B = 5, 7, 2
    hw = h * w
    maps = R.maps_input(B, hw, 12, seed=3)
    seg = R.seg_input(B, hw, seed=3)
    sel = maps[-n_last:] if seg_trans else maps[-8:]
    wgt = R.seg_weights(sel)["wgt"] if seg_trans else R.uniform_wgt(B, 8)
    W, _ = R.aff_weight(sel, wgt, seg if seg_trans else None)
    cams = R.cams_input(3, h, w, seed=1)
    for b in range(B):
        Wo = O.affinity_weight(torch.stack([m[b] for m in maps]), seg[b], seg_trans, n_last)
        np.testing.assert_allclose(Wo.numpy(), W[b].numpy(), rtol=1e-5, atol=0)
        To = O.compute_trans_mat(Wo)
        T, _ = R.trans_mat(Wo[None])
        np.testing.assert_allclose(To.numpy(), T[0].numpy(), rtol=2e-5, atol=1e-10)
        for p in range(3):
            cam = cams[p].reshape(h, w).numpy()
            mask = O.box_mask(cam, 0.4)
            V = (torch.from_numpy(mask) * cams[p].reshape(h, w)).reshape(1, hw, 1)
            ref, _ = R.refine(Wo[None], V)
            np.testing.assert_allclose(O.refine_cam(To, cam, mask).reshape(-1).numpy(), ref[0, :, 0].numpy(), rtol=5e-5, atol=1e-9)


def test_reference_matches_the_trans_mat_golden(golden):
    g = golden("tiny_func.npz")
    T, b = R.trans_mat(torch.from_numpy(g["trans_in"])[None])
    np.testing.assert_allclose(g["trans_out"], T[0].numpy(), rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("h,w,H,Wd", R.UPSAMPLE_SHAPES)
def test_reference_matches_the_oracle_upsampling(h, w, H, Wd):
    from oracle import weclip_oracle as O
    B, Kc = 2, 3
    Rm = R.refined_input(B, h * w, Kc, seed=2)
    nk = torch.tensor([3, 2], dtype=I32)
    u = R.upsample(Rm, nk, h, w, H, Wd)
    for b in range(B):
        n = int(nk[b])
        ups = torch.stack([O.upsample_cam(Rm[b, :, k].reshape(h, w), H, Wd) for k in range(n)])
        np.testing.assert_allclose(ups.numpy(), u["cams"][b, 1:1 + n].numpy(), rtol=0, atol=2e-6)
        np.testing.assert_allclose((1 - ups.max(0)[0]).numpy(), u["cams"][b, 0].numpy(), rtol=0, atol=2e-6)
        assert bool(u["zero"][b, 1 + n:].all()) and not bool(u["zero"][b, :1 + n].any())
        assert (u["cams"][b, 1 + n:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the bounds admit two fp32 evaluations of the same formulas

def _ratio(acc, name, got, ref, A):
    """Records the worst |got - ref| / (EPS A) of stage `name`; where A == 0 the output is exact."""
    err = (got.to(F64) - ref).abs()
    assert bool(torch.isfinite(err).all()), name
    exact = A == 0
    assert bool((err[exact] == 0).all()), f"{name}: an exact element differs"
    r = (err[~exact] / (R.EPS * A[~exact])).max().item() if bool((~exact).any()) else 0.0
    acc[name] = max(acc.get(name, 0.0), r)


def _measure():
    acc = {}
    for mode in ("matmul", "loop"):
        for hw in ALL_HW:
            B, big = _nb(hw), hw >= R.BIG
            # affinity weight
            for nmaps in ((2,) if big else R.NMAPS):
                maps, wgt = R.maps_input(B, hw, nmaps), R.wgt_input(B, nmaps)
                for seg in (None, R.seg_input(B, hw)):
                    W, A = R.aff_weight(maps, wgt, seg)
                    _ratio(acc, "weight", R.aff_weight32(maps, wgt, seg, mode), W, A)
            # reciprocals: c1, r = 1 / (W c), c_next = 1 / (W^T r)
            W, v = R.matrix_input(B, hw), R.vec_input(B, hw)
            ones = torch.ones(B, hw, 1)
            c, A, _ = R.col_scale(W)
            _ratio(acc, "recip", R.matvec32(W, ones, recip=True, transpose=True, mode=mode)[:, :, 0], c, A)
            for tr in (False, True):
                o, A, _ = R.matvec(W, v[:, :, None], recip=True, transpose=tr)
                _ratio(acc, "recip", R.matvec32(W, v[:, :, None], recip=True, transpose=tr, mode=mode), o, A)
            # the linear form and T_sym X
            sin, sout = R.vec_input(B, hw, seed=1), R.vec_input(B, hw, seed=2)
            for Kc in ((1, 5) if big else R.MATVEC_K):
                X, add = R.x_input(B, hw, Kc), R.x_input(B, hw, Kc, seed=9)
                for tr in (False, True):
                    for q in ((7, 0) if big else range(8)):
                        kw = dict(sin=sin if q & 1 else None, sout=sout if q & 2 else None, add=add if q & 4 else None,
                                  alpha=(1.0, 0.5, 0.3)[q % 3], transpose=tr)
                        o, A, _ = R.matvec(W, X, **kw)
                        _ratio(acc, "matvec", R.matvec32(W, X, mode=mode, **kw), o, A)
                t = R.tsym_apply(W, sin, sout, X)
                o32, y32 = R.tsym_apply32(W, sin, sout, X, mode)
                _ratio(acc, "matvec", o32, t["out"], t["A"])
                _ratio(acc, "matvec", y32, t["y1"], t["A_y1"])
        for hw in R.SEG_HW:
            for nmaps in R.SEG_NMAPS:
                maps = R.maps_input(2, hw, nmaps)
                s = R.seg_weights(maps)
                rs32, A32 = R.seg_weights32(maps, mode)
                _ratio(acc, "rowsum", rs32, s["rowsum"], s["A_rowsum"])
                _ratio(acc, "rowsum", A32, s["A_l"], s["A_A"])
    for hw in R.TSYM_HW:
        W, r, c = R.matrix_input(2, hw), R.vec_input(2, hw, seed=1), R.vec_input(2, hw, seed=2)
        T, A, _ = R.tsym_mat(W, r, c)
        _ratio(acc, "tsym", R.tsym_mat32(W, r, c), T, A)
    for h, w, H, Wd in R.UPSAMPLE_SHAPES:
        for Kc in R.UPSAMPLE_K:
            for C in {Kc + 1, max(Kc, 2)}:
                Rm, nk = R.refined_input(3, h * w, Kc), R.nk_input(3, Kc, C)
                u = R.upsample(Rm, nk, h, w, H, Wd, C)
                st32, c32 = R.upsample32(Rm, nk, h, w, H, Wd, C)
                _ratio(acc, "stats", st32, u["stats"], u["A_stats"])
                _ratio(acc, "upsample", c32, u["cams"], u["A"])
    return acc


def test_bounds_admit_the_fp32_emulation():
    acc = _measure()
    print()
    print("K_MEASURED = {" + ", ".join(f'"{k}": {acc[k]:.2f}' for k in R.K) + "}")
    print("K = {" + ", ".join(f'"{k}": {float(math.ceil(4 * acc[k] - 1e-9)):.1f}' for k in R.K) + "}")
    for k in R.K:
        assert acc[k] <= R.K[k], f"{k}: an fp32 emulation is outside the bound ({acc[k]:.3g} > K = {R.K[k]})"
        # the record in tests/affinity_ref.py is this measurement (the serial loop is the same on every host, torch.matmul and
        # torch.sum may order their sums by the host's vector width and thread count: a quarter of room), and K is four times it,
        # rounded up
        assert 0.5 * R.K_MEASURED[k] <= acc[k] <= 1.25 * R.K_MEASURED[k] + 0.01, (k, acc[k], R.K_MEASURED[k])
        assert R.K[k] == math.ceil(4 * R.K_MEASURED[k] - 1e-9), k


# ---------------------------------------------------------------------------------------------------------------------
# planted faults: each one, put into the fp64 reference of its stage, is outside that stage's bound at every shape

@pytest.mark.parametrize("hw", ALL_HW)
def test_sum_faults_exceed_the_reciprocal_bounds(hw):
    """An element dropped from or counted twice in a column sum and a row sum; the last row block skipped (8 rows for c1, 32 rows
    for the sweeps' column pass); chunk 1 (j >= 1024) skipped in a row pass."""
    B = 1
    W, cv = R.matrix_input(B, hw), R.vec_input(B, hw)
    W64, c64 = W.to(F64), cv.to(F64)
    i, j = hw // 2, hw // 3
    col = W64.sum(1)                                    # column sums (B, hw)
    c1, A, _ = R.col_scale(W)
    b = R.bound("recip", A)
    for sign in (-1.0, 1.0):
        s = col.clone()
        s[0, j] += sign * W64[0, i, j]
        assert _exceeds(1.0 / s, c1, b) == 1, f"column sum, element {'dropped' if sign < 0 else 'doubled'}"
    for rpb in (8, 32):
        last = (hw - 1) // rpb * rpb
        assert _exceeds(1.0 / (col - W64[:, last:].sum(1)), c1, b) == hw, f"last {rpb}-row block skipped"
    row = (W64 * c64[:, None, :]).sum(2)
    r, A, _ = R.row_scale(W, cv)
    b = R.bound("recip", A)
    for sign in (-1.0, 1.0):
        s = row.clone()
        s[0, i] += sign * W64[0, i, j] * c64[0, j]
        assert _exceeds(1.0 / s, r, b) == 1, f"row sum, element {'dropped' if sign < 0 else 'doubled'}"
    if hw > 1024:
        s = (W64[:, :, :1024] * c64[:, None, :1024]).sum(2)
        assert _exceeds(1.0 / s, r, b) == hw, "chunk 1 skipped"
    # the same for the weighted column pass c_next = 1 / (W^T r)
    cn, A, _ = R.col_scale_next(W, cv)
    b = R.bound("recip", A)
    last = (hw - 1) // 32 * 32
    s = (W64 * c64[:, :, None]).sum(1)
    assert _exceeds(1.0 / (s - (W64[:, last:] * c64[:, last:, None]).sum(1)), cn, b) == hw, "last 32-row block skipped"
    s[0, j] -= W64[0, i, j] * c64[0, i]
    assert _exceeds(1.0 / s, cn, b) == 1, "weighted column sum, element dropped"


@pytest.mark.parametrize("hw", ALL_HW)
def test_tsym_faults_exceed_the_matvec_bound(hw):
    """r and c swapped; W for W^T; class k with class k + 1's X; the factor 0.5 missing; an element dropped from one class."""
    B, Kc = 1, 3
    W, r, c, X = R.matrix_input(B, hw), R.vec_input(B, hw, seed=1), R.vec_input(B, hw, seed=2), R.x_input(B, hw, 3)
    t = R.tsym_apply(W, r, c, X)
    b, by1 = R.bound("matvec", t["A"]), R.bound("matvec", t["A_y1"])
    assert _exceeds(2.0 * t["out"], t["out"], b) > 0, "0.5 missing"
    sw = R.tsym_apply(W, r, c, X.roll(-1, 2))
    assert _exceeds(sw["out"], t["out"], b) > 0 and _exceeds(sw["y1"], t["y1"], by1) > 0, "class k reads class k + 1"
    if hw > 1:            # one token: T_sym = r W c is its own transpose and symmetric in r and c
        sw = R.tsym_apply(W, c, r, X)
        assert _exceeds(sw["y1"], t["y1"], by1) > 0, "r and c swapped (y1)"
        Tm, A, _ = R.tsym_mat(W, r, c)
        assert _exceeds(R.tsym_mat(W, c, r)[0], Tm, R.bound("tsym", A)) > 0, "r and c swapped (T_sym)"
        assert _exceeds(R.tsym_mat(W.transpose(1, 2), r, c)[0], Tm, R.bound("tsym", A)) > 0, "W for W^T (T_sym)"
        for tr in (False, True):
            o, A, _ = R.matvec(W, X, sin=c, sout=r, transpose=tr)
            assert _exceeds(R.matvec(W, X, sin=c, sout=r, transpose=not tr)[0], o, R.bound("matvec", A)) > 0, "W for W^T"
    # an element dropped from y1 of class 1 only, and the last 32-row block missing from the transposed half
    W64, r64, c64, X64 = W.to(F64), r.to(F64), c.to(F64), X.to(F64)
    i, j = hw // 2, hw // 3
    y1 = t["y1"].clone()
    y1[0, i, 1] -= r64[0, i] * W64[0, i, j] * c64[0, j] * X64[0, j, 1]
    assert _exceeds(y1, t["y1"], by1) == 1, "element dropped from y1"
    last = (hw - 1) // 32 * 32
    y2 = torch.einsum("bij,bi,bik->bjk", W64[:, :last], r64[:, :last], X64[:, :last]) * c64[:, :, None]
    assert _exceeds(0.5 * (t["y1"] + y2), t["out"], b) > 0, "last 32-row block skipped"
    if hw > 1024:
        y1 = torch.einsum("bij,bj,bjk->bik", W64[:, :, :1024], c64[:, :1024], X64[:, :1024]) * r64[:, :, None]
        assert _exceeds(y1, t["y1"], by1) > 0, "chunk 1 skipped"


@pytest.mark.parametrize("hw", ALL_HW)
@pytest.mark.parametrize("seg", [False, True])
def test_weight_faults_exceed_the_weight_bound(hw, seg):
    """A layer dropped or counted twice, the CLS row or column read (an off-by-one of the [1:, 1:] window), seg forgotten."""
    B = _nb(hw)
    nmaps = 2 if hw >= R.BIG else 5
    maps, wgt = R.maps_input(B, hw, nmaps), R.wgt_input(B, nmaps)
    sg = R.seg_input(B, hw) if seg else None
    W, A = R.aff_weight(maps, wgt, sg)
    b = R.bound("weight", A)
    assert _exceeds(R.aff_weight(maps[:-1], wgt[:, :-1], sg)[0] if nmaps > 1 else 0 * W, W, b) == W.numel(), "last layer dropped"
    assert _exceeds(R.aff_weight(maps + maps[-1:], torch.cat([wgt, wgt[:, -1:]], 1), sg)[0], W, b) == W.numel(), "layer twice"
    shifted = [torch.cat([m[:, :, :1], m[:, :, :-1]], 2) for m in maps]            # reads column j instead of j + 1
    assert _exceeds(R.aff_weight(shifted, wgt, sg)[0], W, b) > W.numel() // 2, "CLS column read"
    if seg:
        assert _exceeds(R.aff_weight(maps, wgt, None)[0], W, b) > W.numel() // 2, "seg forgotten"


@pytest.mark.parametrize("h,w,H,Wd", R.UPSAMPLE_SHAPES)
def test_upsampling_faults_exceed_the_bound(h, w, H, Wd):
    """The 1e-7 guard dropped on a constant map; bg over all K maps instead of nk[b]; the half-pixel 0.5 missing."""
    B, Kc = 3, 3
    Rm, nk = R.refined_input(B, h * w, Kc), R.nk_input(B, Kc, Kc + 1)
    assert int(nk.min()) < Kc
    u = R.upsample(Rm, nk, h, w, H, Wd)
    b = R.bound("upsample", u["A"])
    assert bool((u["cams"][B - 1, 1] == 0).all()), "the constant map is 0 / 1e-7 = 0"
    assert _exceeds(R.upsample(Rm, nk, h, w, H, Wd, guard=0.0)["cams"], u["cams"], b) > 0, "guard dropped"
    if h * w > 1:         # one source pixel: every map is constant, all are zero
        assert _exceeds(R.upsample(Rm, nk, h, w, H, Wd, bg_all=True)["cams"][:, 0], u["cams"][:, 0], b[:, 0]) > 0, "bg over all K"
    if (h, w) != (H, Wd) and h * w > 1:
        assert _exceeds(R.upsample(Rm, nk, h, w, H, Wd, half=0.0)["cams"], u["cams"], b) > 0, "half-pixel offset missing"
    sw = u["stats"].clone()
    sw[..., 1] += sw[..., 0]                                                           # max instead of max - min
    assert _exceeds(sw, u["stats"], R.bound("stats", u["A_stats"])) > 0, "range without the minimum"


# ---------------------------------------------------------------------------------------------------------------------
# layer selection: the inputs are unambiguous

@pytest.mark.parametrize("hw", R.SEG_HW + (35, 48, 36))
@pytest.mark.parametrize("nmaps", R.SEG_NMAPS)
def test_layer_selection_inputs_are_far_from_ambiguity(hw, nmaps):
    maps = R.maps_input(3, hw, nmaps)
    sep = R.keep_separation(maps)
    assert sep >= 1000.0, f"A_l within {sep:.3g} bounds of mean A"
    s = R.seg_weights(maps)
    if nmaps > 1:
        assert bool(s["keep"].any(1).all()) and not bool(s["keep"].all(1).any()), "every image keeps some layers and drops some"
    for mode in ("matmul", "loop"):
        A32 = R.seg_weights32(maps, mode)[1]
        assert torch.equal(A32 >= A32.sum(1, keepdim=True) / nmaps, s["keep"])


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
        if name.startswith(("wc_aff_", "wc_matvec", "wc_tsym", "wc_box_mask", "wc_cam_upsample")):
            getattr(so, name).argtypes = [t for t, _ in args]
    return so


P = ctypes.c_void_p(256)            # never dereferenced: every call below is refused before any launch
Q = ctypes.c_void_p(512)
MAPS = (ctypes.c_void_p * 13)(*[256] * 13)      # a real host array (of device pointers that are never dereferenced)


def _call(so, name, order, base, kw):
    assert set(kw) <= set(base), kw          # an unknown key would leave a valid call that launches
    a = dict(base)
    a.update(kw)
    return getattr(so, name)(*[a[k] for k in order], None)


_WEIGHT = ("maps", "nmaps", "wgt", "seg", "W", "B", "L")
_WEIGHT_BASE = dict(maps=MAPS, nmaps=6, wgt=P, seg=P, W=P, B=2, L=37)


@pytest.mark.parametrize("kw", [dict(nmaps=0), dict(nmaps=13), dict(L=1), dict(B=0), dict(maps=None), dict(wgt=None), dict(W=None)])
def test_aff_weight_refusals(so, kw):
    assert _call(so, "wc_aff_weight", _WEIGHT, _WEIGHT_BASE, kw) == WC_ERR_ARG


@pytest.mark.parametrize("kw", [dict(nmaps=0), dict(nmaps=13), dict(L=1), dict(B=0), dict(maps=None), dict(rowsum=None),
                                dict(diff=None), dict(wgt=None)])
def test_aff_seg_weights_refusals(so, kw):
    order = ("maps", "nmaps", "rowsum", "diff", "wgt", "B", "L")
    assert _call(so, "wc_aff_seg_weights", order, dict(maps=MAPS, nmaps=6, rowsum=P, diff=P, wgt=P, B=2, L=37), kw) == WC_ERR_ARG


@pytest.mark.parametrize("kw", [dict(nmaps=0), dict(nmaps=13), dict(L=1), dict(L=7), dict(L=2053), dict(B=0), dict(B=65536),
                                dict(c1=None), dict(ws=None), dict(W=None), dict(wgt=None), dict(maps=None)])
def test_aff_weight_c1_refusals(so, kw):
    order = ("maps", "nmaps", "wgt", "seg", "W", "c1", "ws", "B", "L")
    base = dict(maps=MAPS, nmaps=6, wgt=P, seg=P, W=P, c1=P, ws=P, B=2, L=37)
    assert _call(so, "wc_aff_weight_c1", order, base, kw) == WC_ERR_ARG


@pytest.mark.parametrize("kw", [dict(hw=6), dict(hw=2052), dict(hw=0), dict(hw=3), dict(B=0), dict(B=65536), dict(c_next=None),
                                dict(c_next=None, hw=6, last=1), dict(W=None), dict(c=None), dict(r=None), dict(ws=None)])
def test_aff_sinkhorn_step_refusals(so, kw):
    order = ("W", "c", "r", "c_next", "ws", "B", "hw", "last")
    base = dict(W=P, c=P, r=P, c_next=P, ws=P, B=2, hw=36, last=0)
    assert _call(so, "wc_aff_sinkhorn_step", order, base, kw) == WC_ERR_ARG


@pytest.mark.parametrize("kw", [dict(hw=6), dict(hw=2052), dict(hw=0), dict(K=0), dict(K=5), dict(B=0), dict(B=65536), dict(out=Q),
                                dict(W=None), dict(r=None), dict(c=None), dict(X=None), dict(out=None), dict(y1=None), dict(ws=None)])
def test_aff_tsym_apply_refusals(so, kw):
    order = ("W", "r", "c", "X", "out", "y1", "ws", "B", "hw", "K")
    base = dict(W=P, r=P, c=P, X=Q, out=P, y1=P, ws=P, B=2, hw=36, K=3)           # out == X is dict(out=Q)
    assert _call(so, "wc_aff_tsym_apply", order, base, kw) == WC_ERR_ARG


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=65536), dict(hw=0), dict(K=0), dict(out=Q), dict(out=ctypes.c_void_p(768)),
                                dict(W=None), dict(X=None), dict(out=None)])
@pytest.mark.parametrize("transpose", [0, 1])
def test_matvec_refusals(so, kw, transpose):
    order = ("W", "X", "sin", "sout", "add", "out", "B", "hw", "K", "transpose", "recip", "alpha")
    base = dict(W=P, X=Q, sin=ctypes.c_void_p(768), sout=P, add=P, out=P, B=2, hw=35, K=3, transpose=transpose, recip=0, alpha=1.0)
    assert _call(so, "wc_matvec", order, base, kw) == WC_ERR_ARG       # out == X is dict(out=Q), out == sin dict(out=768)


@pytest.mark.parametrize("kw", [dict(B=0), dict(hw=0), dict(W=None), dict(r=None), dict(c=None), dict(T=None)])
def test_tsym_refusals(so, kw):
    assert _call(so, "wc_tsym", ("W", "r", "c", "T", "B", "hw"), dict(W=P, r=P, c=P, T=P, B=2, hw=35), kw) == WC_ERR_ARG


@pytest.mark.parametrize("kw", [dict(nbox=None), dict(maxbox=0), dict(h=1, w=6827), dict(h=6827, w=1), dict(h=83, w=83), dict(P=0),
                                dict(h=0), dict(w=0), dict(K=0), dict(cam=None), dict(pair_img=None), dict(pair_slot=None),
                                dict(V=None)])
def test_box_mask_refusals(so, kw):
    """h * w = 6827 is the first grid over the 160 KiB LDS rule (6 h w + 4 ints); 83 x 83 = 6889."""
    order = ("cam", "pair_img", "pair_slot", "V", "mask_out", "boxes", "nbox", "maxbox", "P", "h", "w", "K", "thr")
    base = dict(cam=P, pair_img=P, pair_slot=P, V=P, mask_out=P, boxes=P, nbox=P, maxbox=64, P=3, h=5, w=7, K=2, thr=0.4)
    assert _call(so, "wc_box_mask", order, base, kw) == WC_ERR_ARG
    assert (6 * 6826 + 4) * 4 <= 160 * 1024 < (6 * 6827 + 4) * 4


@pytest.mark.parametrize("kw", [dict(C=1), dict(C=5), dict(C=0), dict(B=0), dict(h=0), dict(w=0), dict(K=0), dict(H=0), dict(W=0),
                                dict(R=None), dict(nk=None), dict(stats=None), dict(cams=None)])
def test_cam_upsample_refusals(so, kw):
    """C = 1 has no class channel; C = K + 2 = 5 has more class channels than maps."""
    order = ("R", "nk", "stats", "cams", "B", "h", "w", "K", "C", "H", "W")
    base = dict(R=P, nk=P, stats=P, cams=P, B=2, h=4, w=6, K=3, C=4, H=64, W=96)
    assert _call(so, "wc_cam_upsample", order, base, kw) == WC_ERR_ARG


def test_fused_supported_values(so):
    assert [so.wc_aff_fused_supported(hw) for hw in (0, 3, 4, 6, 2048, 2052)] == [0, 0, 1, 0, 1, 0]
    assert so.wc_aff_fused_supported(-4) == 0


def test_refusals_raise_through_the_binding():
    from weclip_vit_comer_amd import _lib
    with pytest.raises(RuntimeError, match="alias"):
        _lib.lib().wc_matvec(P, Q, None, None, None, Q, 2, 35, 3, 0, 0, 1.0, None)
    with pytest.raises(RuntimeError, match="K <= 4"):
        _lib.lib().wc_aff_tsym_apply(P, P, P, Q, P, P, P, 2, 36, 5, None)
    with pytest.raises(RuntimeError, match="too large"):
        _lib.lib().wc_box_mask(P, P, P, P, None, None, None, 0, 1, 1, 6827, 1, 0.4, None)


# ---------------------------------------------------------------------------------------------------------------------
# the host's size rules are the library's

def test_host_rules_agree_with_the_library(so):
    from weclip_vit_comer_amd import cam_pipeline as CP
    for hw in range(1, 2101):
        assert bool(CP.fused_ok(hw)) == bool(so.wc_aff_fused_supported(hw)), hw
        assert CP._nblk(hw) == -(-hw // 32), hw                   # ceil(hw / 32): the sweeps' column partials
        assert CP._nblk_weight(hw) == -(-hw // 8), hw             # ceil(hw / 8): wc_aff_weight_c1's
    assert not CP.fused_ok(0)
