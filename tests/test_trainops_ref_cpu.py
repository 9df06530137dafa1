"""The fp64 reference of the LayerNorm / optimizer / operand-prep kernel tests (tests/trainops_ref.py) without a GPU: it equals
fp64 torch autograd (F.layer_norm forward and backward, the sum of two norms, sigmoid(F F^T) backward, one torch.optim.AdamW step
from non-zero state), its bounds admit a plain fp32 torch evaluation at every shape of the GPU module (this is the measurement
of K) and reject the faults such kernels make, each planted in an fp32 emulation at the smallest shape that has the edge, and
every documented argument condition of the wc_* entries of csrc/norm.hip and csrc/train_ops.hip is refused before any launch."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as Fn

from tests import trainops_ref as R

F64, F32, F16 = torch.float64, torch.float32, torch.float16
WC_ERR_ARG = 1
LN_ALPHA, OUT_SCALE = R.LN_ALPHA, R.LN_OUT_SCALE


# ---------------------------------------------------------------------------------------------------------------------
# the reference is fp64 autograd

def _autograd_ln(i, two, dt, add=True, alpha=1.0):
    """F.layer_norm and its autograd in dtype dt -> y, dx (+ add), [dgamma], [dbeta] (times alpha)."""
    leaf = lambda t: t.detach().to(dt).clone().requires_grad_(True)
    x = leaf(i["x"])
    D = x.shape[1]
    ws = [leaf(i["w"])] + ([leaf(i["wb"])] if two else [])
    bs = [torch.zeros(D, dtype=dt, requires_grad=True) for _ in ws]
    bs[0] = leaf(i["b"])
    ys = [Fn.layer_norm(x, (D,), w, b, R.LN_EPS) for w, b in zip(ws, bs)]
    sum((y * i[n].to(dt)).sum() for y, n in zip(ys, ("dy", "dyb"))).backward()
    dx = x.grad + i["add"].to(dt) if add else x.grad
    return ys[0].detach(), dx, [alpha * w.grad for w in ws], [alpha * b.grad for b in bs]


@pytest.mark.parametrize("rows,D", [(5, 4), (17, 64), (33, 260)])
@pytest.mark.parametrize("two", [False, True])
def test_layernorm_reference_is_fp64_autograd(two, rows, D):
    i = R.ln_inputs(rows, D, seed=1)
    y, dx, dg, db = _autograd_ln(i, two, F64, alpha=LN_ALPHA)
    tol = lambda t: 1e-12 * max(1.0, t.abs().max().item())
    ry, _ = R.ln_fwd(i["x"], i["w"], i["b"])
    assert ry.dtype == F64 and (ry - y).abs().max().item() < tol(y)
    r = R.ln_bwd([i["dy"], i["dyb"]][:1 + two], [i["w"], i["wb"]][:1 + two], i["x"], i["add"], alpha=LN_ALPHA)
    assert (r["dx"] - dx).abs().max().item() < tol(dx)
    for k in range(1 + two):
        assert (r["dgamma"][k] - dg[k]).abs().max().item() < tol(dg[k])
        assert (r["dbeta"][k] - db[k]).abs().max().item() < tol(db[k])
    # the companions dominate their outputs
    assert (r["A_dx"] >= r["dx"].abs() * (1 - 1e-12)).all() and (r["A_dgamma"][0] >= r["dgamma"][0].abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("n", [5, 68])
def test_gram_reference_is_fp64_autograd(n):
    g = torch.Generator().manual_seed(n)
    F = torch.randn(2, n, 16, generator=g, dtype=F64, requires_grad=True)
    AP = torch.sigmoid(F @ F.transpose(1, 2) * 0.2)
    dAP = torch.randn(2, n, n, generator=g, dtype=F64)
    (AP * dAP).sum().backward()
    S, A = R.gram(dAP, AP.detach(), 0.2)
    assert (S @ F.detach() - F.grad).abs().max().item() < 1e-12 * F.grad.abs().max().item()
    assert torch.equal(S, S.transpose(1, 2)) and (A >= S.abs()).all()


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("grp", R.ADAMW_GROUPS, ids=str)
def test_adamw_reference_is_torch_adamw_in_fp64(grp, step):
    p, g, m, v = (t.double() for t in R.adamw_inputs(300, seed=step))
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    opt = torch.optim.AdamW([q], lr=grp["lr"], betas=R.ADAMW_BETAS, eps=R.ADAMW_EPS, weight_decay=grp["weight_decay"], foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    po, mo, vo, Ap, Am, Av = R.adamw(p, g, m, v, step, **grp)
    st = opt.state[q]
    assert float(st["step"]) == step
    assert (po - q.detach()).abs().max().item() <= 1e-12 * q.detach().abs().max().item()
    assert (mo - st["exp_avg"]).abs().max().item() < 1e-15 and (vo - st["exp_avg_sq"]).abs().max().item() < 1e-15
    assert (Am >= mo.abs() * (1 - 1e-12)).all() and (Av >= vo * (1 - 1e-12)).all()


def test_plain_references():
    """Column sum, transpose, column-scale split and weight conversion against their one-line definitions."""
    src = R.colsum_input(257, 300, 304)
    assert torch.isnan(src[:, 300:]).all() and not torch.isnan(src[:, :300]).any()
    assert torch.equal(src[:, :300].half().float(), src[:, :300])
    s, A = R.colsum(src[:, :300], -0.5)
    assert torch.equal(s, -0.5 * src[:, :300].double().sum(0)) and (A >= s.abs() * (1 - 1e-12)).all()
    x = R.weight_values((3, 7, 5))
    hi, lo = R.transpose(x, 9, 0.25)
    assert hi.shape == (5, 2 * 9 + 7) and (hi[:, 7:9] == 0).all() and (lo[:, 16:18] == 0).all()
    assert hi[3, 9 + 2] == (x[1, 2, 3] * 0.25).half() and hi[4, 18 + 6] == (x[2, 6, 4] * 0.25).half()
    h, l = R.split16(x)
    assert torch.equal(h, x.half()) and torch.equal(l, (x - x.half().float()).half())
    assert ((h.double() + l.double() - x.double()).abs() <= R.hl_bound(x.double())).all()
    assert (l != 0).any() and (h == 0).any() and ((h.float().abs() < 6e-5) & (h != 0)).any(), "values must reach the fp16 subnormals"
    y, A = R.colscale(x[0], torch.tensor([[2.0] * 5, [3.0] * 5]), 4, -0.5)
    assert torch.equal(y[:4], -1.0 * x[0, :4].double()) and torch.equal(y[4:], -1.5 * x[0, 4:].double()) and torch.equal(A, y.abs())
    a, b = R.weight_values((68, 8)), R.weight_values((60, 8), seed=1)
    chi, clo, chiT, cloT = R.convert_weights([a, b])
    assert chi.shape == (128, 8) and chiT.shape == (8, 128) and torch.equal(chiT.t()[68:], b.half()) and torch.equal(cloT.t(), clo)
    assert R.convert_weights([R.weight_values((7, 5))])[2].shape == (5, 64)


# ---------------------------------------------------------------------------------------------------------------------
# the bounds admit the fp32 emulation at every shape of the GPU module: the measurement of K

def _ratio(got, ref, A):
    """worst |got - ref| / (EPS A); an element with A == 0 must be exact."""
    err = (got.double() - ref).abs()
    assert (err[A == 0] == 0).all()
    return (err / (R.EPS * A).clamp(min=1e-300)).max().item()


def _measure():
    w = {k: 0.0 for k in R.K}
    up = lambda k, v: w.__setitem__(k, max(w[k], v))
    for rows, D in R.LN_FWD_SHAPES:
        i = R.ln_inputs(rows, D)
        y, A = R.ln_fwd(i["x"], i["w"], i["b"])
        up("ln_y", _ratio(Fn.layer_norm(i["x"], (D,), i["w"], i["b"], R.LN_EPS), y, A))
    cases = [(r, D, False) for D in R.LN_BWD_D for r in R.LN_BWD_ROWS] + [(r, D, False) for r, D in R.LN_BWD_GRID]
    cases += [(r, D, True) for D in R.LN_BWD2_D for r in R.LN_BWD_ROWS + (R.LN_GRID_ROWS,)]
    for rows, D, two in cases:
        i = R.ln_inputs(rows, D)
        for add in (True, False):
            _, dx, dg, db = _autograd_ln(i, two, F32, add, LN_ALPHA)
            r = R.ln_bwd([i["dy"], i["dyb"]][:1 + two], [i["w"], i["wb"]][:1 + two], i["x"], i["add"] if add else None, alpha=LN_ALPHA)
            up("ln_dx", _ratio(dx, r["dx"], r["A_dx"]))
            for k in range(1 + two):
                up("ln_dgamma", _ratio(dg[k], r["dgamma"][k], r["A_dgamma"][k]))
                up("ln_dbeta", _ratio(db[k], r["dbeta"][k], r["A_dbeta"][k]))
    for Rr, C, ld in R.COLSUM_SHAPES:
        src = R.colsum_input(Rr, C, ld)[:, :C]
        for alpha, _ in R.colsum_cases(Rr):
            s, A = R.colsum(src, alpha)
            up("colsum", _ratio(src.sum(0) * torch.tensor(alpha, dtype=F32), s, A))
    for n in R.GRAM_N:
        d, a = R.gram_inputs(2, n)
        for scale in (1.0, 0.5):
            S, A = R.gram(d, a, scale)
            z = d * a * (1 - a)
            up("gram", _ratio(scale * (z + z.transpose(1, 2)), S, A))
    for rows, C, rpb, _ in R.COLSCALE_SHAPES:
        x, cs = R.colscale_inputs(rows, C, rpb)
        for alpha in (1.0, -0.5):
            y, A = R.colscale(x, cs, rpb, alpha)
            up("colscale", _ratio(alpha * x * cs.repeat_interleave(rpb, 0), y, A))
    for n in R.ADAMW_SIZES:
        p, g, m, v = R.adamw_inputs(n)
        for grp in R.ADAMW_GROUPS:
            for step in (1, 1000):
                ref = R.adamw(p, g, m, v, step, **grp)
                got = R.adamw(p, g, m, v, step, dt=F32, **grp)
                for k, name in enumerate(("adamw_p", "adamw_m", "adamw_v")):
                    up(name, _ratio(got[k], ref[k], ref[3 + k]))
    return w


def test_bounds_admit_the_fp32_emulation():
    w = _measure()
    for k in sorted(w):
        print(f"K measured {k}: {w[k]:.3f}; trainops_ref.K_MEASURED {R.K_MEASURED[k]}, K {R.K[k]}")
    for k in w:
        # (fp32 torch on the CPU: its last bits may differ between machines, hence the window)
        assert w[k] / 1.25 <= R.K_MEASURED[k] <= 1.25 * w[k], f"trainops_ref.K_MEASURED[{k}] is not the measured worst ratio {w[k]:.3f}"
        assert R.K[k] == math.ceil(4 * R.K_MEASURED[k]), k
        assert w[k] <= R.K[k]


def test_drift_bound_admits_an_fp32_trajectory():
    """Five fp32 steps on their own state against the fp64 trajectory, within the bound R.adamw_drift carries along; a
    trajectory whose third step skips the weight decay leaves it."""
    sched = dict(warmup_iter=2, warmup_ratio=1e-3, max_iter=50, power=0.9)
    for n in (4, 2 * 16384 + 5):
        p0 = R.adamw_inputs(n, seed=5)[0]
        for grp0 in R.ADAMW_GROUPS:
            ref, E = (p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)), tuple(torch.zeros(n, dtype=F64) for _ in range(3))
            st, bad = (p0, torch.zeros(n), torch.zeros(n)), (p0, torch.zeros(n), torch.zeros(n))
            for it in range(5):
                g = torch.randn(n, generator=torch.Generator().manual_seed(100 + it)) * (0.1 + it)
                g[it::7] = 0.0
                grp = dict(grp0, lr=grp0["lr"] * R.poly_lr_mult(it, **sched))
                ref, E = R.adamw_drift(E, ref, g, it + 1, **grp)
                st = R.adamw(st[0], g, st[1], st[2], it + 1, dt=F32, **grp)[:3]
                bad = R.adamw(bad[0], g, bad[1], bad[2], it + 1, dt=F32, **dict(grp, weight_decay=0.0 if it == 2 else grp["weight_decay"]))[:3]
            worst = [((st[j].double() - ref[j]).abs() / E[j].clamp(min=1e-300)).max().item() for j in range(3)]
            print(f"n={n} {grp0}: fp32 trajectory, worst err / drift bound p {worst[0]:.3g} m {worst[1]:.3g} v {worst[2]:.3g}")
            assert max(worst) <= 1
            assert ((bad[0].double() - ref[0]).abs() > E[0]).any(), "a skipped weight decay is admissible"


# ---------------------------------------------------------------------------------------------------------------------
# the bounds reject planted faults, each in an fp32 emulation written from the formula

def ln32(i, two=False, fault=None, add=True, alpha=LN_ALPHA):
    """LayerNorm forward and backward in fp32, step by step -> y, dx, [dgamma], [dbeta]."""
    x = i["x"]
    rows, D = x.shape
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).sum(-1, keepdim=True) / (D - 1 if fault == "variance_over_D_minus_1" else D)
    rstd = 1 / (var.sqrt() + R.LN_EPS) if fault == "eps_outside_the_square_root" else 1 / (var + R.LN_EPS).sqrt()
    xhat = (x - mean) * rstd
    y = xhat * i["w"] + i["b"]
    dys = [i["dy"], i["dyb"]][:1 + two]
    ws = [i["w"], i["wb"]][:1 + two]
    if fault == "second_gamma_for_both_norms":
        ws = [i["wb"], i["wb"]]
    g = sum(d * w for d, w in zip(dys, ws))
    keep = torch.ones(rows, 1)
    if fault == "xhat_term_dropped_in_the_last_row":
        keep[-1] = 0
    dx = rstd * (g - g.mean(-1, keepdim=True) - keep * xhat * (g * xhat).mean(-1, keepdim=True))
    if add:
        dx = dx + i["add"]
    dg = [(d * xhat).sum(0) for d in dys]
    db = [d.sum(0) for d in dys]
    if fault == "dbeta_from_g":
        db = [(d * w).sum(0) for d, w in zip(dys, ws)]
    if fault == "dead_row_counted_into_dgamma":
        dg = [s + d[-1] * xhat[-1] for s, d in zip(dg, dys)]
    return y, dx, [alpha * t for t in dg], [alpha * t for t in db]


def _ln_check(i, two, got):
    """-> {output: worst err / bound} of an emulation result against the reference."""
    y, A = R.ln_fwd(i["x"], i["w"], i["b"])
    r = R.ln_bwd([i["dy"], i["dyb"]][:1 + two], [i["w"], i["wb"]][:1 + two], i["x"], i["add"], alpha=LN_ALPHA)
    out = {"y": _ratio(got[0], y, A) / R.K["ln_y"], "dx": _ratio(got[1], r["dx"], r["A_dx"]) / R.K["ln_dx"]}
    out["dx16"] = ((got[1] * torch.tensor(OUT_SCALE, dtype=F32)).half().double() - OUT_SCALE * r["dx"]).abs().div(
        R.dx16_bound(r["dx"], R.K["ln_dx"] * R.EPS * r["A_dx"])).max().item()
    for k in range(1 + two):
        out[f"dgamma{k}"] = _ratio(got[2][k], r["dgamma"][k], r["A_dgamma"][k]) / R.K["ln_dgamma"]
        out[f"dbeta{k}"] = _ratio(got[3][k], r["dbeta"][k], r["A_dbeta"][k]) / R.K["ln_dbeta"]
    return out


# fault -> (rows, D, two norms, the outputs that must leave their bound): the smallest shape with the edge -- one row group plus
# one live row (17) for the faults of the last row, the narrowest row otherwise
LN_FAULTS = {
    "variance_over_D_minus_1": (5, 4, False, ("y", "dx", "dx16", "dgamma0")),
    "eps_outside_the_square_root": (5, 4, False, ("y", "dx", "dx16", "dgamma0")),
    "xhat_term_dropped_in_the_last_row": (17, 4, False, ("dx", "dx16")),
    "dbeta_from_g": (1, 4, False, ("dbeta0",)),
    "dead_row_counted_into_dgamma": (17, 4, False, ("dgamma0",)),
    "second_gamma_for_both_norms": (1, 4, True, ("dx", "dx16")),
}


@pytest.mark.parametrize("fault", LN_FAULTS)
def test_bounds_reject_planted_layernorm_fault(fault):
    rows, D, two, outs = LN_FAULTS[fault]
    i = R.ln_inputs(rows, D)
    good, bad = _ln_check(i, two, ln32(i, two)), _ln_check(i, two, ln32(i, two, fault))
    print(f"{fault}: worst err / bound {({k: round(bad[k], 3) for k in outs})}; fault-free {max(good.values()):.3g}")
    assert max(good.values()) <= 1, f"the fault-free emulation is outside the bound: {good}"
    for k in outs:
        assert bad[k] > 1, f"the planted fault is admissible in {k}"


def _round_down(x):
    """fp16 of x rounded toward zero."""
    h = x.half()
    up = h.float().abs() > x.abs()
    return torch.where(up, (h.view(torch.int16) - 1).view(F16), h)


def test_bounds_reject_planted_gram_faults():
    n = 68                                   # two tiles: the pair (0, 1) is the first off-diagonal one
    d, a = R.gram_inputs(1, n)
    S, A = R.gram(d, a, 0.5)
    b32 = R.K["gram"] * R.EPS * A
    z = d * a * (1 - a)
    good = 0.5 * (z + z.transpose(1, 2))
    hi, lo = R.split16(good)
    assert ((good.double() - S).abs() <= b32).all() and ((hi.double() - S).abs() <= R.h_bound(S, b32)).all()
    assert ((hi.double() + lo.double() - S).abs() <= R.hl_bound(S, b32)).all()
    # z^T of the tile (0, 1) taken from the tile (1, 1) in place of (1, 0)
    zt = z.transpose(1, 2).clone()
    zt[:, 0:4, 64:68] = z[:, 64:68, 64:68].transpose(1, 2)
    bad = 0.5 * (z + zt)
    over = ((bad.double() - S).abs() > b32)
    print(f"zT_from_the_wrong_tile: {int(over.sum())} elements outside the bound")
    assert over[:, 0:4, 64:68].any() and not over[:, :64, :64].any()
    assert ((bad.half().double() - S).abs() > R.h_bound(S, b32)).any()
    # lo computed from the rounded-down value: hi + lo is then one fp16 ulp off wherever hi was rounded up
    lo_bad = (good - _round_down(good).float()).half()
    over = (hi.double() + lo_bad.double() - S).abs() > R.hl_bound(S, b32)
    print(f"lo_from_the_rounded_down_value: {int(over.sum())} of {over.numel()} elements outside the bound")
    assert over.any()


def test_bit_exact_references_reject_planted_faults():
    x = R.weight_values((1, 5, 3))
    hi, lo = R.transpose(x, 5)
    bad = hi.clone()
    bad[2, 4], bad[2, 3] = hi[2, 3].clone(), hi[2, 4].clone()            # one element displaced by one column
    assert not torch.equal(bad.view(torch.int16), hi.view(torch.int16))
    w = R.weight_values((7, 5))
    chi, clo, _, _ = R.convert_weights([w])
    lo_bad = (w - _round_down(w).float()).half()
    assert not torch.equal(lo_bad.view(torch.int16), clo.view(torch.int16))
    assert torch.equal(torch.tensor([0.0, -0.0]).half().view(torch.int16), torch.tensor([0, -32768], dtype=torch.int16))


def adamw32(p, g, m, v, step, lr, weight_decay, fault=None):
    """The documented update order in fp32 with one fault planted."""
    b1, b2 = R.ADAMW_BETAS
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    if fault == "bias_corrections_swapped":
        bc1, bc2 = bc2, bc1
    f = lambda val: torch.tensor(val, dtype=F64).float()
    decay, ss, bs, eps = f(1.0 - lr * weight_decay), f(lr / bc1), f(bc2 ** 0.5), f(R.ADAMW_EPS)
    mo = m + f(1.0 - b1) * (g - m)
    vo = v * f(b2) + (f(1.0 - b2) * g) * g
    denom = (vo / (bs * bs) + eps).sqrt() if fault == "eps_inside_the_square_root" else vo.sqrt() / bs + eps
    po = (p - ss * (mo / denom)) * decay if fault == "decay_after_the_update" else p * decay - ss * (mo / denom)
    if fault == "last_four_elements_skipped":
        po[-4:], mo[-4:], vo[-4:] = p[-4:], m[-4:], v[-4:]
    return po, mo, vo


@pytest.mark.parametrize("fault", ["bias_corrections_swapped", "decay_after_the_update", "eps_inside_the_square_root",
                                   "last_four_elements_skipped"])
def test_bounds_reject_planted_adamw_fault(fault):
    n, step, grp = 4, 2, R.ADAMW_GROUPS[1]                 # one 16-byte access: the smallest tensor; its last four = all of it
    p, g, m, v = R.adamw_inputs(n)
    ref = R.adamw(p, g, m, v, step, **grp)
    names = ("adamw_p", "adamw_m", "adamw_v")
    good = [_ratio(t, ref[k], ref[3 + k]) / R.K[names[k]] for k, t in enumerate(adamw32(p, g, m, v, step, **grp))]
    bad = [_ratio(t, ref[k], ref[3 + k]) / R.K[names[k]] for k, t in enumerate(adamw32(p, g, m, v, step, fault=fault, **grp))]
    print(f"{fault}: worst err / bound p {bad[0]:.3g} m {bad[1]:.3g} v {bad[2]:.3g}; fault-free {max(good):.3g}")
    assert max(good) <= 1, "the fault-free emulation is outside the bound"
    assert bad[0] > 1, "the planted fault is admissible"
    if fault == "last_four_elements_skipped":
        assert bad[1] > 1 and bad[2] > 1


# ---------------------------------------------------------------------------------------------------------------------
# C-ABI refusals, before any launch (none of the pointers is ever dereferenced)

def _P(i, off=0):
    return ctypes.c_void_p(4096 * (i + 1) + off)


# every entry: its arguments in header order (without the stream) with values of a valid call
ENTRIES = {
    "wc_layernorm": dict(x=_P(0), ldx=64, w=_P(1), b=_P(2), eps=1e-5, y32=_P(3), y16=_P(4), y16lo=_P(5), rows=5, D=64),
    "wc_layernorm_bwd": dict(dy=_P(0), x=_P(1), w=_P(2), add=_P(3), eps=1e-5, dx32=_P(4), dx16=_P(5), out_scale=1.0, part=_P(6),
                             dgb=_P(7), alpha=1.0, rows=5, D=64),
    "wc_layernorm_bwd_h": dict(dy16=_P(0), x=_P(1), w=_P(2), add=_P(3), eps=1e-5, dx32=_P(4), dx16=_P(5), out_scale=1.0, part=_P(6),
                               dgb=_P(7), alpha=1.0, rows=5, D=64),
    "wc_layernorm_bwd2_h": dict(dya16=_P(0), wa=_P(1), dyb16=_P(2), wb=_P(3), x=_P(4), add=_P(5), eps=1e-5, dx32=_P(6), dx16=_P(7),
                                out_scale=1.0, part=_P(8), dgba=_P(9), dgbb=_P(10), alpha=1.0, rows=5, D=64),
    "wc_colsum": dict(src=_P(0), src_f32=1, ld=8, part=_P(1), out=_P(2), R=5, C=8, alpha=1.0, round16=0),
    "wc_transpose_f16": dict(src=_P(0), src_f32=1, ld=8, sSrc=40, hi=_P(1), lo=_P(2), ldo=64, oR=5, batch=2, R=5, C=8, scale=1.0),
    "wc_sigmoid_gram_bwd": dict(dAP=_P(0), AP=_P(1), hi=_P(2), lo=_P(3), B=2, n=5, ldo=64, scale=1.0),
    "wc_colscale_split": dict(x=_P(0), cs=_P(1), out32=_P(2), hi=_P(3), lo=_P(4), rows=6, C=8, rows_per_batch=3, alpha=1.0),
    "wc_convert_weights": dict(table=_P(0), count=2, blocks_per_tensor=32),
    "wc_adamw_multi": dict(table=_P(0), count=2, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, bias_correction1=0.1,
                           bias_correction2=0.001, blocks_per_tensor=64),
}


@pytest.fixture(scope="module")
def so():
    from weclip_vit_comer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    protos = {name: args for name, _, args in _lib.parse_header()}
    for name, a in ENTRIES.items():
        assert [n for _, n in protos[name]] == list(a) + ["stream"], f"{name}: ENTRIES does not follow the header"
        getattr(so, name).argtypes = [t for t, _ in protos[name]]
    return so


def _refused(so, name, kw):
    a = dict(ENTRIES[name])
    assert set(kw) <= set(a), kw          # an unknown key would leave a valid call that launches
    a.update(kw)
    return getattr(so, name)(*a.values(), None) == WC_ERR_ARG


def test_the_refusal_tests_cover_every_entry_of_the_two_files():
    from weclip_vit_comer_amd import _lib
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
    names = set()
    for f in ("norm.hip", "train_ops.hip"):
        names |= set(re.findall(r'extern "C" int (wc_\w+)\(', open(os.path.join(csrc, f)).read()))
    assert names == set(ENTRIES)
    tested = {n for n, _ in _REFUSALS}
    assert tested == names


_M16, _M8 = 4, 4          # pointer offsets that break the 16-byte (fp16: 8-byte) alignment
_LN_BWD = [dict(x=None), dict(w=None), dict(part=None), dict(dgb=None), dict(rows=0), dict(rows=-1), dict(D=0), dict(D=6), dict(D=1028),
           dict(dx32=None, dx16=None), dict(x=_P(1, _M16)), dict(w=_P(2, _M16)), dict(add=_P(3, _M16)), dict(dx32=_P(4, _M16)),
           dict(dx16=_P(5, _M8))]
_REFUSALS = (
    [("wc_layernorm", kw) for kw in [dict(x=None), dict(w=None), dict(b=None), dict(rows=0), dict(rows=-2), dict(D=0), dict(D=6, ldx=8),
                                     dict(D=4100, ldx=4100), dict(ldx=60), dict(ldx=66), dict(y32=None, y16=None),
                                     dict(y32=None, y16=None, y16lo=None)]] +
    [("wc_layernorm_bwd", kw) for kw in _LN_BWD + [dict(dy=None), dict(dy=_P(0, _M16))]] +
    [("wc_layernorm_bwd_h", kw) for kw in _LN_BWD + [dict(dy16=None), dict(dy16=_P(0, _M8))]] +
    [("wc_layernorm_bwd2_h", kw) for kw in [dict(dya16=None), dict(dyb16=None), dict(wa=None), dict(wb=None), dict(x=None),
                                            dict(part=None), dict(dgba=None), dict(dgbb=None), dict(rows=0), dict(D=0), dict(D=6),
                                            dict(D=260), dict(dx32=None, dx16=None), dict(x=_P(4, _M16)), dict(wa=_P(1, _M16)),
                                            dict(wb=_P(3, _M16)), dict(add=_P(5, _M16)), dict(dx32=_P(6, _M16)), dict(dx16=_P(7, _M8)),
                                            dict(dya16=_P(0, _M8)), dict(dyb16=_P(2, _M8))]] +
    [("wc_colsum", kw) for kw in [dict(src=None), dict(part=None), dict(out=None), dict(R=0), dict(C=0), dict(ld=7),
                                  dict(R=256 * 65535 + 1)]] +
    [("wc_transpose_f16", kw) for kw in [dict(src=None), dict(hi=None), dict(batch=0), dict(R=0), dict(C=0), dict(ld=7), dict(oR=4),
                                         dict(ldo=9), dict(batch=65536, ldo=1 << 20)]] +
    [("wc_sigmoid_gram_bwd", kw) for kw in [dict(dAP=None), dict(AP=None), dict(hi=None), dict(B=0), dict(n=0), dict(n=65536, ldo=65536),
                                            dict(ldo=4)]] +
    [("wc_colscale_split", kw) for kw in [dict(x=None), dict(hi=None), dict(rows=0), dict(C=0), dict(rows_per_batch=0)]] +
    [("wc_convert_weights", kw) for kw in [dict(table=None), dict(count=0), dict(count=-1), dict(count=65536), dict(blocks_per_tensor=0)]] +
    [("wc_adamw_multi", kw) for kw in [dict(table=None), dict(count=0), dict(count=65536), dict(blocks_per_tensor=0),
                                       dict(bias_correction1=0.0), dict(bias_correction1=-0.1), dict(bias_correction2=0.0),
                                       dict(bias_correction2=-1.0)]]
)


def _id(v):
    name, kw = v
    show = lambda x: ("NULL" if x.value is None else f"p+{x.value % 4096}") if isinstance(x, ctypes.c_void_p) else x
    return name[3:] + ":" + ",".join(f"{k}={show(x)}" for k, x in kw.items())


@pytest.mark.parametrize("case", _REFUSALS, ids=_id)
def test_trainops_refusals(so, case):
    name, kw = case
    assert _refused(so, name, kw), f"{name} accepted {kw}"
