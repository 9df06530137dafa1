"""Every attention kernel path of csrc/attention.hip, csrc/attention_bwd.hip and the GradCAM column sums of csrc/gradcam.hip
against the fp64 reference of tests/attn_ref.py, through the C ABI.

Every output and workspace is filled with NaN (0xFF bytes) before a call: an element the kernels leave unwritten fails.  Each
checked element is held to the error-model bound derived in tests/attn_ref.py.  The inputs plant dominant scores on the edge
keys (key 0, key L-1, the first L % 64, both sides of every 64-key tile edge) from the checked rows, so a dropped, doubled
or misplaced key moves an output by O(|v|).  The reference runs on row subsets (tests/attn_ref.check_rows) and, for the
large shapes, on a few (b, h) pairs; the NaN, bit-identity and o16 == fp16(o32) checks cover whole tensors."""
import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu

F32, F16, F64, I32 = torch.float32, torch.float16, torch.float64, torch.int32


def _L():
    from weclip_vit_comer_amd import _lib as L
    return L


def _nan(n, dtype):
    t = torch.empty(n, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(255)
    return t


def _dev(x, dtype):
    t = _nan(x.numel(), dtype)
    t.copy_(x.reshape(-1).to(dtype).cuda())
    return t


def _p(t):
    return _L().ptr(t)


def _check(name, got, ref, bound):
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} elements not written (still NaN)"
    err = (got - ref).abs()
    bound = bound.expand_as(err)
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    if (err > bound).any():
        i = int(torch.argmax((err - bound).reshape(-1)))
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ref.shape))
        raise AssertionError(f"{name}: {int((err > bound).sum())} of {err.numel()} elements outside the bound, worst "
                             f"err / bound {ratio:.3g}; at {idx}: got {got.reshape(-1)[i]:.9g} ref {ref.reshape(-1)[i]:.9g}")
    WORST[name.split(" ", 1)[1]] = max(WORST.get(name.split(" ", 1)[1], 0.0), ratio)
    return ratio


WORST = {}          # kernel path / output -> worst err / bound seen


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """Prints the worst err / bound per path and output after the module (visible with -s)."""
    yield
    for k in sorted(WORST):
        print(f"WORST {k}: {WORST[k]:.3g}")


def _finite(name, t):
    n = int((~torch.isfinite(t)).sum())
    assert n == 0, f"{name}: {n} elements not written (still NaN)"


# ---------------------------------------------------------------------------------------------------------------------
# host rules of wc_attn_fwd / wc_attn_mean, mirrored

LDS_FWD = {64: 2 * (64 * (64 * 2 + 16) + 64 * 128), 32: 2 * (64 * (32 * 2 + 16) + 64 * 64)}     # bytes


def fwd_path(B, L, H, DH):
    """(NW, r, kr) that wc_attn_fwd picks: 8 waves when DH == 64 and cdiv(L, 256) H B >= 512; r = rows done by the row path
    (attn_origin, set to 0 when the row path's L + 20 + (NT / (DH / 8)) DH floats exceed the kernel's LDS); kr = keys done
    by the 8-wave VALU loop (L % 64 in [1, 8], L >= 64)."""
    nw = 8 if DH == 64 and -(-L // 256) * H * B >= 512 else 4
    r = R.origin(L)
    if r and (L + 4 + 16 + (nw * 64 // (DH // 8)) * DH) * 4 > LDS_FWD[DH]:
        r = 0
    kr = L % 64 if nw == 8 and L >= 64 and 0 < L % 64 <= R.EDGE_MAX else 0
    return nw, r, kr


def fwd_name(B, L, H, DH):
    return f"attn_fwd_kernel<{DH}, {fwd_path(B, L, H, DH)[0]}>"


def mean_name(L, DH):
    r = R.origin(L)
    return f"attn_mean_kernel<{DH}, {0 if r == 0 else (1 if r == 1 else 8)}>"


def _timed(fn):
    """Run fn with the kernel timers on; -> (fn's result, names of the kernels it launched)."""
    from weclip_vit_comer_amd import ops
    ops.KernelTimer.enable(1)
    try:
        out = fn()
        names = set(ops.KernelTimer.summary())
    finally:
        ops.KernelTimer.enable(0)
    return out, names


def run_fwd(qd, B, L, H, DH, want_o32=True):
    E = H * DH
    o16 = _nan(B * L * E, F16)
    o32 = _nan(B * L * E, F32) if want_o32 else None
    lse = _nan(B * H * L, F32)
    _L().lib().wc_attn_fwd(_p(qd), _p(o16), _p(o32), _p(lse), B, L, H, DH, _L().stream())
    torch.cuda.synchronize()
    return o16, o32, lse


def run_mean(qd, lse, B, L, H, DH):
    m = _nan(B * L * L, F32)
    _L().lib().wc_attn_mean(_p(qd), _p(lse), _p(m), B, L, H, DH, _L().stream())
    torch.cuda.synchronize()
    return m


def _bh(B, H, cap=24, seed=0):
    """All (b, h) pairs when there are few, else the corners, the batch tail and a seeded sample."""
    if B * H <= cap:
        return [(b, h) for b in range(B) for h in range(H)]
    g = torch.Generator().manual_seed(seed)
    s = {(0, 0), (B - 1, H - 1), (B - 1, 0), (0, H - 1), ((B - 1) // 8 * 8, H // 2)}
    s |= {(int(b), int(h)) for b, h in zip(torch.randint(0, B, (6,), generator=g), torch.randint(0, H, (6,), generator=g))}
    return sorted(s)


FWD_CASES = [  # (B, L, H, DH): the path each selects (NW waves, r row-path rows, kr VALU keys), see fwd_path
    *[(2, L, 2, 32) for L in (1, 2, 63, 64, 65, 129, 136, 137, 1024, 1025)],   # <32,4>; 1025: the decoder geometry, r = 1
    (1, 2561, 2, 32),           # <32,4> row-path fallback: r = 0 (L + 2068 floats > LDS) while the mean uses R = 1
    *[(2, L, 2, 64) for L in (1, 65, 197, 401, 1025, 1032)],                 # <64,4>: small batches; 1032: r = 8
    (1, 6657, 1, 64),           # <64,4> fallback: r = 0
    (9, 65, 64, 64),            # <64,8> kr = 1
    (8, 72, 64, 64),            # <64,8> kr = 8
    (10, 64, 64, 64),           # <64,8> exact tiles
    (3, 257, 96, 64),           # <64,8> r = 1, kr = 1
    (2, 1032, 52, 64),          # <64,8> r = 8, kr = 8
    (2, 1033, 52, 64),          # <64,8> no edges
    (9, 1025, 12, 64),          # <64,8> batch tail (9 images: the XCD-remapped grid rounds to 16)
    (16, 1025, 12, 64),         # <64,8> bench geometry
    (1, 4609, 28, 64),          # <64,8> row-path fallback (L + 4116 floats > LDS) with kr = 1
]
EXPECT = {  # the paths the table above claims for its fallback and 8-wave rows
    (1, 2561, 2, 32): (4, 0, 0), (1, 6657, 1, 64): (4, 0, 0), (9, 65, 64, 64): (8, 0, 1), (8, 72, 64, 64): (8, 0, 8),
    (10, 64, 64, 64): (8, 0, 0), (3, 257, 96, 64): (8, 1, 1), (2, 1032, 52, 64): (8, 8, 8), (2, 1033, 52, 64): (8, 0, 0),
    (9, 1025, 12, 64): (8, 1, 1), (16, 1025, 12, 64): (8, 1, 1), (1, 4609, 28, 64): (8, 0, 1),
}


@pytest.mark.parametrize("B,L,H,DH", FWD_CASES)
def test_forward_and_mean(B, L, H, DH):
    path = fwd_path(B, L, H, DH)
    assert EXPECT.get((B, L, H, DH), path) == path, f"case does not take the path it documents: {path}"
    if (B, L, H, DH) not in EXPECT:
        assert path[0] == 4 and path[1] == R.origin(L), path
    qkv, _ = R.make_inputs(B, L, H, DH, seed=B * 131 + L)
    qd = _dev(qkv, F16)
    (o16, o32, lse), names = _timed(lambda: run_fwd(qd, B, L, H, DH))
    assert fwd_name(B, L, H, DH) in names, names
    mean, names = _timed(lambda: run_mean(qd, lse, B, L, H, DH))
    assert mean_name(L, DH) in names, names
    for n, t in (("o16", o16), ("o32", o32), ("lse", lse), ("mean", mean)):
        _finite(f"{n}", t)
    assert torch.equal(o16, o32.half()), "o16 is not o32 rounded to fp16"
    # a second call is bit-identical; without out32 the fp16 output and lse do not change
    o16b, o32b, lseb = run_fwd(qd, B, L, H, DH)
    assert torch.equal(o16b, o16) and torch.equal(o32b, o32) and torch.equal(lseb, lse), "forward not deterministic"
    assert torch.equal(run_mean(qd, lse, B, L, H, DH), mean), "mean map not deterministic"
    o16c, _, lsec = run_fwd(qd, B, L, H, DH, want_o32=False)
    assert torch.equal(o16c, o16) and torch.equal(lsec, lse), "want_o32 off changes o16 / lse"
    # per element against fp64
    rows = R.check_rows(L)
    bh = _bh(B, H)
    O, lse_r, bO, blse = R.fwd(qkv, B, L, H, DH, rows=rows, bh=bh)
    tag = f"L={L} fwd<{DH},{path[0]}>"
    b_i = torch.tensor([b for b, _ in bh])
    h_i = torch.tensor([h for _, h in bh])
    o32h = o32.view(B, L, H, DH).cpu()[b_i[:, None], rows[None, :], h_i[:, None]]
    o16h = o16.view(B, L, H, DH).cpu()[b_i[:, None], rows[None, :], h_i[:, None]]
    _check(f"{tag} o32", o32h, O, bO)
    _check(f"{tag} o16", o16h, O, bO + R.ulp16(O))
    _check(f"{tag} lse", lse.view(B, H, L).cpu()[b_i[:, None], h_i[:, None], rows[None, :]], lse_r, blse)
    imgs = sorted({0, B - 1})
    M, bM = R.mean(qkv, B, L, H, DH, imgs, rows)
    _check(f"L={L} {mean_name(L, DH)} mean", mean.view(B, L, L).cpu()[imgs][:, rows], M, bM)


def test_every_forward_and_mean_instantiation_runs():
    """One small launch per instantiation, names from the kernel timers: all three forward and all six mean kernels."""
    cases = [(2, 65, 2, 32), (2, 129, 2, 32), (2, 136, 2, 32), (2, 65, 2, 64), (2, 1025, 2, 64), (2, 1032, 2, 64),
             (9, 65, 64, 64)]
    seen = set()
    for B, L, H, DH in cases:
        qkv, _ = R.make_inputs(B, L, H, DH, seed=L)
        qd = _dev(qkv, F16)

        def both():
            _, _, lse = run_fwd(qd, B, L, H, DH)
            run_mean(qd, lse, B, L, H, DH)
        seen |= _timed(both)[1]
    want = {f"attn_fwd_kernel<{a}>" for a in ("64, 8", "64, 4", "32, 4")}
    want |= {f"attn_mean_kernel<{d}, {r}>" for d in (64, 32) for r in (0, 1, 8)}
    assert want <= seen, f"not exercised: {sorted(want - seen)}"


# ---------------------------------------------------------------------------------------------------------------------
# backward

def run_bwd(qd, dOd, o32, lse, B, L, H, DH, Lp, with_lo=True):
    E = H * DH
    ws = [_nan(B * H * DH * Lp, F16) for _ in range(3)]
    delta = _nan(B * H * L, F32)
    hi = _nan(B * L * 3 * E, F16)
    lo = _nan(B * L * 3 * E, F16) if with_lo else None
    _L().lib().wc_attn_bwd(_p(qd), _p(dOd), _p(o32), _p(lse), _p(ws[0]), _p(ws[1]), _p(ws[2]), _p(delta), _p(hi), _p(lo),
                           B, L, Lp, H, DH, _L().stream())
    torch.cuda.synchronize()
    return hi, lo


def _assert_true_split(hi, lo):
    """hi is the fp16 nearest to hi + lo (a tie may round to the other neighbour): |lo| <= half an ulp of hi."""
    x = hi.double() + lo.double()
    r = x.to(F32).half()
    bad = r != hi
    if bad.any():
        tie = (x - hi.double()).abs() == (x - r.double()).abs()
        assert tie[bad].all(), f"hi is not fp16(hi + lo) at {int((bad & ~tie).sum())} elements"


def _sum_hl(hi, lo):
    return hi.double() + lo.double()


BWD_CASES = [(B, L, H, DH) for DH, H in ((32, 2), (64, 1)) for L in (1, 2, 63, 64, 65, 127, 128, 129, 1024, 1025)
             for B in (1, 3)]


def _bwd_case(B, L, H, DH, rows, bh, seed):
    E = H * DH
    qkv, dO = R.make_inputs(B, L, H, DH, seed=seed)
    qd, dOd = _dev(qkv, F16), _dev(dO, F16)
    _, o32, lse = run_fwd(qd, B, L, H, DH)
    Lp = -(-L // 64) * 64
    hi, lo = run_bwd(qd, dOd, o32, lse, B, L, H, DH, Lp)
    _finite("dqkv hi", hi)
    _finite("dqkv lo", lo)
    hi2, lo2 = run_bwd(qd, dOd, o32, lse, B, L, H, DH, Lp + 64)
    assert torch.equal(hi2, hi) and torch.equal(lo2, lo), "workspace slack Lp + 64 changes the result"
    hi3, lo3 = run_bwd(qd, dOd, o32, lse, B, L, H, DH, Lp)
    assert torch.equal(hi3, hi) and torch.equal(lo3, lo), "backward not deterministic"
    hi4, _ = run_bwd(qd, dOd, o32, lse, B, L, H, DH, Lp, with_lo=False)
    assert torch.equal(hi4, hi), "with_lo=False changes hi"
    _assert_true_split(hi.cpu(), lo.cpu())
    tag = f"L={L} bwd<{DH}>"
    o32c, lsec = o32.cpu(), lse.cpu()
    refs = R.bwd(qkv, dO, o32c, lsec, B, L, H, DH, rows=rows, bh=bh)
    exact = R.bwd(qkv, dO, None, None, B, L, H, DH, rows=rows, bh=bh, exact=True, fwd_err=True)
    x = _sum_hl(hi, lo).cpu().view(B, L, 3, H, DH)
    h16 = hi.cpu().view(B, L, 3, H, DH)
    b_i = torch.tensor([b for b, _ in bh])
    h_i = torch.tensor([h for _, h in bh])
    for j, name in enumerate(("dq", "dk", "dv")):
        got = x[b_i[:, None], rows[None, :], j, h_i[:, None]]
        ref, bnd = refs[j], refs[3 + j]
        _check(f"{tag} {name}", got, ref, bnd + 2.0 ** -22 * ref.abs() + R.SUB16)
        _check(f"{tag} {name}_hi", h16[b_i[:, None], rows[None, :], j, h_i[:, None]], ref, bnd + R.ulp16(ref))
        _check(f"{tag} {name}_exact_fwd", got, exact[j], exact[3 + j] + 2.0 ** -22 * exact[j].abs() + R.SUB16)
    return qkv, dO, hi, lo


@pytest.mark.parametrize("B,L,H,DH", BWD_CASES)
def test_backward(B, L, H, DH):
    _bwd_case(B, L, H, DH, R.check_rows(L), _bh(B, H), seed=L * 7 + B)


def test_backward_decoder_geometry():
    """The decoder's (16, 1024, 8, 32) on a subset of (b, h)."""
    _bwd_case(16, 1024, 8, 32, R.check_rows(1024, n_rand=16), [(0, 0), (7, 3), (15, 7), (9, 5)], seed=5)


# ---------------------------------------------------------------------------------------------------------------------
# GradCAM column sums

def run_colsum(qd, dOd, o32, lse, pair_img, L, H, DH):
    Pn, E = len(pair_img), H * DH
    pi = torch.tensor(pair_img, dtype=I32, device="cuda")
    ws = [_nan(Pn * H * L, F32) for _ in range(4)]
    c = _nan(Pn * 3 * E, F32)
    _L().lib().wc_attn_bwd_colsum(_p(qd), _p(dOd), _p(o32), _p(lse), _p(pi), _p(ws[0]), _p(ws[1]), _p(ws[2]), _p(ws[3]),
                                  _p(c), Pn, L, H, DH, _L().stream())
    torch.cuda.synchronize()
    return c


PAIRS = [2, 0, 2, 1, 0]          # repeats, out of order; P*H % 8 != 0 for H = 3 and 6
COLSUM_CASES = [(L, DH, s) for DH in (64, 32) for L in (50, 133, 136, 137, 197, 401, 1025) for s in (1.0,)] + \
    [(L, DH, 4096.0) for DH in (64, 32) for L in (137, 1025)]


@pytest.mark.parametrize("L,DH,dscale", COLSUM_CASES)
def test_colsum(L, DH, dscale):
    H = 3 if DH == 64 else 6
    E = H * DH
    assert len(PAIRS) * H % 8 != 0 and E % 64 == 0
    B = max(PAIRS) + 1
    qkv, _ = R.make_inputs(B, L, H, DH, seed=L + DH)
    _, dO = R.make_inputs(len(PAIRS), L, H, DH, seed=L + 1, plant=False, dscale=dscale, cls_zero=True)
    qd, dOd = _dev(qkv, F16), _dev(dO, F16)
    _, o32, lse = run_fwd(qd, B, L, H, DH)
    c = run_colsum(qd, dOd, o32, lse, PAIRS, L, H, DH)
    _finite("c", c)
    assert torch.equal(run_colsum(qd, dOd, o32, lse, PAIRS, L, H, DH), c), "colsum not deterministic"
    o32c, lsec = o32.cpu(), lse.cpu()
    cr, bc = R.colsum(qkv, dO, o32c, lsec, PAIRS, L, H, DH)
    tag = f"L={L} colsum<{DH}>{'' if dscale == 1 else ' x4096'}"
    _check(f"{tag} c", c.cpu(), cr, bc)
    if dscale != 1.0:
        return
    # cross-check: the patch-token sums of wc_attn_bwd's dqkv on the same inputs (one "image" per pair), the two bounds
    # added; the formulas differ by the rows of dS / P not summing exactly to 0 / 1 under the kernel's o32 / lse, which
    # the reference evaluates exactly
    pi = torch.tensor(PAIRS)
    qkv_p = qkv.view(B, L, -1)[pi].reshape(-1, 3 * E)
    o_p = o32.view(B, L, E)[pi.cuda()].reshape(-1, E).contiguous()
    l_p = lse.view(B, H, L)[pi.cuda()].contiguous()
    Lp = -(-L // 64) * 64
    hi, lo = run_bwd(_dev(qkv_p, F16), dOd, o_p, l_p, len(PAIRS), L, H, DH, Lp)
    s = _sum_hl(hi, lo).cpu().view(len(PAIRS), L, 3 * E)[:, 1:].sum(1)
    dq, dk, dv, bq, bk, bv = R.bwd(qkv_p, dO, o_p.cpu(), l_p.cpu(), len(PAIRS), L, H, DH)
    bsum = torch.stack([(b + 2.0 ** -22 * r.abs() + R.SUB16).view(len(PAIRS), H, L, DH)[:, :, 1:].sum(2)
                        for b, r in ((bq, dq), (bk, dk), (bv, dv))], 1).reshape(len(PAIRS), 3 * E)
    direct = torch.stack([r.view(len(PAIRS), H, L, DH)[:, :, 1:].sum(2) for r in (dq, dk, dv)], 1).reshape(len(PAIRS), 3 * E)
    _check(f"{tag} c_vs_bwd", c.cpu().double().view(len(PAIRS), 3 * E) - s, cr - direct, bc + bsum)
