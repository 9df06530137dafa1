"""Every deformable-attention kernel path of csrc/msdeform.hip (and the prep kernels of csrc/comer.hip) against the fp64
reference of tests/msda_ref.py, through the C ABI the way the CoMer engine calls it.

Every output and workspace is filled with NaN (0xFF bytes) before a call: an element the kernels leave unwritten fails.
Bounds come from the error model, per element:
  fp32 arithmetic     |got - ref| <= c 2^-24 sum|terms|, c = 64 (sum|terms|: the same evaluation on absolute values);
  fp16 inputs         the reference's inputs are rounded to fp16 first, then the same bound;
  fp16 outputs        one fp16 ulp of the reference on top;
  grad_value          (pairs(pixel) / 2 + 1) q + c 2^-24 sum|terms|, q = max|gout| max(1, max|attn|) 2^-24: the fixed-point
                      quantum of the bucketed gather (pairs = (sample, corner) pairs with a non-zero weight on the pixel);
  location gradients  only samples farther than 1e-3 pixel from a kink of the bilinear derivative.
Sampling locations are drawn on a 2^-12 grid and the fused tests use power-of-two maps with offsets on a 2^-8 grid, so that
loc * size - 0.5 (and the fused loc = ref + offset / size) is exact in fp32: the bounds above need no position term."""
import numpy as np
import pytest
import torch

from tests import msda_ref as R

pytestmark = pytest.mark.gpu

F32, F16, F64, I32 = torch.float32, torch.float16, torch.float64, torch.int32
U = R.U
C = 64                        # the c of the fp32 bound


def _L():
    from weclip_vit_comer_amd import _lib as L
    return L


def _nan(n, dtype, skew=0):
    """Device buffer of n elements with every byte 0xFF (NaN for f32 / f16, -1 for int32); skew: start that many 4-byte words
    past a 16-byte boundary."""
    extra = skew * 4 // torch.tensor([], dtype=dtype).element_size()
    t = torch.empty(n + extra, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(255)
    return t[extra:]


def _dev(x, dtype, skew=0):
    t = _nan(x.numel(), dtype, skew)
    t.copy_(x.reshape(-1).to(dtype).cuda())
    return t


def _ptr(t):
    return _L().ptr(t)


def _hs(shapes):
    return _L().int_array([v for hw in shapes for v in hw])


def _ulp16(r):
    a = r.abs().clamp(min=2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def _check(name, got, ref, bound, mask=None):
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} elements not written (still NaN)"
    err = (got - ref).abs()
    if mask is not None:
        err, bound = err[mask], bound.expand_as(ref)[mask]
    bound = bound.expand_as(err)
    bad = err > bound
    if bad.any():
        ratio = (err / bound.clamp(min=1e-300)).max().item()
        i = int(torch.argmax((err - bound).reshape(-1)))
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst err / bound "
                             f"{ratio:.3g}; e.g. got {got.reshape(-1)[i] if mask is None else got[mask][i]:.9g} "
                             f"ref {ref.reshape(-1)[i] if mask is None else ref[mask][i]:.9g}")


def _grid(x, step=2.0 ** -12):
    return torch.round(x / step) * step


def _edge_px(size):
    """Pixel coordinates at the edges: exactly -1 and size (excluded), just inside them, the first / last pixel centre,
    far outside; and loc 0 and 1."""
    e = 2.0 ** -8
    px = [-1.0, float(size), -1.0 + e, size - e, 0.0, size - 1.0, -37.25, 5.0 * size + 3.25]
    return [(p + 0.5) / size for p in px] + [0.0, 1.0]


def _inputs(shapes, N, Lq, M, D, P, seed, lo=-0.15, hi=1.15, edges=True, attn="softmax"):
    g = torch.Generator().manual_seed(seed)
    nL = len(shapes)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(N, S, M, D, generator=g)
    loc = _grid(torch.rand(N, Lq, M, nL, P, 2, generator=g) * (hi - lo) + lo)
    if edges:                                  # query 0 of every image: the edge coordinates, x in even heads, y in odd ones
        for l, (H, W) in enumerate(shapes):
            for k in range(M * P):
                m, p = divmod(k, P)
                e = _edge_px((W, H)[m % 2])
                loc[:, 0, m, l, p, m % 2] = _grid(torch.tensor(e[(k + l) % len(e)]))
    if attn == "softmax":
        a = torch.softmax(torch.randn(N, Lq, M, nL * P, generator=g), -1).view(N, Lq, M, nL, P)
    else:
        a = torch.randn(N, Lq, M, nL, P, generator=g) * attn
    gout = torch.randn(N, Lq, M * D, generator=g)
    return value, loc, a.float(), gout


class _Ref:
    """fp64 forward / backward of the definition and its error scales, on the inputs as the kernels see them."""

    def __init__(self, value, shapes, loc, attn, gout):
        self.shapes = shapes
        v, l, a = [t.double().requires_grad_(True) for t in (value, loc, attn)]
        out = R.msda_fp64(v, shapes, l, a)
        out.backward(gout.double().reshape(out.shape))
        self.out, self.gv, self.gl, self.ga = out.detach(), v.grad, l.grad, a.grad
        self.out_abs, self.ga_abs, self.gv_abs = R.abs_scales(value, shapes, loc, attn, gout)
        self.gl_abs = R.loc_grad_abs(value, shapes, loc, attn, gout)
        self.far = R.kink_distance(shapes, loc) > 1e-3      # (the derivative along x has its kinks where x is an integer)
        self.pairs = R.pair_counts(shapes, loc, value.shape[1])[..., None]
        self.q = gout.abs().max().item() * max(1.0, attn.abs().max().item()) * U

    def gv_bound(self):
        return (self.pairs / 2 + 1) * self.q + C * U * self.gv_abs


def _far_fraction(far):
    f = far.float().mean().item()
    assert f >= 0.9, f"only {f:.1%} of the location-gradient elements are away from a kink (>= 90 % must be checked)"
    return f


def _fwd(kind, value, shapes, loc, attn, M, D, P, v16=False, outs=("out",), skew=0):
    L = _L()
    N, S = value.shape[:2]
    Lq = loc.shape[1]
    val = _dev(value, F16 if v16 else F32, skew)
    out = _nan(N * Lq * M * D, F32) if "out" in outs else None
    out16 = _nan(N * Lq * M * D, F16) if "out16" in outs else None
    locd, attnd = _dev(loc, F32), _dev(attn, F32)            # (held until the kernels ran: a freed block is reused at once)
    if kind == "fwd":
        L.lib().wc_msda_fwd(_ptr(val), _hs(shapes), len(shapes), _ptr(locd), _ptr(attnd), _ptr(out),
                            N, Lq, M, D, P, L.stream())
    else:
        L.lib().wc_msda_fwd_h(_ptr(val), int(v16), _hs(shapes), len(shapes), _ptr(locd), _ptr(attnd),
                              _ptr(out), _ptr(out16), N, Lq, M, D, P, L.stream())
    torch.cuda.synchronize()
    return out, out16


def _ws(N, M, S, nL, Lq, P):
    return _nan(N * M * (2 * S + nL * Lq * P * 8), I32), _nan(2, I32)


def _bwd(kind, value, shapes, loc, attn, gout, M, D, P, v16=False, g16=False, gvs=("gv",), skew=0):
    L = _L()
    N, S = value.shape[:2]
    Lq, nL = loc.shape[1], len(shapes)
    val = _dev(value, F16 if v16 else F32, skew)
    go = _dev(gout, F16 if g16 else F32)
    gv = _nan(N * S * M * D, F32) if "gv" in gvs else None
    gv16 = _nan(N * S * M * D, F16) if "gv16" in gvs else None
    gl, ga = _nan(loc.numel(), F32), _nan(attn.numel(), F32)
    ws, gmax = _ws(N, M, S, nL, Lq, P)
    locd, attnd = _dev(loc, F32), _dev(attn, F32)
    if kind == "bwd":
        L.lib().wc_msda_bwd(_ptr(val), _hs(shapes), nL, _ptr(locd), _ptr(attnd), _ptr(go), _ptr(gv),
                            _ptr(gl), _ptr(ga), _ptr(gmax), _ptr(ws), N, Lq, M, D, P, L.stream())
    else:
        L.lib().wc_msda_bwd_h(_ptr(val), int(v16), _hs(shapes), nL, _ptr(locd), _ptr(attnd), _ptr(go),
                              int(g16), _ptr(gv), _ptr(gv16), _ptr(gl), _ptr(ga), _ptr(gmax), _ptr(ws), N, Lq, M, D, P,
                              L.stream())
    torch.cuda.synchronize()
    return gv, gv16, gl, ga


def _round_inputs(value, gout, v16, g16):
    return (value.half().float() if v16 else value), (gout.half().float() if g16 else gout)


def _check_fwd(tag, ref, out, out16):
    b = C * U * ref.out_abs
    if out is not None:
        _check(f"{tag} out", out, ref.out, b)
    if out16 is not None:
        _check(f"{tag} out16", out16, ref.out, b + _ulp16(ref.out))
    if out is not None and out16 is not None:
        assert torch.equal(out16, out.half()), f"{tag}: out16 is not out rounded to fp16"


def _check_gv(tag, ref, gv, gv16):
    b = ref.gv_bound()
    if gv is not None:
        _check(f"{tag} gvalue", gv, ref.gv, b)
    if gv16 is not None:
        _check(f"{tag} gvalue16", gv16, ref.gv, b + _ulp16(ref.gv))
    if gv is not None and gv16 is not None:
        assert torch.equal(gv16, gv.half()), f"{tag}: gvalue16 is not gvalue rounded to fp16"


def _check_bwd(tag, ref, gv, gv16, gl, ga):
    _check_gv(tag, ref, gv, gv16)
    _check(f"{tag} gattn", ga, ref.ga, C * U * ref.ga_abs)
    f = _far_fraction(ref.far)
    _check(f"{tag} gloc ({f:.1%} of the elements checked)", gl, ref.gl, C * U * ref.gl_abs, mask=ref.far)
    assert torch.isfinite(gl).all()


# ---------------------------------------------------------------------------------------------------------------------------
# generic one-thread-per-channel kernels: M * D / 4 not dividing 256, or a value pointer off 16-byte alignment

@pytest.mark.parametrize("M,D,skew", [(12, 16, 1), (12, 16, 0), (8, 32, 1), (4, 64, 3)])
def test_generic_kernels(M, D, skew):
    shapes = [(5, 7), (1, 9), (6, 1), (1, 1)]
    N, Lq, P = 3, 10, 3
    value, loc, attn, gout = _inputs(shapes, N, Lq, M, D, P, seed=M + D + skew)
    ref = _Ref(value, shapes, loc, attn, gout)
    out, _ = _fwd("fwd", value, shapes, loc, attn, M, D, P, skew=skew)
    _check_fwd(f"fwd M{M} D{D}", ref, out, None)
    gv, _, gl, ga = _bwd("bwd", value, shapes, loc, attn, gout, M, D, P, skew=skew)
    _check_bwd(f"bwd M{M} D{D}", ref, gv, None, gl, ga)


# ---------------------------------------------------------------------------------------------------------------------------
# channel-quad kernels with f32 / f16 value and output gradient, every output combination

_GEO = [  # shapes, N, Lq, M, D, P: M*D 64 (16 queries per workgroup, NQ = 21 not a multiple), 256 with 8 levels incl.
          # 1x1 / 1xW / Hx1, 1024 (one query per workgroup)
    ([(5, 7), (3, 3), (1, 4)], 3, 7, 4, 16, 4),
    ([(6, 5), (1, 1), (1, 9), (7, 1), (4, 4), (3, 8), (2, 2), (5, 3)], 3, 5, 8, 32, 2),
    ([(9, 11), (4, 5)], 3, 6, 16, 64, 4),
    ([(7, 6), (3, 2)], 3, 9, 2, 32, 3),
]


@pytest.mark.parametrize("v16,g16", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("which", ["f32", "f16", "both"])
def test_quad_kernels(v16, g16, which):
    k = (v16 * 2 + g16 + {"f32": 0, "f16": 1, "both": 2}[which]) % len(_GEO)
    shapes, N, Lq, M, D, P = _GEO[k]
    value, loc, attn, gout = _inputs(shapes, N, Lq, M, D, P, seed=10 + k + 7 * v16 + 3 * g16)
    vr, gr = _round_inputs(value, gout, v16, g16)
    ref = _Ref(vr, shapes, loc, attn, gr)
    outs = {"f32": ("out",), "f16": ("out16",), "both": ("out", "out16")}[which]
    out, out16 = _fwd("fwd_h", value, shapes, loc, attn, M, D, P, v16=bool(v16), outs=outs)
    tag = f"M{M} D{D} v16={v16} g16={g16}"
    _check_fwd(f"fwd_h {tag}", ref, out, out16)
    gvs = {"f32": ("gv",), "f16": ("gv16",), "both": ("gv", "gv16")}[which]
    gv, gv16, gl, ga = _bwd("bwd_h", value, shapes, loc, attn, gout, M, D, P, v16=bool(v16), g16=bool(g16), gvs=gvs)
    _check_bwd(f"bwd_h {tag}", ref, gv, gv16, gl, ga)


# ---------------------------------------------------------------------------------------------------------------------------
# fused forms (locations + soft-max inside the kernels) and the prep-kernel fallback

def _fused_inputs(shapes, N, Lq, M, D, P, nl_ref, bias, pad, seed, ref_pts=None):
    g = torch.Generator().manual_seed(seed)
    nL, T = len(shapes), len(shapes) * P
    S = sum(h * w for h, w in shapes)
    ld = 3 * M * T + pad
    value = torch.randn(N, S, M, D, generator=g)
    ow = torch.full((N * Lq, ld), float("nan"))          # padding columns NaN: the kernels must not read them
    ow[:, :2 * M * T] = _grid(torch.randn(N * Lq, 2 * M * T, generator=g) * 1.5, 2.0 ** -8)
    ow[:, 2 * M * T:3 * M * T] = torch.randn(N * Lq, M * T, generator=g)
    boff = _grid(torch.randn(M * T * 2, generator=g), 2.0 ** -8) if bias else None
    baw = (torch.randn(M * T, generator=g) * 0.5) if bias else None
    ref = ref_pts if ref_pts is not None else _grid(torch.rand(Lq, nl_ref, 2, generator=g))
    gout = torch.randn(N, Lq, M * D, generator=g)
    return value, ow, ld, boff, baw, ref, gout


class _FusedRef:
    def __init__(self, value, shapes, ow, ld, boff, baw, ref, nl_ref, M, P, gout):
        N = value.shape[0]
        nL, T = len(shapes), len(shapes) * P
        owd = ow.double().clone()
        owd[:, 3 * M * T:] = 0
        owd.requires_grad_(True)
        v = value.double().requires_grad_(True)
        dbl = lambda t: None if t is None else t.double()
        loc, attn, out = R.msda_fused_fp64(v, shapes, owd, ld, dbl(boff), dbl(baw), ref.double(), nl_ref, M, P)
        out.backward(gout.double().reshape(out.shape))
        self.loc, self.attn, self.out, self.dow, self.gv = loc.detach(), attn.detach(), out.detach(), owd.grad, v.grad
        self.out_abs, ga_abs, self.gv_abs = R.abs_scales(value, shapes, self.loc, self.attn, gout)
        sz = R.level_sizes(shapes).reshape(1, 1, 1, nL, 1, 2)
        goff_abs = R.loc_grad_abs(value, shapes, self.loc, self.attn, gout) / sz
        glog_abs = self.attn * (ga_abs + (self.attn * ga_abs).sum((-1, -2), keepdim=True))
        self.dow_abs = torch.cat([goff_abs.reshape(ow.shape[0], -1), glog_abs.reshape(ow.shape[0], -1),
                                  torch.zeros(ow.shape[0], ld - 3 * M * T, dtype=F64)], 1)
        far = R.kink_distance(shapes, self.loc) > 1e-3
        self.far = torch.cat([far.reshape(ow.shape[0], -1), torch.ones(ow.shape[0], ld - 2 * M * T, dtype=torch.bool)], 1)
        self.far_frac = far.float().mean().item()
        self.pairs = R.pair_counts(shapes, self.loc, value.shape[1])[..., None]
        self.q = gout.abs().max().item() * U              # soft-max weights: max|attn| <= 1
        # loc = ref + (off + b) / size: sum |terms|; attention logits z = logit + b (their magnitude scales the error of exp)
        o = ow.double()[:, :2 * M * T].reshape(self.loc.shape).abs() + (0 if boff is None else boff.double().abs().reshape(M, nL, P, 2))
        self.loc_abs = ref.double().abs().reshape(1, -1, 1, nl_ref, 1, 2) + o / sz
        z = ow.double()[:, 2 * M * T:3 * M * T].reshape(N, -1, M, T) + (0 if baw is None else baw.double().reshape(M, T))
        self.zmax = z.abs().amax(-1, keepdim=True).reshape(N, -1, M, 1, 1)


def _check_fused_fwd(tag, fr, loc, attn, out, out16):
    _check(f"{tag} loc", loc, fr.loc, 2.0 ** -22 * fr.loc_abs)
    # soft-max weights: 2^-22 relative per unit of the logits' magnitude (the exponent's argument carries U |z|)
    _check(f"{tag} attn", attn, fr.attn, 2.0 ** -22 * fr.attn * (1 + fr.zmax))
    b = C * U * fr.out_abs
    if out is not None:
        _check(f"{tag} out", out, fr.out, b)
    if out16 is not None:
        _check(f"{tag} out16", out16, fr.out, b + _ulp16(fr.out))


def _check_fused_bwd(tag, fr, gv, gv16, dow16, dow32=None):
    b = (fr.pairs / 2 + 1) * fr.q + C * U * fr.gv_abs
    if gv is not None:
        _check(f"{tag} gvalue", gv, fr.gv, b)
    if gv16 is not None:
        _check(f"{tag} gvalue16", gv16, fr.gv, b + _ulp16(fr.gv))
    if gv is not None and gv16 is not None:
        assert torch.equal(gv16, gv.half())
    assert fr.far_frac >= 0.9, f"only {fr.far_frac:.1%} of the offset gradients away from a kink"
    db = C * U * fr.dow_abs
    tag = f"{tag} ({fr.far_frac:.1%} of the offset gradients checked)"
    if dow32 is not None:
        _check(f"{tag} dow32", dow32, fr.dow, db, mask=fr.far)
    _check(f"{tag} dow16", dow16, fr.dow, db + _ulp16(fr.dow), mask=fr.far)


def _run_fused(value, shapes, ow, ld, boff, baw, ref, nl_ref, gout, M, D, P, v16, g16, outs, gvs, via_prep=False):
    L = _L()
    lib = L.lib()
    N, S = value.shape[:2]
    nL, T = len(shapes), len(shapes) * P
    Lq = ow.shape[0] // N
    val = _dev(value, F16 if v16 else F32)
    owd, refd = _dev(ow, F32), _dev(ref, F32)
    bo = None if boff is None else _dev(boff, F32)
    ba = None if baw is None else _dev(baw, F32)
    loc, attn = _nan(N * Lq * M * T * 2, F32), _nan(N * Lq * M * T, F32)
    out = _nan(N * Lq * M * D, F32) if "out" in outs else None
    out16 = _nan(N * Lq * M * D, F16) if "out16" in outs else None
    hs = _hs(shapes)
    if via_prep:
        lib.wc_msda_prep_fwd(_ptr(owd), _ptr(bo), _ptr(ba), _ptr(refd), _ptr(loc), _ptr(attn), hs, nL, N, Lq, M, P, ld, nl_ref,
                             L.stream())
        lib.wc_msda_fwd_h(_ptr(val), int(v16), hs, nL, _ptr(loc), _ptr(attn), _ptr(out), _ptr(out16), N, Lq, M, D, P, L.stream())
    else:
        lib.wc_msda_fwd_f(_ptr(val), int(v16), hs, nL, _ptr(owd), ld, _ptr(bo), _ptr(ba), _ptr(refd), nl_ref, _ptr(loc),
                          _ptr(attn), _ptr(out), _ptr(out16), N, Lq, M, D, P, L.stream())
    go = _dev(gout, F16 if g16 else F32)
    gv = _nan(N * S * M * D, F32) if "gv" in gvs else None
    gv16 = _nan(N * S * M * D, F16) if "gv16" in gvs else None
    dow16 = _nan(N * Lq * ld, F16)
    dow32 = None
    ws, gmax = _ws(N, M, S, nL, Lq, P)
    if via_prep:
        gl, ga = _nan(loc.numel(), F32), _nan(attn.numel(), F32)
        dow32 = _nan(N * Lq * ld, F32)
        lib.wc_msda_bwd_h(_ptr(val), int(v16), hs, nL, _ptr(loc), _ptr(attn), _ptr(go), int(g16), _ptr(gv), _ptr(gv16), _ptr(gl),
                          _ptr(ga), _ptr(gmax), _ptr(ws), N, Lq, M, D, P, L.stream())
        lib.wc_msda_prep_bwd(_ptr(gl), _ptr(ga), _ptr(attn), _ptr(dow32), _ptr(dow16), hs, nL, N, Lq, M, P, ld, L.stream())
    else:
        lib.wc_msda_bwd_f(_ptr(val), int(v16), hs, nL, _ptr(loc), _ptr(attn), _ptr(go), int(g16), _ptr(gv), _ptr(gv16),
                          _ptr(dow16), ld, _ptr(gmax), _ptr(ws), N, Lq, M, D, P, L.stream())
    torch.cuda.synchronize()
    return loc, attn, out, out16, gv, gv16, dow16, dow32


_FUSED = [  # nL, nl_ref, bias, pad, v16, g16, M, D, outs, gvs
    (3, 3, True, 0, 1, 1, 8, 32, ("out16",), ("gv16",)),
    (3, 1, False, 8, 0, 0, 4, 16, ("out",), ("gv",)),
    (1, 1, True, 8, 1, 0, 16, 64, ("out", "out16"), ("gv", "gv16")),
    (1, 1, False, 0, 0, 1, 2, 32, ("out",), ("gv16",)),
    (3, 1, True, 8, 0, 1, 4, 64, ("out", "out16"), ("gv",)),
    (3, 3, False, 0, 1, 0, 16, 16, ("out16",), ("gv", "gv16")),
]


@pytest.mark.parametrize("cfg", _FUSED, ids=lambda c: "nL{}-ref{}-bias{}-pad{}-v{}-g{}-M{}D{}".format(*c[:8]))
def test_fused_kernels(cfg):
    nL, nl_ref, bias, pad, v16, g16, M, D, outs, gvs = cfg
    shapes = [(8, 16), (4, 2), (1, 4)] if nL == 3 else [(16, 8)]
    N, Lq, P = 3, 7, 4
    value, ow, ld, boff, baw, ref, gout = _fused_inputs(shapes, N, Lq, M, D, P, nl_ref, bias, pad, seed=sum(cfg[:8]))
    vr, gr = _round_inputs(value, gout, v16, g16)
    fr = _FusedRef(vr, shapes, ow, ld, boff, baw, ref, nl_ref, M, P, gr)
    loc, attn, out, out16, gv, gv16, dow16, _ = _run_fused(value, shapes, ow, ld, boff, baw, ref, nl_ref, gout, M, D, P, v16, g16,
                                                           outs, gvs)
    tag = "fused " + "nL{}-ref{}-bias{}-pad{}-v{}-g{}-M{}D{}".format(*cfg[:8])
    _check_fused_fwd(tag, fr, loc, attn, out, out16)
    _check_fused_bwd(tag, fr, gv, gv16, dow16)
    if pad:
        assert (dow16.reshape(-1, ld)[:, 3 * M * nL * P:] == 0).all(), f"{tag}: padding columns of dow16 not zeroed"


@pytest.mark.parametrize("shapes,P,nl_ref", [([(8, 16), (4, 2), (1, 4)], 4, 1), ([(4, 8), (2, 2)], 3, 2)])
def test_prep_kernels_with_fwd_h_and_bwd_h(shapes, P, nl_ref):
    """The engine's fallback when the fused form is unsupported: prep_fwd + fwd_h, bwd_h + prep_bwd (dow as f32 and f16)."""
    N, Lq, M, D = 3, 6, 8, 32
    nL = len(shapes)
    lib = _L().lib()
    assert lib.cdll.wc_msda_fused_supported(nL, M, D, P) == (1 if (nL, P) == (3, 4) else 0)
    value, ow, ld, boff, baw, ref, gout = _fused_inputs(shapes, N, Lq, M, D, P, nl_ref, True, 8, seed=40 + P)
    fr = _FusedRef(value.half().float(), shapes, ow, ld, boff, baw, ref, nl_ref, M, P, gout.half().float())
    loc, attn, out, out16, gv, gv16, dow16, dow32 = _run_fused(value, shapes, ow, ld, boff, baw, ref, nl_ref, gout, M, D, P, 1, 1,
                                                               ("out16",), ("gv16",), via_prep=True)
    tag = f"prep nL{nL} P{P}"
    _check_fused_fwd(tag, fr, loc, attn, out, out16)
    _check_fused_bwd(tag, fr, gv, gv16, dow16, dow32)
    assert (dow32.reshape(-1, ld)[:, 3 * M * nL * P:] == 0).all() and (dow16.reshape(-1, ld)[:, 3 * M * nL * P:] == 0).all()


def test_fused_supported_agrees_with_the_fused_calls():
    L = _L()
    lib = L.lib()
    for nL in (1, 2, 3, 4):
        for P in (2, 4):
            for M, D in ((8, 32), (12, 16), (4, 16), (32, 32)):
                sup = lib.cdll.wc_msda_fused_supported(nL, M, D, P)
                expect = P == 4 and nL in (1, 3) and 256 % (M * D // 4) == 0
                assert bool(sup) == expect, (nL, M, D, P)
                shapes = [(4, 2)] * nL
                N, Lq = 1, 3
                value, ow, ld, boff, baw, ref, gout = _fused_inputs(shapes, N, Lq, M, D, P, 1, False, 0, seed=1)
                call = lambda: _run_fused(value, shapes, ow, ld, boff, baw, ref, 1, gout, M, D, P, 0, 0, ("out",), ("gv",))
                if sup:
                    loc, attn, out, *_ = call()
                    assert torch.isfinite(out).all()
                else:
                    with pytest.raises(RuntimeError, match="wc_msda_fwd_f"):
                        call()


# ---------------------------------------------------------------------------------------------------------------------------
# level sizes, bucket density, fixed-point range

def test_level_of_16384_pixels_and_the_limit():
    shapes = [(128, 128), (3, 5)]
    N, Lq, M, D, P = 1, 24, 4, 16, 3
    value, loc, attn, gout = _inputs(shapes, N, Lq, M, D, P, seed=3)
    ref = _Ref(value, shapes, loc, attn, gout)
    gv, _, gl, ga = _bwd("bwd", value, shapes, loc, attn, gout, M, D, P)
    _check_bwd("128x128", ref, gv, None, gl, ga)
    # one pixel more: refused before anything is launched (every output and workspace keeps its NaN / 0xFF bytes)
    L = _L()
    big = [(129, 128)]
    S = 129 * 128
    value = torch.randn(N, S, M, D)
    P = 4                                          # (a fused configuration: wc_msda_bwd_f must get as far as the level check)
    loc, attn = torch.rand(N, Lq, M, 1, P, 2), torch.full((N, Lq, M, 1, P), 0.25)
    gout = torch.randn(N, Lq, M * D)
    val, go = _dev(value, F32), _dev(gout, F32)
    gv, gl, ga = _nan(value.numel(), F32), _nan(loc.numel(), F32), _nan(attn.numel(), F32)
    dow16 = _nan(N * Lq * 3 * M * P, F16)
    ws, gmax = _ws(N, M, S, 1, Lq, P)
    locd, attnd = _dev(loc, F32), _dev(attn, F32)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="16384"):
        L.lib().wc_msda_bwd(_ptr(val), _hs(big), 1, _ptr(locd), _ptr(attnd), _ptr(go), _ptr(gv), _ptr(gl),
                            _ptr(ga), _ptr(gmax), _ptr(ws), N, Lq, M, D, P, L.stream())
    with pytest.raises(RuntimeError, match="16384"):
        L.lib().wc_msda_bwd_f(_ptr(val), 0, _hs(big), 1, _ptr(locd), _ptr(attnd), _ptr(go), 0, _ptr(gv), None,
                              _ptr(dow16), 3 * M * P, _ptr(gmax), _ptr(ws), N, Lq, M, D, P, L.stream())
    torch.cuda.synchronize()
    for name, t in (("gvalue", gv), ("gloc", gl), ("gattn", ga), ("dow16", dow16), ("gmax", gmax), ("ws", ws)):
        assert (t.view(torch.uint8) == 255).all(), f"{name} was written by a call that was refused"


# eight levels whose mean bucket lengths (Lq * P * 4 / pixels = 1024 / HW) select every GatherPlan.gl from CL to D
_DENSITY = [(32, 32), (16, 16), (12, 12), (8, 8), (6, 6), (4, 4), (2, 2), (1, 1)]


@pytest.mark.parametrize("D,g16", [(64, 0), (16, 1), (32, 1)])
def test_bucket_density_from_empty_to_crowded(D, g16):
    N, Lq, M, P = 2, 64, 4, 4
    shapes = _DENSITY
    value, loc, attn, gout = _inputs(shapes, N, Lq, M, D, P, seed=D + g16, edges=False)
    # image 0: the samples of every level crowd into a 3 x 3 pixel corner (buckets of hundreds of entries: many GL rounds,
    # every other pixel empty); image 1: spread over the map
    sz = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32).view(1, 1, len(shapes), 1, 2)
    loc[0] = _grid((torch.rand(Lq, M, len(shapes), P, 2) * 2.5 + 0.5) / sz)
    _, gr = _round_inputs(value, gout, 0, g16)
    ref = _Ref(value, shapes, loc, attn, gr)
    gv, gv16, gl, ga = _bwd("bwd_h", value, shapes, loc, attn, gout, M, D, P, g16=bool(g16), gvs=("gv", "gv16"))
    _check_bwd(f"density D{D} g16={g16}", ref, gv, gv16, gl, ga)
    empty = (ref.pairs.expand_as(ref.gv) == 0)
    assert empty.float().mean() > 0.3 and (ref.pairs > 100).any()
    assert (gv.cpu().reshape(ref.gv.shape)[empty] == 0).all(), "a pixel without samples has a non-zero value gradient"


def test_all_zero_output_gradient():
    shapes = [(6, 5), (3, 3)]
    N, Lq, M, D, P = 2, 9, 8, 32, 4
    value, loc, attn, gout = _inputs(shapes, N, Lq, M, D, P, seed=4)
    gout.zero_()
    for kind, g16 in (("bwd", False), ("bwd_h", True)):
        gv, gv16, gl, ga = _bwd(kind, value, shapes, loc, attn, gout, M, D, P, g16=g16,
                                gvs=("gv",) if kind == "bwd" else ("gv", "gv16"))
        assert (gv == 0).all() and (gl == 0).all() and (ga == 0).all(), kind
        assert gv16 is None or (gv16 == 0).all()


def test_fixed_point_range_large_attention_weights():
    """|attn| up to 50 (the public wc_msda_bwd / _MSDAFunction accept any weights), samples at pixel centres (bilinear weight 1),
    D = 64 with fp32 gout (16 products per lane and round of the gather), crowded buckets."""
    shapes = [(8, 8), (4, 4)]
    N, Lq, M, D, P = 2, 48, 4, 64, 4
    value, _, _, gout = _inputs(shapes, N, Lq, M, D, P, seed=6, edges=False)
    g = torch.Generator().manual_seed(7)
    nL = len(shapes)
    loc = torch.empty(N, Lq, M, nL, P, 2)
    for l, (H, W) in enumerate(shapes):           # every sample of a level on the centre of pixel (1, 2) or (2, 1)
        c = torch.randint(0, 2, (N, Lq, M, P), generator=g).float()
        loc[..., l, :, 0], loc[..., l, :, 1] = (1 + c + 0.5) / W, (2 - c + 0.5) / H
    attn = torch.rand(N, Lq, M, nL, P, generator=g) * 30 + 20
    attn[1] = -attn[1]
    attn[0, 0, 0, 0, 0] = 50.0
    gout = gout.abs() * 0.5 + 0.5 * gout.abs().max()         # products of one sign: the int32 rounds see their full range
    ref = _Ref(value, shapes, loc, attn, gout)
    assert ref.pairs.max() >= 16
    gv, _, gl, ga = _bwd("bwd", value, shapes, loc, attn, gout, M, D, P)
    _check_gv("attn-range", ref, gv, None)
    _check("attn-range gattn", ga, ref.ga, C * U * ref.ga_abs)


def test_fixed_point_quantum_with_an_outlier_gradient():
    """One output-gradient element 1e4 times the rest: the quantum max|gout| 2^-24 then dominates the small value gradients;
    the documented bound (pairs / 2 + 1) q must still hold, and the fp32 accumulation must not overflow."""
    shapes = [(6, 6), (3, 3)]
    N, Lq, M, D, P = 2, 40, 4, 32, 4
    value, loc, attn, gout = _inputs(shapes, N, Lq, M, D, P, seed=8)
    gout[1, 3, 5] = 1e4 * gout.abs().max()
    ref = _Ref(value, shapes, loc, attn, gout)
    for g16, kind in ((False, "bwd"), (False, "bwd_h")):
        gv, _, gl, ga = _bwd(kind, value, shapes, loc, attn, gout, M, D, P, g16=g16)
        _check_gv(f"outlier {kind}", ref, gv, None)
    go16 = gout.clone()
    go16[1, 3, 5] = 6e4                                   # within fp16 range
    _, gr = _round_inputs(value, go16, 0, True)
    ref16 = _Ref(value, shapes, loc, attn, gr)
    gv, _, _, _ = _bwd("bwd_h", value, shapes, loc, attn, go16, M, D, P, g16=True)
    _check_gv("outlier f16 gout", ref16, gv, None)


# ---------------------------------------------------------------------------------------------------------------------------
# the CTI geometry of the benchmark: one image, 64^2 / 32^2 / 16^2 pyramid, 32^2 tokens, M = 8, D = 32, P = 4 (engine form)

def test_cti_geometry_fused_engine_form():
    shapes = [(64, 64), (32, 32), (16, 16)]
    N, Lq, M, D, P = 1, 1024, 8, 32, 4
    ys, xs = torch.meshgrid((torch.arange(32) + 0.5) / 32, (torch.arange(32) + 0.5) / 32, indexing="ij")
    ref_pts = torch.stack([xs.reshape(-1), ys.reshape(-1)], -1).view(Lq, 1, 2)
    value, ow, ld, boff, baw, ref, gout = _fused_inputs(shapes, N, Lq, M, D, P, 1, True, 0, seed=11, ref_pts=ref_pts)
    gout = gout * 1e-2
    fr = _FusedRef(value.half().float(), shapes, ow, ld, boff, baw, ref, 1, M, P, gout.half().float())
    loc, attn, out, out16, gv, gv16, dow16, _ = _run_fused(value, shapes, ow, ld, boff, baw, ref, 1, gout, M, D, P, 1, 1,
                                                           ("out16",), ("gv16",))
    _check_fused_fwd("CTI", fr, loc, attn, out, out16)
    _check_fused_bwd("CTI", fr, gv, gv16, dow16)


# ---------------------------------------------------------------------------------------------------------------------------
# the value gradient is bit-identical to the outputs of the kernels before the fixed-point scale took max|attn| into account
# (softmax weights: max|attn| <= 1, so nothing may change; tests/golden/msda_gvalue.npz holds the inputs and the outputs that
# the previous kernels produced for them on an MI355X)

def test_value_gradient_bits_unchanged_for_softmax_weights(golden):
    z = golden("msda_gvalue.npz")
    for tag in ("f32", "f16"):
        shapes = [tuple(s) for s in z[f"{tag}_shapes"].tolist()]
        M, D, P = [int(v) for v in z[f"{tag}_mdp"]]
        g16 = tag == "f16"
        value, loc, attn, gout = [torch.from_numpy(z[f"{tag}_{k}"]) for k in ("value", "loc", "attn", "gout")]
        gv, gv16, _, _ = _bwd("bwd_h", value, shapes, loc, attn, gout, M, D, P, v16=g16, g16=g16, gvs=("gv", "gv16"))
        assert np.array_equal(gv.cpu().numpy().view(np.uint32), z[f"{tag}_gvalue"].reshape(-1).view(np.uint32)), tag
        assert np.array_equal(gv16.cpu().numpy().view(np.uint16), z[f"{tag}_gvalue16"].reshape(-1).view(np.uint16)), tag
