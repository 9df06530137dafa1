"""Every kernel path of csrc/par.hip against the fp64 reference of tests/par_ref.py, through the C ABI.

Every output and workspace is filled with NaN (0xFF bytes) before a call and carries a 256-float sentinel tail: `out` and `tmp`
behind their B C H W floats, `aff_ws` behind exactly its documented size.  After the call every output element is finite, every
sentinel untouched, the inputs bit-unchanged, and each element inside the error-model bound derived in tests/par_ref.py.  The
kernel timers name the instantiation that ran.  Constant-colour images (every weight 1/T + pi_t) show a wrong neighbour at full
strength; sparse probe masks make an output the sum of one or two weights, so that one misplaced 16-bit weight fails."""
import functools

import pytest
import torch

from tests import par_ref as R

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
TAIL = 256
DIL6 = R.DIL6
C_ALL, C_FEW = tuple(range(1, 10)), (1, 3, 4, 7)


def _L():
    from weclip_vit_comer_amd import _lib as L
    return L


def _nan(n):
    t = torch.empty(n + TAIL, dtype=F32, device="cuda")
    t.view(torch.uint8).fill_(255)
    return t


def _dev(x):
    return x.contiguous().cuda()


def _p(t):
    return _L().ptr(t)


def _tail_ok(name, t, n):
    assert t.numel() == n + TAIL
    bad = int((t[n:].view(I32) != -1).sum())
    assert bad == 0, f"{name}: {bad} floats written behind its {n} floats"


def _finite(name, t):
    n = int((~torch.isfinite(t)).sum())
    assert n == 0, f"{name}: {n} elements not written (still NaN)"


WORST = {}          # kernel instantiation -> worst err / bound seen


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """Prints the worst err / bound per instantiation after the module (visible with -s)."""
    yield
    for k in sorted(WORST):
        print(f"WORST {k}: {WORST[k]:.3g}")


def _check(path, what, got, ref, bound):
    got = got.detach().double().cpu().reshape(ref.shape)
    _finite(f"{path} {what}", got)
    err = (got - ref).abs()
    bound = bound.expand_as(err)
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    if (err > bound).any():
        i = int(torch.argmax((err - bound).reshape(-1)))
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ref.shape))
        raise AssertionError(f"{path} {what}: {int((err > bound).sum())} of {err.numel()} elements outside the bound, worst "
                             f"err / bound {ratio:.3g}; at {idx}: got {got.reshape(-1)[i]:.9g} ref {ref.reshape(-1)[i]:.9g}")
    WORST[path] = max(WORST.get(path, 0.0), ratio)


def _timed(fn):
    """Run fn with the kernel timers on; -> names of the kernels it launched."""
    from weclip_vit_comer_amd import ops
    ops.KernelTimer.enable(1)
    try:
        fn()
        names = set(ops.KernelTimer.summary())
    finally:
        ops.KernelTimer.enable(0)
    torch.cuda.synchronize()
    return names


# ---------------------------------------------------------------------------------------------------------------------
# names and workspace sizes, mirrored from par_iter_name / launch_affinity / the header

def aff_name(n_dil, tiled=False, h16=False):
    if n_dil != 6:
        return "par_affinity_kernel"
    return f"par_affinity_reg_kernel<6, {'true, true' if h16 else ('true' if tiled else 'false')}>"


def iter_name(C, tiled=False, h16=False):
    cg = 2 if C <= 2 else (3 if C == 3 else 4)
    return f"par_iter_kernel<{cg}, true, true, 8, 12>" if h16 else f"par_iter_kernel<{cg}, {'true' if tiled else 'false'}>"


def ws_floats(B, group, T, H, W, h16):
    """aff_ws as documented: min(group, B) T H ceil64(W) floats, or (T / 2 + 1) dwords per pixel for the 16-bit form."""
    return min(group, B) * (T // 2 + 1 if h16 else T) * H * ((W + 63) // 64 * 64)


# ---------------------------------------------------------------------------------------------------------------------
# launches

def gpu_affinity(imgd, dil):
    B, _, H, W = imgd.shape
    n = B * 8 * len(dil) * H * W
    aff = _nan(n)
    keep = imgd.clone()
    names = _timed(lambda: _L().lib().wc_par_affinity(_p(imgd), _p(aff), B, H, W, _L().int_array(dil), len(dil), _L().stream()))
    _tail_ok("aff", aff, n)
    assert torch.equal(imgd, keep), "wc_par_affinity changed the image"
    return aff[:n].view(B, 8 * len(dil), H, W), names


def gpu_iterate(affd, md, dil):
    B, C, H, W = md.shape
    n = md.numel()
    out = _nan(n)
    keep, keep_a = md.clone(), affd.clone()
    names = _timed(lambda: _L().lib().wc_par_iterate(_p(affd), _p(md), _p(out), B, C, H, W, _L().int_array(dil), len(dil),
                                                     _L().stream()))
    _tail_ok("masks_out", out, n)
    assert torch.equal(md.view(I32), keep.view(I32)) and torch.equal(affd.view(I32), keep_a.view(I32)), "inputs changed"
    _finite("masks_out", out[:n])
    return out[:n].view(B, C, H, W), names


def gpu_forward(imgd, md, dil, n_iter, group, h16):
    B, C, H, W = md.shape
    n = md.numel()
    ws = ws_floats(B, group, 8 * len(dil), H, W, h16)
    out, tmp, aff = _nan(n), _nan(n), _nan(ws)
    keep, keep_i = md.clone(), imgd.clone()
    fn = _L().lib().wc_par_forward_h if h16 else _L().lib().wc_par_forward
    names = _timed(lambda: fn(_p(imgd), _p(md), _p(out), _p(tmp), _p(aff), B, C, H, W, _L().int_array(dil), len(dil), n_iter,
                              group, _L().stream()))
    _tail_ok("out", out, n)
    _tail_ok("tmp", tmp, n)
    _tail_ok("aff_ws", aff, ws)
    assert torch.equal(md.view(I32), keep.view(I32)) and torch.equal(imgd.view(I32), keep_i.view(I32)), "inputs changed"
    _finite("out", out[:n])
    if n_iter > 1:
        _finite("tmp", tmp[:n])
    return out[:n].view(B, C, H, W), names


# ---------------------------------------------------------------------------------------------------------------------
# references, computed once per (image kind, shape, dilations) and shared

class Ref:
    """img (B, 3, H, W) fp32 and, in the layout (T, B, 1, H, W) that broadcasts against masks (B, C, H, W): aff, e, the fp32
    affinity bound ab; amax (B, 1, H, W)."""

    def __init__(self, kind, B, H, W, dil, seed):
        self.img = R.images(kind, B, H, W, seed=seed)
        per = [R.affinity(self.img[b], dil) for b in range(B)]
        self.aff = torch.stack([p[0] for p in per], 1).unsqueeze(2)
        self.e = torch.stack([p[3] for p in per], 1).unsqueeze(2)
        self.amax = torch.stack([p[1] for p in per], 0).unsqueeze(1)
        self.ab = R.aff_bound(self.aff, self.e, dil)
        self.dil = tuple(dil)


@functools.lru_cache(maxsize=None)
def ref(kind, B, H, W, dil, seed=1):
    return Ref(kind, B, H, W, dil, seed)


def other_kind(H, W):
    """The second image kind of a shape (beside const): cycles through the four structured kinds."""
    return R.KINDS[1 + R.SHAPES.index((H, W)) % 4]


def c_list(H, W):
    return C_ALL if (H, W) == (9, 65) else C_FEW


# ---------------------------------------------------------------------------------------------------------------------
# affinity: <6, false> and the generic kernel

@pytest.mark.parametrize("H,W", R.SHAPES)
@pytest.mark.parametrize("dil", R.AFF_DILS, ids=str)
def test_affinity(dil, H, W):
    B = 2
    for kind in (R.KINDS if (H, W) == (40, 72) else ("const", "piecewise")):
        r = ref(kind, B, H, W, dil)
        aff, names = gpu_affinity(_dev(r.img), dil)
        assert names == {aff_name(len(dil))}, names
        _check(aff_name(len(dil)), f"{kind} {H}x{W} {dil}", aff.permute(1, 0, 2, 3).unsqueeze(2), r.aff, r.ab)


# ---------------------------------------------------------------------------------------------------------------------
# plane-major sweep on test-supplied weights: par_iter_kernel<CG, false>, T = 48 and other tap counts

@pytest.mark.parametrize("H,W", R.SHAPES)
@pytest.mark.parametrize("dil", [DIL6, (3,), (2, 5), (1, 2, 3, 4, 6, 8, 12, 24)], ids=str)
def test_plane_major_sweep(dil, H, W):
    B, T = 3, 8 * len(dil)
    g = torch.Generator().manual_seed(H * 131 + W + T)
    w = torch.randn(B, T, H, W, generator=g) * 0.1
    w[torch.rand(B, T, H, W, generator=g) < 0.1] = 0.0
    w64 = w.double().permute(1, 0, 2, 3).unsqueeze(2)
    wd = _dev(w)
    for C in c_list(H, W):
        m = R.masks("dense", B, C, H, W, seed=T) - (0.25 if C % 2 else 0.0)           # negative mask values too
        out, names = gpu_iterate(wd, _dev(m), dil)
        assert names == {iter_name(C)}, names
        want, s_am, _, _ = R.sweep_terms(w64, m, dil)
        _check(iter_name(C), f"C={C} {H}x{W} T={T}", out, want, R.acc_bound(s_am, T))


# ---------------------------------------------------------------------------------------------------------------------
# tiled fp32 path: wc_par_forward, one sweep

@pytest.mark.parametrize("H,W", R.SHAPES)
def test_tiled_fp32_forward(H, W):
    B = 2
    for kind in ("const", other_kind(H, W)):
        r = ref(kind, B, H, W, DIL6)
        imgd = _dev(r.img)
        affd, _ = gpu_affinity(imgd, DIL6)
        for C in c_list(H, W):
            m = R.masks("dense", B, C, H, W, seed=2)
            md = _dev(m)
            out, names = gpu_forward(imgd, md, DIL6, 1, B, False)
            assert names == {aff_name(6, tiled=True), iter_name(C, tiled=True)}, names
            want, s_am, _, s_b = R.sweep_terms(r.aff, m, DIL6, r.ab)
            _check(iter_name(C, tiled=True), f"{kind} C={C} {H}x{W}", out, want, R.acc_bound(s_am, 48) + s_b)
            # the same arithmetic in the plane-major layout: only the addressing differs
            two, _ = gpu_iterate(affd, md, DIL6)
            assert torch.equal(out, two), f"{kind} C={C}: tiled forward != wc_par_affinity + wc_par_iterate"


# ---------------------------------------------------------------------------------------------------------------------
# H16 path: wc_par_forward_h, one sweep; dilation sets that move the tile / gather boundary

@pytest.mark.parametrize("H,W", R.SHAPES)
@pytest.mark.parametrize("dil", R.H16_DILS, ids=str)
def test_h16_forward(dil, H, W):
    B = 2
    for kind in ("const", other_kind(H, W)):
        r = ref(kind, B, H, W, dil)
        imgd = _dev(r.img)
        for C in c_list(H, W):
            for mk in ("dense", "ones", "probes"):
                m = R.masks(mk, B, C, H, W, seed=3)
                out, names = gpu_forward(imgd, _dev(m), dil, 1, B, True)
                assert names == {aff_name(6, h16=True), iter_name(C, h16=True)}, names
                tag = f"{kind} {mk} C={C} {H}x{W} {dil}"
                if mk == "ones":
                    _check(iter_name(C, h16=True), tag, out, r.aff.sum(0).expand(B, C, H, W),
                           R.h16_ones_bound(r.aff, r.amax, r.e, dil))
                    continue
                want = R.sweep_terms(r.aff, m, dil)[0]
                _check(iter_name(C, h16=True), tag, out, want, R.h16_bound(r.aff, r.amax, r.e, m, dil))
                if mk == "dense":
                    _check(iter_name(C, h16=True) + " (Abel bound)", tag, out, want,
                           R.h16_bound(r.aff, r.amax, r.e, m, dil, abel=True))


# ---------------------------------------------------------------------------------------------------------------------
# ping-pong and grouping, both forward entry points

@pytest.mark.parametrize("B,group", [(5, 2), (3, 3), (2, 7), (4, 1)])
@pytest.mark.parametrize("n_iter", [1, 2, 3])
@pytest.mark.parametrize("h16,dil", [(False, DIL6), (True, DIL6), (False, (2, 5))], ids=["fp32", "h16", "fp32-16taps"])
def test_ping_pong_and_grouping(h16, dil, n_iter, B, group):
    C, H, W = 5, 25, 70
    r = ref("synth", B, H, W, dil, seed=2)
    m = R.masks("dense", B, C, H, W, seed=4)
    imgd, md = _dev(r.img), _dev(m)
    out, names = gpu_forward(imgd, md, dil, n_iter, group, h16)
    tiled = len(dil) == 6
    assert names == {aff_name(len(dil), tiled, h16), iter_name(C, tiled, h16)}, names
    whole, _ = gpu_forward(imgd, md, dil, n_iter, B, h16)
    assert torch.equal(out, whole), f"group = {group} differs from group = {B}"
    for b in range(B):
        one, _ = gpu_forward(imgd[b:b + 1].contiguous(), md[b:b + 1].contiguous(), dil, n_iter, 1, h16)
        assert torch.equal(out[b:b + 1], one), f"image {b} of {B} (group {group}) differs from its own B = 1 call"
    wb = r.ab + (R.h16_weight_bound(r.amax) if h16 else 0.0)
    want = m.double()
    for _ in range(n_iter):
        want = R.sweep_terms(r.aff, want, dil)[0]
    _check(iter_name(C, tiled, h16), f"{n_iter} sweeps B={B} group={group}", out, want,
           R.forward_bound(r.aff, m, dil, n_iter, wb))


# ---------------------------------------------------------------------------------------------------------------------
# labels

def gpu_labels(m, keys, nch):
    B, C, H, W = m.shape
    n = B * H * W
    lab = torch.full((n + TAIL,), -7, dtype=I64, device="cuda")
    md, kd = _dev(m), _dev(keys)
    nd = None if nch is None else _dev(nch.to(I32))
    _L().lib().wc_par_labels(_p(md), _p(kd), _p(nd), _p(lab), B, C, H, W, _L().stream())
    torch.cuda.synchronize()
    assert (lab[n:] == -7).all(), "labels written behind B H W"
    assert torch.equal(md.cpu().view(I32), m.view(I32))
    return lab[:n].view(B, H, W).cpu()


@pytest.mark.parametrize("H,W", [(1, 1), (1, 257), (40, 70)])
@pytest.mark.parametrize("C", [1, 2, 5])
def test_labels(C, H, W):
    B = 3
    g = torch.Generator().manual_seed(C * 1000 + W)
    m = torch.randint(0, 4, (B, C, H, W), generator=g).float() * 0.25                  # few levels: exact ties everywhere
    if C > 1:
        m[0, C - 1] = m[0, 0].clone()                                                    # channel 0 ties with the last one
        m[0, 0, :, ::2] = 2.0
        m[0, C - 1, :, ::2] = 2.0
        m[1, C - 1] = 9.0                                                                # padded: larger than every live one
    keys = torch.arange(B * C, dtype=I64).view(B, C) * 3 + 1
    for nch in (None, torch.tensor([C, max(C - 1, 1), 1])):
        want = R.labels(m, keys, nch)
        got = gpu_labels(m, keys, nch)
        assert torch.equal(got, want), f"nch={nch}: {int((got != want).sum())} of {want.numel()} labels differ"
        if nch is not None:
            assert (got[2] == keys[2, 0]).all()                                          # nch = 1: channel 0 always
            if C > 1:
                assert not (got[1] == keys[1, C - 1]).any()                              # the padded channel never wins
    if C > 1:
        assert (gpu_labels(m, keys, None)[0, :, ::2] == keys[0, 0]).all()                # the first maximum wins the tie


# ---------------------------------------------------------------------------------------------------------------------

def test_every_par_instantiation_runs():
    """One small launch per instantiation, names from the kernel timers."""
    B, H, W = 2, 9, 65
    seen = set()
    r = ref("piecewise", B, H, W, DIL6)
    imgd = _dev(r.img)
    seen |= gpu_affinity(imgd, (1,))[1]
    affd, n = gpu_affinity(imgd, DIL6)
    seen |= n
    for C in (2, 3, 4):
        md = _dev(R.masks("dense", B, C, H, W))
        seen |= gpu_iterate(affd, md, DIL6)[1]
        seen |= gpu_forward(imgd, md, DIL6, 1, B, False)[1]
        seen |= gpu_forward(imgd, md, DIL6, 1, B, True)[1]
    want = {"par_affinity_kernel", "par_affinity_reg_kernel<6, false>", "par_affinity_reg_kernel<6, true>",
            "par_affinity_reg_kernel<6, true, true>"}
    want |= {f"par_iter_kernel<{cg}, {v}>" for cg in (2, 3, 4) for v in ("false", "true", "true, true, 8, 12")}
    assert want <= seen, f"not exercised: {sorted(want - seen)}"
