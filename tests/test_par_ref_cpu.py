"""The fp64 PAR reference of the kernel tests (tests/par_ref.py) without a GPU: it is the oracle's definition evaluated in
fp64, it reproduces the reference goldens, its bounds admit the fp32 oracle and an emulation of the 16-bit quantiser and
reject the faults a tiled stencil kernel makes (each at the smallest case where it can occur), and every C-ABI limit of the
PAR entry points is refused before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import weclip_oracle as O
from tests import par_ref as R

F64, F32 = torch.float64, torch.float32
WC_ERR_ARG = 1
DIL = list(R.DIL6)


# ---------------------------------------------------------------------------------------------------------------------
# the reference is the oracle's definition

@pytest.mark.parametrize("dil", [R.DIL6, (3,), (2, 5), (1, 2, 4, 8, 12), (1, 2, 3, 4, 6, 8, 12, 24)], ids=str)
def test_reference_is_the_oracle_in_fp64(dil):
    H, W, C = 21, 38, 3
    img = R.images("ramp_noise", 1, H, W, seed=2).double()
    m = R.masks("dense", 1, C, H, W, seed=2).double()
    aff, amax, de, e = R.affinity(img[0], dil)
    ref_aff = O.par_affinity(img, dil)
    assert ref_aff.dtype == F64
    assert (aff - ref_aff).abs().max().item() < 1e-12
    assert torch.equal(amax, aff.max(0).values) and de.max().item() == 0 and torch.equal(de, e - e.max(0).values)
    offs, pi = R.taps(dil)
    assert len(offs) == 8 * len(dil) and offs[:3] == [(-dil[0], -dil[0]), (-dil[0], 0), (-dil[0], dil[0])]
    assert abs((aff.sum(0) - 1 - pi.sum()).abs().max().item()) < 1e-14 and abs(pi.sum().item() - 0.01) < 1e-15
    one = O.par_iterate(ref_aff, m[0], 1, dil)
    assert (R.sweep(aff, m[0], dil) - one).abs().max().item() < 1e-12
    three = O.par(img, m, 3, dil)
    assert three.dtype == F64
    assert (R.forward(img[0], m[0], dil, 3) - three[0]).abs().max().item() < 1e-12


def test_reference_reproduces_the_goldens(golden):
    g = golden("tiny_func.npz")
    img = synth.make_images(2, *synth.TINY_HW)[:1]
    out = R.forward(img[0], torch.from_numpy(g["par_masks"])[0], DIL, 20)
    np.testing.assert_allclose(out.numpy(), g["par_out"][0], rtol=0, atol=3e-5)
    img2 = synth.make_images(1, 37, 53, seed=5)
    out2 = R.forward(img2[0], torch.from_numpy(g["par2_masks"])[0], DIL, 3)
    np.testing.assert_allclose(out2.numpy(), g["par2_out"][0], rtol=0, atol=2e-5)


def test_labels_reference():
    m = torch.tensor([[[[1.0, 2.0, 5.0]], [[1.0, 3.0, 5.0]], [[0.0, 3.0, 9.0]]]])       # (1, 3, 1, 3)
    keys = torch.tensor([[10, 20, 30]])
    assert R.labels(m, keys).tolist() == [[[10, 20, 30]]]                                 # first maximum wins
    assert R.labels(m, keys, torch.tensor([2])).tolist() == [[[10, 20, 10]]]
    assert R.labels(m, keys, torch.tensor([1])).tolist() == [[[10, 10, 10]]]
    x = torch.rand(2, 4, 5, 7)
    assert torch.equal(R.labels(x, torch.arange(8).view(2, 4)), x.argmax(1) + torch.tensor([0, 4]).view(2, 1, 1))


def test_input_builders():
    for kind in R.KINDS:
        a, b = R.images(kind, 2, 9, 65, seed=1), R.images(kind, 2, 9, 65, seed=1)
        assert a.dtype == F32 and a.shape == (2, 3, 9, 65) and torch.equal(a, b) and a.is_contiguous()
    c = R.images("const", 2, 9, 65)
    assert (c == c[:, :, :1, :1]).all()
    p = R.images("piecewise", 1, 9, 65)[0]
    assert (p[:, :, :32] == p[:, :, :1]).all() and (p[0, :, 32:] == p[0, 0, 32]).all() and p[0, 0, 31] != p[0, 0, 32]
    assert p[1, 3, 0] != p[1, 4, 0] and p[0, 3, 0] == p[0, 4, 0]
    pr = R.masks("probes", 2, 3, 40, 72)
    assert set(pr.unique().tolist()) == {0.0, 1.0} and (pr.flatten(2).sum(2) >= 1).all()
    assert 0.3 / 97 < pr.mean().item() < 3.0 / 97
    assert R.masks("probes", 1, 2, 1, 1).sum().item() == 2 and (R.masks("ones", 1, 2, 3, 4) == 1).all()
    d = R.masks("dense", 1, 2, 3, 4)
    assert d.min() >= 0 and d.max() < 1


# ---------------------------------------------------------------------------------------------------------------------
# the bounds admit the fp32 oracle (this is the measurement of K) ...

def _cases():
    """(kind, (H, W)) of the GPU module: all five kinds at (40, 72), const and piecewise at every shape."""
    return [(k, s) for s in R.SHAPES for k in R.KINDS if s == (40, 72) or k in ("const", "piecewise")]


def test_affinity_bound_admits_the_fp32_oracle():
    worst = {}
    for dil in R.AFF_DILS + R.H16_DILS[1:]:
        for kind, (H, W) in _cases():
            img = R.images(kind, 2, H, W, seed=1)
            for b in range(2):
                aff, _, _, e = R.affinity(img[b], dil)
                err = (O.par_affinity(img[b:b + 1], dil).double() - aff).abs()
                worst[kind] = max(worst.get(kind, 0.0), (err / R.aff_unit(aff, e)).max().item())
                assert (err <= R.aff_bound(aff, e, dil)).all(), (dil, kind, H, W)
    print("fp32 oracle affinity, worst err / unit per image kind:", {k: round(v, 3) for k, v in worst.items()})
    k = max(worst.values())
    print(f"K measured {k:.3f}; par_ref.K_MEASURED {R.K_MEASURED}, K_AFF {R.K_AFF}")
    # (the oracle is fp32 torch on the CPU: its last bits may differ between machines, hence the window)
    assert k / 1.25 <= R.K_MEASURED <= 1.25 * k, "par_ref.K_MEASURED is not the measured worst ratio"
    assert 4 * R.K_MEASURED <= R.K_AFF <= 4 * R.K_MEASURED + 1


def test_sweep_bound_admits_the_fp32_oracle():
    worst = [0.0, 0.0]
    for kind, (H, W) in _cases():
        img = R.images(kind, 1, H, W, seed=3)
        for C, mk in ((1, "dense"), (4, "ones"), (7, "probes"), (3, "dense")):
            m = R.masks(mk, 1, C, H, W, seed=C)[0]
            aff, _, _, e = R.affinity(img[0], DIL)
            a32 = O.par_affinity(img, DIL)
            # test-supplied weights: the accumulation term alone
            got = O.par_iterate(a32, m, 1, DIL).double()
            ref = R.sweep(a32.double(), m, DIL)
            b = R.sweep_bound(a32.double(), m, DIL)
            assert ((got - ref).abs() <= b).all(), (kind, H, W, C)
            worst[0] = max(worst[0], ((got - ref).abs() / b.clamp(min=1e-300)).max().item())
            # weights computed in fp32: plus the affinity bound
            ref = R.sweep(aff, m, DIL)
            b = R.sweep_bound(aff, m, DIL, R.aff_bound(aff, e, DIL))
            assert ((got - ref).abs() <= b).all(), (kind, H, W, C)
            worst[1] = max(worst[1], ((got - ref).abs() / b.clamp(min=1e-300)).max().item())
    print(f"fp32 oracle sweep, worst err / bound: given weights {worst[0]:.3g}, own weights {worst[1]:.3g}")


def test_forward_bound_admits_the_fp32_oracle():
    H, W, C = 25, 70, 3
    img = R.images("synth", 1, H, W, seed=4)
    m = R.masks("dense", 1, C, H, W, seed=4)
    aff, _, _, e = R.affinity(img[0], DIL)
    for n in (1, 2, 3):
        err = (O.par(img, m, n, DIL)[0].double() - R.forward(img[0], m[0], DIL, n)).abs()
        assert (err <= R.forward_bound(aff, m[0], DIL, n, R.aff_bound(aff, e, DIL))).all(), n


# ---------------------------------------------------------------------------------------------------------------------
# ... and an emulation of the quantiser, written from its description in csrc/par.hip

def quantise(a32, diffuse=True):
    """a32 (T, H, W) fp32 -> (n (T, H, W) fp32 integers 0..65535, scale (H, W) fp32): scale = amax / 65535, n = clamp(rint(a'
    * 65535 / amax)) with a' = a + carry, carry = a' - n scale handed on in tap order (diffuse=False: plain rounding)."""
    amax = a32.max(0).values
    scale = amax * torch.tensor(1.0 / 65535.0, dtype=F32)
    rs = torch.tensor(65535.0, dtype=F32) / amax
    carry = torch.zeros_like(amax)
    n = torch.empty_like(a32)
    for t in range(a32.shape[0]):
        a = a32[t] + carry
        n[t] = torch.round(a * rs).clamp(0.0, 65535.0)           # torch.round is rintf: half to even
        if diffuse:
            carry = a - n[t] * scale
    return n, scale


def h16_sweep(n, scale, m, dil, swap=False):
    """acc = sum_t n_t m(nbr_t) in fp32, times the scale.  swap: the two halves of every 16-bit pair exchanged."""
    if swap:
        n = n.view(-1, 2, *n.shape[1:]).flip(1).reshape(n.shape)
    return R.sweep_terms(n, m.float(), dil)[0] * scale


@pytest.mark.parametrize("dil", R.H16_DILS, ids=str)
def test_h16_bounds_admit_the_quantiser_emulation(dil):
    worst = {"weight": 0.0, "prefix": 0.0, "dense": 0.0, "abel": 0.0, "ones": 0.0, "probes": 0.0}
    for kind, (H, W) in _cases():
        img = R.images(kind, 1, H, W, seed=5)
        aff, amax, _, e = R.affinity(img[0], dil)
        a32 = O.par_affinity(img, dil)
        n, scale = quantise(a32)
        d = n.double() * scale.double() - a32.double()
        worst["weight"] = max(worst["weight"], (d.abs() / R.h16_weight_bound(amax)).max().item())
        c = 0.5 * amax / 65535 * (1 + 1e-3) + 2 * R.EPS * amax + 2 * R.EPS * aff.sum(0)
        worst["prefix"] = max(worst["prefix"], (d.cumsum(0).abs() / c).max().item())
        for mk in ("dense", "ones", "probes"):
            m = R.masks(mk, 1, 3, H, W, seed=6)[0]
            err = (h16_sweep(n, scale, m, dil).double() - R.sweep(aff, m, dil)).abs()
            b = R.h16_ones_bound(aff, amax, e, dil) if mk == "ones" else R.h16_bound(aff, amax, e, m, dil)
            assert (err <= b).all(), (kind, H, W, mk)
            worst[mk] = max(worst[mk], (err / b).max().item())
            if mk != "ones":
                ba = R.h16_bound(aff, amax, e, m, dil, abel=True)
                assert (err <= ba).all(), (kind, H, W, mk, "abel")
                worst["abel"] = max(worst["abel"], (err / ba).max().item())
    print("quantiser emulation, worst err / bound:", {k: round(v, 4) for k, v in worst.items()})
    assert worst["weight"] <= 1 and worst["prefix"] <= 1


# ---------------------------------------------------------------------------------------------------------------------
# the bounds reject planted faults, each in an fp32 emulation of one sweep

def sweep32(w, m, dil, nbr=None, chan=None, live=None):
    """One fp32 sweep out[c](p) = sum_t w_t(p) m[chan[c]](nbr(t, dy, dx)(p)); nbr -> (yy, xx) index grids, default: clamped to
    the image; live (H, W) bool: pixels that are written (the others stay 0)."""
    C, H, W = m.shape
    Y, X = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
    src = m if chan is None else m[chan]
    out = torch.zeros(C, H, W, dtype=F32)
    for t, (dy, dx) in enumerate(R.taps(dil)[0]):
        yy, xx = (Y + dy, X + dx) if nbr is None else nbr(t, dy, dx, Y, X)
        out = out + w[t] * src[:, yy.clamp(0, H - 1), xx.clamp(0, W - 1)]
    return out if live is None else out * live


def _to_block(Y, X, dy, dx, halo):
    """Neighbour clamped to the pixel's 64 x 8 block grown by `halo` (then, by sweep32, to the image)."""
    y0, x0 = Y // 8 * 8, X // 64 * 64
    return (torch.minimum(torch.maximum(Y + dy, y0 - halo), y0 + 7 + halo),
            torch.minimum(torch.maximum(X + dx, x0 - halo), x0 + 63 + halo))


def _tile_read(m, dy, dx, halo=12):
    """The H16 kernel's near path on a one-block image (H <= 8, W <= 64): the tile of (8 + 2 halo) x (64 + 2 halo) clamped
    values, read at the thread's own index plus dy * TW + dx."""
    C, H, W = m.shape
    TH, TW = 8 + 2 * halo, 64 + 2 * halo
    ty, tx = (torch.arange(TH) - halo).clamp(0, H - 1), (torch.arange(TW) - halo).clamp(0, W - 1)
    tile = m[:, ty][:, :, tx].reshape(C, -1)
    Y, X = torch.arange(H)[:, None], torch.arange(W)[None, :]
    o = ((Y + halo + dy) * TW + X + halo + dx).clamp(0, TH * TW - 1)
    return tile[:, o]


FAULTS = ["tap_off_by_one", "clamp_to_block", "clamp_to_halo_x", "clamp_to_halo_y", "dilation_13_from_the_tile",
          "last_rows_skipped", "last_columns_skipped", "channel_group_reads_last_channel", "pair_halves_swapped",
          "plain_rounding", "second_group_reads_first_images"]


def _planted(fault):
    """-> (got, ref, bound, good): the faulty fp32 result, the fp64 reference, its bound, and the fault-free fp32 result."""
    dil = DIL
    if fault in ("pair_halves_swapped", "plain_rounding", "dilation_13_from_the_tile"):
        kind, (H, W), mk = {"pair_halves_swapped": ("piecewise_noise", (9, 65), "probes"),
                            "plain_rounding": ("const", (1, 1), "ones"),
                            "dilation_13_from_the_tile": ("const", (8, 64), "dense")}[fault]
        dil = [1, 2, 4, 8, 13, 24] if fault == "dilation_13_from_the_tile" else DIL
        img = R.images(kind, 1, H, W, seed=7)
        m = R.masks(mk, 1, 2, H, W, seed=7)[0]
        aff, amax, _, e = R.affinity(img[0], dil)
        a32 = O.par_affinity(img, dil)
        n, scale = quantise(a32)
        ref = R.sweep(aff, m, dil)
        good = h16_sweep(n, scale, m, dil)
        if fault == "pair_halves_swapped":
            return h16_sweep(n, scale, m, dil, swap=True), ref, R.h16_bound(aff, amax, e, m, dil), good
        if fault == "plain_rounding":
            return h16_sweep(quantise(a32, diffuse=False)[0], scale, m, dil), ref, R.h16_ones_bound(aff, amax, e, dil), good
        acc = torch.zeros_like(m)
        for t, (dy, dx) in enumerate(R.taps(dil)[0]):
            acc = acc + n[t] * (_tile_read(m, dy, dx) if abs(dy) <= 13 and abs(dx) <= 13 else R.shift(m, dy, dx))
        return acc * scale, ref, R.h16_bound(aff, amax, e, m, dil), good
    if fault == "second_group_reads_first_images":
        B, C, H, W = 3, 2, 9, 65                                    # group = 2: image 2 is the second group's first
        img = R.images("ramp_noise", B, H, W, seed=8)
        m = R.masks("dense", B, C, H, W, seed=8)
        aff, _, _, e = R.affinity(img[2], dil)
        ref = R.sweep(aff, m[2], dil)
        bound = R.sweep_bound(aff, m[2], dil, R.aff_bound(aff, e, dil))
        return (sweep32(O.par_affinity(img[0:1], dil), m[2], dil), ref, bound,
                sweep32(O.par_affinity(img[2:3], dil), m[2], dil))
    # constant image: every weight is 1/48 + pi_t, a wrong neighbour shows at full strength
    H, W = {"clamp_to_halo_x": (13, 130), "clamp_to_halo_y": (40, 72)}.get(fault, (9, 65))
    C = 5
    img = R.images("const", 1, H, W, seed=9)
    m = R.masks("dense", 1, C, H, W, seed=9)[0]
    aff, _, _, e = R.affinity(img[0], dil)
    a32 = O.par_affinity(img, dil)
    ref = R.sweep(aff, m, dil)
    bound = R.sweep_bound(aff, m, dil, R.aff_bound(aff, e, dil))
    kw = {
        "tap_off_by_one": dict(nbr=lambda t, dy, dx, Y, X: (Y + dy, X + dx + (t == 47))),
        "clamp_to_block": dict(nbr=lambda t, dy, dx, Y, X: _to_block(Y, X, dy, dx, 0)),
        "clamp_to_halo_x": dict(nbr=lambda t, dy, dx, Y, X: _to_block(Y, X, dy, dx, 12)),
        "clamp_to_halo_y": dict(nbr=lambda t, dy, dx, Y, X: _to_block(Y, X, dy, dx, 12)),
        "last_rows_skipped": dict(live=(torch.arange(H) < H // 8 * 8)[:, None].expand(H, W)),
        "last_columns_skipped": dict(live=(torch.arange(W) < W // 64 * 64)[None, :].expand(H, W)),
        "channel_group_reads_last_channel": dict(chan=[0, 1, 2, 3, 4][:3] + [C - 1, C - 1]),
    }[fault]
    return sweep32(a32, m, dil, **kw), ref, bound, sweep32(a32, m, dil)


@pytest.mark.parametrize("fault", FAULTS)
def test_bounds_reject_planted_fault(fault):
    got, ref, bound, good = _planted(fault)
    assert ((good.double() - ref).abs() <= bound).all(), "the fault-free emulation is outside the bound"
    over = (got.double() - ref).abs() / bound.clamp(min=1e-300)
    print(f"{fault}: worst err / bound {over.max().item():.3g} at {int((over > 1).sum())} of {over.numel()} elements; "
          f"fault-free {((good.double() - ref).abs() / bound.clamp(min=1e-300)).max().item():.3g}")
    assert over.max().item() > 1, "the planted fault is admissible"


# ---------------------------------------------------------------------------------------------------------------------
# C-ABI refusals, before any launch (none of the pointers is ever dereferenced)

@pytest.fixture(scope="module")
def so():
    from weclip_vit_comer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, _, args in _lib.parse_header():
        if name.startswith("wc_par"):
            getattr(so, name).argtypes = [t for t, _ in args]
    return so


def _P(i):
    return ctypes.c_void_p(4096 * (i + 1))


D6 = (ctypes.c_int * 6)(1, 2, 4, 8, 12, 24)
D9 = (ctypes.c_int * 9)(*range(1, 10))
D5 = (ctypes.c_int * 5)(1, 2, 4, 8, 12)


def _affinity(so, **kw):
    a = dict(img=_P(0), aff=_P(1), B=2, H=9, W=65, dil=D6, n_dil=6)
    assert set(kw) <= set(a), kw          # an unknown key would leave a valid call that launches
    a.update(kw)
    return so.wc_par_affinity(a["img"], a["aff"], a["B"], a["H"], a["W"], a["dil"], a["n_dil"], None)


def _iterate(so, **kw):
    a = dict(aff=_P(0), src=_P(1), dst=_P(2), B=2, C=3, H=9, W=65, dil=D6, n_dil=6)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return so.wc_par_iterate(a["aff"], a["src"], a["dst"], a["B"], a["C"], a["H"], a["W"], a["dil"], a["n_dil"], None)


def _forward(so, fn, **kw):
    a = dict(img=_P(0), masks=_P(1), out=_P(2), tmp=_P(3), aff_ws=_P(4), B=2, C=3, H=9, W=65, dil=D6, n_dil=6, num_iter=2,
             group=2)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return getattr(so, fn)(a["img"], a["masks"], a["out"], a["tmp"], a["aff_ws"], a["B"], a["C"], a["H"], a["W"], a["dil"],
                           a["n_dil"], a["num_iter"], a["group"], None)


def _kwid(kw):
    """str(kw) with a ctypes array shown by its values (its repr holds an address: a test id that changes from run to run)."""
    return str({k: list(v) if isinstance(v, ctypes.Array) else v for k, v in kw.items()})


_SIZES = [dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-3)]
_DILS = [dict(n_dil=0), dict(n_dil=9, dil=D9), dict(n_dil=-1), dict(dil=None)]


@pytest.mark.parametrize("kw", _SIZES + _DILS + [dict(img=None), dict(aff=None)], ids=_kwid)
def test_par_affinity_refusals(so, kw):
    assert _affinity(so, **kw) == WC_ERR_ARG


@pytest.mark.parametrize("kw", _SIZES + _DILS + [dict(C=0), dict(aff=None), dict(src=None), dict(dst=None),
                                                 dict(dst=_P(1))], ids=_kwid)
def test_par_iterate_refusals(so, kw):
    assert _iterate(so, **kw) == WC_ERR_ARG


@pytest.mark.parametrize("fn", ["wc_par_forward", "wc_par_forward_h"])
@pytest.mark.parametrize("kw", _SIZES + _DILS + [
    dict(C=0), dict(num_iter=0), dict(num_iter=-1), dict(group=0), dict(group=-2), dict(out=_P(1)), dict(tmp=_P(1)),
    dict(out=_P(3)), dict(img=None), dict(masks=None), dict(out=None), dict(tmp=None), dict(aff_ws=None)], ids=_kwid)
def test_par_forward_refusals(so, fn, kw):
    assert _forward(so, fn, **kw) == WC_ERR_ARG


def test_par_forward_h_needs_six_dilations(so):
    assert _forward(so, "wc_par_forward_h", dil=D5, n_dil=5) == WC_ERR_ARG
    from weclip_vit_comer_amd import _lib
    with pytest.raises(RuntimeError, match="6 dilations"):
        _lib.lib().wc_par_forward_h(_P(0), _P(1), _P(2), _P(3), _P(4), 2, 3, 9, 65, D5, 5, 2, 2, None)
    with pytest.raises(RuntimeError, match="alias"):
        _lib.lib().wc_par_forward(_P(0), _P(1), _P(2), _P(2), _P(4), 2, 3, 9, 65, D6, 6, 2, 2, None)
    with pytest.raises(RuntimeError, match="in-place"):
        _lib.lib().wc_par_iterate(_P(0), _P(1), _P(1), 2, 3, 9, 65, D6, 6, None)


@pytest.mark.parametrize("kw", [dict(masks=None), dict(keys=None), dict(labels=None), dict(B=0), dict(C=0), dict(H=0),
                                dict(W=0)], ids=str)
def test_par_labels_refusals(so, kw):
    a = dict(masks=_P(0), keys=_P(1), nch=None, labels=_P(2), B=2, C=3, H=9, W=65)
    assert set(kw) <= set(a), kw
    a.update(kw)
    assert so.wc_par_labels(a["masks"], a["keys"], a["nch"], a["labels"], a["B"], a["C"], a["H"], a["W"], None) == WC_ERR_ARG
