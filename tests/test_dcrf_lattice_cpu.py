"""The permutohedral-lattice bilateral term without a GPU: properties of the fp64 restatement tests/dcrf_lattice_ref.py, and
the host side of the feature (header, keyword, parser, a-priori key bound)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import weclip_vit_comer_amd  # noqa: F401
from weclip_vit_comer_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcrf_lattice_ref as LR  # noqa: E402
import dcrf_ref as R  # noqa: E402

WC_ERR_ARG = 1
SYMBOLS = ("wc_dcrf_lattice_key_bound", "wc_dcrf_lattice_workspace_bytes", "wc_dcrf_lattice_build", "wc_dcrf_lattice_filter",
           "wc_dcrf_lattice_message", "wc_dcrf_lattice_inference")


def _random_image(H, W, seed):
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _smooth_image(H, W, seed):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(3, 4, 5, generator=g) * 255
    return (F.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
            + 6 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)


@pytest.fixture(scope="module", params=[("random", 16.0, 13.0), ("random", 64.0, 5.0), ("smooth", 64.0, 5.0), ("smooth", 80.0, 13.0)])
def lattice(request):
    kind, xy, rgb = request.param
    H, W = 37, 53
    img = _random_image(H, W, 1) if kind == "random" else _smooth_image(H, W, 2)
    return LR.build(img, H, W, xy, rgb), H * W


def test_weights_are_a_partition_of_one(lattice):
    lat, N = lattice
    assert lat.bary.shape == (N, LR.D + 1) and lat.bary.min() >= -1e-12
    assert np.abs(lat.bary.sum(1) - 1).max() <= 1e-12
    assert lat.vert.min() >= 1 and lat.vert.max() == lat.M <= (LR.D + 1) * N


def test_random_colours_are_near_the_capacity_worst_case():
    lat = LR.build(_random_image(37, 53, 1), 37, 53, 16.0, 13.0)
    assert lat.M > 0.9 * (LR.D + 1) * 37 * 53


def test_filter_is_linear(lattice):
    lat, N = lattice
    rng = np.random.default_rng(0)
    u, v = rng.random((N, 3)), rng.random((N, 3))
    a = LR.filter(lat, 2.0 * u - 0.5 * v)
    b = 2.0 * LR.filter(lat, u) - 0.5 * LR.filter(lat, v)
    assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max()


def test_filter_symmetry(lattice):
    """Splat and slice are transposes and every blur pass is a symmetric matrix, so <u, F v> = <F' u, v> with F' the same
    filter blurring along d..0.  (<u, F v> = <F u, v> itself holds only where the passes commute: not where a blur neighbour
    is absent, which on a sparse lattice is nearly everywhere -- the two differ by ~1e-3 relative on these images.)"""
    lat, N = lattice
    rng = np.random.default_rng(1)
    u, v = rng.random((N, 3)), rng.random((N, 3))
    lhs, rhs = (u * LR.filter(lat, v)).sum(), (LR.filter(lat, u, reverse=True) * v).sum()
    assert abs(lhs - rhs) <= 1e-9 * abs(lhs)
    # each pass is symmetric: n2 undoes n1 wherever n1 exists
    idx = np.arange(lat.M + 1)
    for j in range(LR.D + 1):
        for a, b in ((0, 1), (1, 0)):
            has = lat.nbr[j, a] > 0
            assert (lat.nbr[j, b][lat.nbr[j, a][has]] == idx[has]).all()


def test_lattice_crf_labels_flat_regions():
    """The flat-regions case of test_dcrf_gpu.test_crf_labels_flat_regions, through the restatement."""
    H, W = 48, 64
    img = np.zeros((H, W, 3), np.uint8)
    img[:, :32] = (200, 40, 40)
    img[:, 32:] = (30, 60, 220)
    truth = np.zeros((H, W), np.int64)
    truth[:, 32:] = 1
    rng = np.random.default_rng(0)
    p1 = np.clip(np.where(truth == 1, 0.65, 0.35) + rng.normal(0, 0.25, (H, W)), 0.01, 0.99)
    P = np.stack([1 - p1, p1]).astype(np.float32)
    assert (P.argmax(0) != truth).mean() > 0.25
    Q = LR.inference(img, R.unary_from_prob(P), 10, 3, 3, 10, 50, 5)
    assert (Q.argmax(0).numpy() == truth).all()


# ---------------------------------------------------------------------------------------------- host side of the feature
def test_header_declares_the_lattice_entries_and_the_library_has_them():
    names = {n for n, _, _ in _lib.parse_header()}
    assert set(SYMBOLS) <= names
    lib = _lib.lib()
    for s in SYMBOLS:
        assert callable(getattr(lib, s))


def test_bilateral_keyword():
    import inspect
    from weclip_vit_comer_amd.utils import dcrf
    assert dcrf.DenseCRF(10, 3, 3, 4, 64, 5).bilateral == "exact"
    assert dcrf.DenseCRF(10, 3, 3, 4, 64, 5, bilateral="lattice").bilateral == "lattice"
    with pytest.raises(ValueError):
        dcrf.DenseCRF(10, 3, 3, 4, 64, 5, bilateral="nope")
    for fn in (dcrf.inference, dcrf.message, dcrf.crf_inference, dcrf.crf_inference_label, dcrf.DenseCRF.__init__):
        assert inspect.signature(fn).parameters["bilateral"].default == "exact"
    assert "bilateral" in inspect.signature(dcrf.DenseCRF.with_unary).parameters
    img, P = np.zeros((4, 5, 3), np.uint8), np.full((2, 4, 5), 0.5, np.float32)
    for call in (lambda: dcrf.crf_inference(img, P, labels=2, bilateral="nope"),
                 lambda: dcrf.crf_inference_label(img, np.zeros((4, 5), np.int64), n_labels=2, bilateral="nope"),
                 lambda: dcrf.inference(img, torch.zeros(2, 4, 5), 1, 3, 3, 4, 64, 5, bilateral="nope"),
                 lambda: dcrf.message(img, torch.zeros(2, 4, 5), 3, 64, 5, bilateral="nope")):
        with pytest.raises(ValueError):
            call()
    assert callable(dcrf.lattice_filter)


def test_eval_parser_knows_crf_bilateral():
    from weclip_vit_comer_amd import msc_flip_eval
    p = msc_flip_eval.build_parser()
    assert p.parse_args([]).crf_bilateral == "exact"
    assert p.parse_args(["--crf", "--crf_bilateral", "lattice"]).crf_bilateral == "lattice"
    with pytest.raises(SystemExit):
        p.parse_args(["--crf_bilateral", "nope"])


def test_torch_op_is_listed():
    from weclip_vit_comer_amd import torch_ops
    assert "dense_crf_lattice" in torch_ops.OPS
    assert torch.ops.weclip.dense_crf_lattice.default._schema.arguments[-1].name == "bi_rgb_std"


@pytest.fixture(scope="module")
def so():
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, _, args in _lib.parse_header():
        if name.startswith("wc_dcrf_lattice"):
            getattr(so, name).argtypes = [t for t, _ in args]
    return so


def test_key_bound_accepts_the_reference_parameters_and_refuses_tiny_stds(so):
    b = ctypes.c_double(-1.0)
    for xy, rgb in ((80.0, 13.0), (50.0, 5.0), (64.0, 5.0)):
        assert so.wc_dcrf_lattice_key_bound(640, 640, xy, rgb, ctypes.byref(b)) == 0 and 20 < b.value <= 2047
    assert so.wc_dcrf_lattice_key_bound(640, 640, 64.0, 0.1, ctypes.byref(b)) == WC_ERR_ARG and b.value > 2047
    assert so.wc_dcrf_lattice_key_bound(1, 409600, 64.0, 5.0, ctypes.byref(b)) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_key_bound(641, 640, 64.0, 5.0, ctypes.byref(b)) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_key_bound(8, 8, 0.0, 5.0, ctypes.byref(b)) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_key_bound(8, 8, 64.0, float("nan"), ctypes.byref(b)) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_key_bound(8, 8, 64.0, 5.0, None) == WC_ERR_ARG


def test_key_bound_covers_the_restatement():
    """The host's bound is an upper bound on every key coordinate the restatement produces (random colours, both extremes)."""
    b = ctypes.c_double()
    H, W = 37, 53
    img = _random_image(H, W, 3)
    img[0, 0], img[-1, -1] = 255, 255
    for xy, rgb in ((16.0, 13.0), (0.2, 13.0), (64.0, 1.0)):
        _lib.lib().wc_dcrf_lattice_key_bound(H, W, xy, rgb, ctypes.byref(b))
        lat = LR.build(img, H, W, xy, rgb)
        coords = ((lat.keys[:, None] >> LR.SHIFT) & ((1 << LR.BITS) - 1)) - LR.BIAS
        assert np.abs(coords).max() + LR.D <= b.value


P = ctypes.c_void_p(256)           # never dereferenced: every call below is rejected before any launch


def test_entries_check_their_limits_before_any_launch(so):
    assert so.wc_dcrf_lattice_build(P, 1, P, 640, 640, 64.0, 0.1, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_build(P, 1, P, 0, 8, 64.0, 5.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_build(None, 1, P, 8, 8, 64.0, 5.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_build(P, 1, None, 8, 8, 64.0, 5.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_filter(P, P, P, P, P, 129, 8, 8, 10, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_filter(P, P, P, P, P, 21, 8, 8, 0, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_filter(P, P, P, P, P, 21, 8, 8, 6 * 64 + 1, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_filter(P, P, None, P, P, 21, 8, 8, 10, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_message(P, P, P, P, P, P, P, 21, 700, 700, 10, 3.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_message(P, P, P, P, P, P, P, 21, 8, 8, 10, 0.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_inference(P, P, P, P, P, 21, 8, 8, 10, -1, 3.0, 3.0, 4.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_inference(P, P, P, P, P, 0, 8, 8, 10, 10, 3.0, 3.0, 4.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_inference(P, P, P, P, P, 21, 8, 8, 10, 10, 3.0, float("inf"), 4.0, None) == WC_ERR_ARG
    assert so.wc_dcrf_lattice_inference(P, None, P, P, P, 21, 8, 8, 10, 10, 3.0, 3.0, 4.0, None) == WC_ERR_ARG
    n = ctypes.c_long(-7)
    assert so.wc_dcrf_lattice_workspace_bytes(200, 8, 8, ctypes.byref(n), ctypes.byref(n)) == WC_ERR_ARG and n.value == -7
