"""The fp64 dense CRF reference (tests/dcrf_ref.py) that the GPU tests rely on, checked against the model's definition."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcrf_ref as R  # noqa: E402

F64 = torch.float64
PARAMS = dict(pos_w=3.0, pos_xy_std=1.5, bi_w=4.0, bi_xy_std=2.0, bi_rgb_std=30.0)


def _case(H=5, W=7, C=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (H, W, 3), generator=g).to(torch.uint8)
    P = torch.softmax(2 * torch.randn(C, H, W, generator=g, dtype=F64), 0)
    return img, P


def _loop_inference(img, U, t, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std):
    """The model written out pixel by pixel (plain Python loops)."""
    C, H, W = U.shape
    pix = [(x, y) for y in range(H) for x in range(W)]
    col = [[float(v) for v in img[y, x]] for (x, y) in pix]
    N = len(pix)

    def kpos(i, j):
        return math.exp(-((pix[i][0] - pix[j][0]) ** 2 + (pix[i][1] - pix[j][1]) ** 2) / (2 * pos_xy_std ** 2))

    def kbil(i, j):
        d = ((pix[i][0] - pix[j][0]) ** 2 + (pix[i][1] - pix[j][1]) ** 2) / (2 * bi_xy_std ** 2)
        d += sum((col[i][c] - col[j][c]) ** 2 for c in range(3)) / (2 * bi_rgb_std ** 2)
        return math.exp(-d)
    n_p = [sum(kpos(i, j) for j in range(N)) ** -0.5 for i in range(N)]
    n_b = [sum(kbil(i, j) for j in range(N)) ** -0.5 for i in range(N)]
    u = [[float(U[l, pix[i][1], pix[i][0]]) for l in range(C)] for i in range(N)]

    def softmax(z):
        m = max(z)
        e = [math.exp(v - m) for v in z]
        return [v / sum(e) for v in e]
    Q = [softmax([-v for v in u[i]]) for i in range(N)]
    for _ in range(t):
        Q = [softmax([-u[i][l] + pos_w * n_p[i] * sum(kpos(i, j) * n_p[j] * Q[j][l] for j in range(N))
                      + bi_w * n_b[i] * sum(kbil(i, j) * n_b[j] * Q[j][l] for j in range(N)) for l in range(C)])
             for i in range(N)]
    out = torch.empty(C, H, W, dtype=F64)
    for i, (x, y) in enumerate(pix):
        out[:, y, x] = torch.tensor(Q[i], dtype=F64)
    return out


def test_reference_matches_pixel_loop():
    img, P = _case()
    U = R.unary_from_prob(P)
    for t in (0, 1, 3):
        assert torch.allclose(R.inference(img, U, t, **PARAMS), _loop_inference(img, U, t, **PARAMS), atol=1e-12, rtol=0)


def test_q_is_normalised():
    img, P = _case(9, 11, 4, seed=1)
    Q = R.inference(img, R.unary_from_prob(P), 5, **PARAMS)
    assert (Q.sum(0) - 1).abs().max().item() < 1e-12 and (Q >= 0).all()


def test_no_iterations_or_no_weights_give_softmax_of_minus_u():
    img, P = _case(6, 8, 3, seed=2)
    U = R.unary_from_prob(P)
    s = torch.softmax(-U, 0)
    assert torch.allclose(R.inference(img, U, 0, **PARAMS), s, atol=1e-14)
    p = dict(PARAMS, pos_w=0.0, bi_w=0.0)
    assert torch.allclose(R.inference(img, U, 4, **p), s, atol=1e-14)


def test_permuting_labels_permutes_q():
    img, P = _case(6, 8, 5, seed=3)
    perm = torch.tensor([3, 0, 4, 1, 2])
    Q = R.inference(img, R.unary_from_prob(P), 4, **PARAMS)
    Qp = R.inference(img, R.unary_from_prob(P[perm]), 4, **PARAMS)
    assert torch.allclose(Qp, Q[perm], atol=1e-13)


@pytest.mark.parametrize("std", [0.5, 3.0, 7.0])
def test_truncated_separable_gaussian_within_bound(std):
    """The kernels' separable Gaussian drops |d| > R = ceil(std sqrt(60 ln 2)); the dropped mass stays below 2^-29 S."""
    g = torch.Generator().manual_seed(4)
    H, W = 60, 90
    V = torch.rand(2, H, W, generator=g, dtype=F64)
    img = torch.zeros(H, W, 3)
    big = R.gauss_separable(V, std, R=max(H, W))
    cut = R.gauss_separable(V, std)
    S = R.gauss_separable(torch.ones(1, H, W, dtype=F64), std, R=max(H, W))[0]
    assert ((big - cut).abs() <= 2.0 ** -29 * S * V.max()).all()
    mp, _, sp, _ = R.messages(img, V, std, 1.0, 1.0)        # the dense fp64 message is the untruncated separable sum
    n = sp.rsqrt()
    assert torch.allclose(mp, n * R.gauss_separable(n * V, std, R=max(H, W)), rtol=1e-12, atol=0)
    assert math.exp(-R.gauss_radius(std) ** 2 / (2 * std * std)) <= 2.0 ** -30


def test_unary_helpers_follow_their_formulas():
    P = torch.tensor([[0.0, 1e-7, 0.3, 1.0, 1.5]], dtype=F64)
    assert torch.allclose(R.unary_from_prob(P), -torch.log(torch.tensor([[1e-5, 1e-5, 0.3, 1.0, 1.0]], dtype=F64)))
    lab = torch.tensor([[0, 2], [1, 255]])
    U = R.unary_from_labels(lab, 3, 0.7)
    on, off = -math.log(0.7), -math.log((1 - 0.7) / 2)
    assert U.shape == (3, 2, 2)
    assert U[0, 0, 0] == on and U[2, 0, 1] == on and U[1, 1, 0] == on and U[1, 0, 0] == off
    assert (U[:, 1, 1] == off).all()
