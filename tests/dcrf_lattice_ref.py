"""Float64 numpy restatement of the permutohedral-lattice bilateral filter (Adams, Baek, Davis 2010; d = 5) that
csrc/dcrf_lattice.hip is pinned to (DESIGN.md "Dense CRF", include/weclip_hip.h wc_dcrf_lattice_*).

build: scale, elevate, nearest zero-remainder point, rank, barycentric weights, packed vertex keys, unique vertices and
their blur neighbours.  filter: splat, d + 1 blur passes new = old + (n1 + n2) / 2, slice with alpha = 1 / (1 + 2^-d).
message / inference: the symmetric normalisation of the exact path around that filter; the Gaussian term and the unaries
come from tests/dcrf_ref.py.  Vectorised (packed keys + searchsorted): 500x375 takes seconds."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcrf_ref as R  # noqa: E402

D = 5
BITS = 12                       # bits per packed key coordinate
BIAS = 1 << (BITS - 1)
ALPHA = 1.0 / (1.0 + 2.0 ** -D)
SCALE = np.array([math.sqrt(2.0 / 3.0) * (D + 1) / math.sqrt((j + 1) * (j + 2)) for j in range(D)])
CANON = np.array([[r if m <= D - r else r - (D + 1) for m in range(D + 1)] for r in range(D + 1)], dtype=np.int64)
SHIFT = np.array([BITS * (D - 1 - i) for i in range(D)], dtype=np.int64)


class Lattice(object):
    """bary (N, d+1) fp64 weights, vert (N, d+1) vertex indices 1..M (0 = the absent vertex, an all-zero value row),
    nbr (d+1, 2, M+1) blur neighbours of every vertex along every direction, M unique vertices."""

    def __init__(self, bary, vert, nbr, M, keys):
        self.bary, self.vert, self.nbr, self.M, self.keys = bary, vert, nbr, M, keys


def features(img, H, W, xy_std, rgb_std):
    img = np.asarray(torch.as_tensor(img).to(torch.float64).numpy()).reshape(H * W, 3)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([xs.reshape(-1) / xy_std, ys.reshape(-1) / xy_std] + [img[:, c] / rgb_std for c in range(3)], 1)


def build(img, H, W, xy_std, rgb_std):
    N = H * W
    c = features(img, H, W, float(xy_std), float(rgb_std)) * SCALE
    e = np.empty((N, D + 1))
    sm = np.zeros(N)
    for j in range(D, 0, -1):
        e[:, j] = sm - j * c[:, j - 1]
        sm = sm + c[:, j - 1]
    e[:, 0] = sm
    v = e / (D + 1)
    up, dn = np.ceil(v) * (D + 1), np.floor(v) * (D + 1)
    rem0 = np.where(up - e < e - dn, up, dn)
    tot = np.rint((rem0 / (D + 1)).sum(1)).astype(np.int64)
    delta = e - rem0
    rank = np.zeros((N, D + 1), dtype=np.int64)
    for i in range(D + 1):
        for j in range(i + 1, D + 1):
            lt = delta[:, i] < delta[:, j]
            rank[:, i] += lt
            rank[:, j] += ~lt
    rank += tot[:, None]
    neg, big = rank < 0, rank > D
    rank = rank + (D + 1) * neg - (D + 1) * big
    rem0 = rem0 + (D + 1) * neg - (D + 1) * big
    t = (e - rem0) / (D + 1)
    b = np.zeros((N, D + 2))
    rows = np.arange(N)
    for i in range(D + 1):
        b[rows, D - rank[:, i]] += t[:, i]
        b[rows, D + 1 - rank[:, i]] -= t[:, i]
    b[:, 0] += 1.0 + b[:, D + 1]
    bary = b[:, :D + 1]
    r0 = rem0[:, :D].astype(np.int64)
    k = r0[:, None, :] + CANON[:, rank[:, :D]].transpose(1, 0, 2)                 # (N, d+1 vertices, d coordinates)
    assert (np.abs(k) + D + 1 < BIAS).all(), "key outside the packing"
    packed = ((k + BIAS) << SHIFT).sum(2)                                       # (N, d+1)
    keys, inv = np.unique(packed.reshape(-1), return_inverse=True)
    M = len(keys)
    vert = inv.reshape(N, D + 1) + 1
    nbr = np.zeros((D + 1, 2, M + 1), dtype=np.int64)
    for j in range(D + 1):
        off = -np.ones(D, dtype=np.int64)
        if j < D:
            off[j] = D
        dp = int((off << SHIFT).sum())
        for s, sign in enumerate((1, -1)):
            want = keys + sign * dp
            pos = np.minimum(np.searchsorted(keys, want), M - 1)
            nbr[j, s, 1:] = np.where(keys[pos] == want, pos + 1, 0)
    return Lattice(bary, vert, nbr, M, keys)


def filter(lat, values, reverse=False):
    """values (N, K) fp64 -> the un-normalised filter (N, K).  reverse: blur along d..0 instead of 0..d, which is the
    adjoint (the passes do not commute where a neighbour is absent, so the filter itself is not symmetric)."""
    values = np.asarray(values, dtype=np.float64)
    N, K = values.shape
    flat = lat.vert.reshape(-1)
    order = np.argsort(flat, kind="stable")
    starts = np.flatnonzero(np.r_[True, flat[order][1:] != flat[order][:-1]])
    val = np.zeros((lat.M + 1, K))
    val[1:] = np.add.reduceat(lat.bary.reshape(-1)[order, None] * values[order // (D + 1)], starts, axis=0)
    for j in (range(D, -1, -1) if reverse else range(D + 1)):
        val = val + 0.5 * (val[lat.nbr[j, 0]] + val[lat.nbr[j, 1]])
        val[0] = 0.0
    out = np.zeros((N, K))
    for r in range(D + 1):
        out += lat.bary[:, r, None] * val[lat.vert[:, r]]
    return ALPHA * out


def filter_planes(lat, V):
    """(C,H,W) -> (C,H,W), the layout of wc_dcrf_lattice_filter."""
    V = np.asarray(torch.as_tensor(V).to(torch.float64).numpy())
    C, H, W = V.shape
    return filter(lat, V.reshape(C, -1).T).T.reshape(C, H, W)


def normaliser(lat):
    S = filter(lat, np.ones((lat.bary.shape[0], 1)))[:, 0]
    return S, (S + 1e-20) ** -0.5


def message(lat, Q):
    """(M_bil (C,H,W), S_bil (H,W)): M_bil(:, i) = n(i) filter(n Q)(i), n = (filter(1) + 1e-20)^-1/2."""
    Q = np.asarray(torch.as_tensor(Q).to(torch.float64).numpy())
    C, H, W = Q.shape
    S, n = normaliser(lat)
    M = n[:, None] * filter(lat, n[:, None] * Q.reshape(C, -1).T)
    return M.T.reshape(C, H, W), S.reshape(H, W)


def inference(img, U, iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std):
    """Q (C,H,W) fp64 torch tensor after iter_max mean-field updates from softmax(-U); exact Gaussian term, lattice
    bilateral term."""
    U = torch.as_tensor(U).to(torch.float64)
    C, H, W = U.shape
    N = H * W
    lat = build(img, H, W, bi_xy_std, bi_rgb_std)
    _, nb = normaliser(lat)
    nb = torch.from_numpy(nb)
    fp = R._features(img, H, W, pos_xy_std)
    npos = R.kernel_sums(fp, torch.ones(N, 1, dtype=torch.float64))[:, 0].rsqrt()
    Uf = U.reshape(C, N).T
    Q = torch.softmax(-Uf, 1)
    for _ in range(iter_max):
        mb = nb[:, None] * torch.from_numpy(filter(lat, (nb[:, None] * Q).numpy()))
        m = pos_w * npos[:, None] * R.kernel_sums(fp, npos[:, None] * Q) + bi_w * mb
        Q = torch.softmax(-Uf + m, 1)
    return Q.T.reshape(C, H, W)
