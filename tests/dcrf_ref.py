"""Float64 CPU reference of the dense CRF model (DESIGN.md "Dense CRF"; include/weclip_hip.h wc_dcrf_*).

Exact all-pairs sums (no truncation, no lattice), vectorised in torch and chunked over query rows so that a 500x375
image needs only a (rows x N) block at a time.  Image (H,W,3) HWC, probabilities / Q (C,H,W)."""
import math

import torch

F64 = torch.float64


def _features(img, H, W, xy_std, rgb_std=None):
    img = torch.as_tensor(img).to(F64).reshape(H * W, 3)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    f = [xs.reshape(-1) / xy_std, ys.reshape(-1) / xy_std]
    if rgb_std is not None:
        f += [img[:, c] / rgb_std for c in range(3)]
    f = torch.stack(f, 1)
    return f - f.mean(0)                   # centred: the fp64 differences stay exact to far below what the tests resolve


def kernel_sums(f, V, chunk=None):
    """out (N, K) = sum_j exp(-|f_i - f_j|^2 / 2) V(j, :) for V (N, K), fp64, chunked over i."""
    N = f.shape[0]
    chunk = chunk or max(1, (1 << 24) // N)
    out = torch.empty(N, V.shape[1], dtype=F64)
    for s in range(0, N, chunk):
        d2 = torch.cdist(f[s:s + chunk], f, compute_mode="donot_use_mm_for_euclid_dist").square_()
        out[s:s + chunk] = torch.exp(-0.5 * d2) @ V
    return out


def unary_from_prob(P):
    return -torch.log(torch.as_tensor(P).to(F64).clamp(1e-5, 1.0))


def unary_from_labels(labels, n_labels, gt_prob):
    lab = torch.as_tensor(labels).long()
    U = torch.full((n_labels,) + tuple(lab.shape), -math.log((1 - gt_prob) / (n_labels - 1)), dtype=F64)
    for c in range(n_labels):
        U[c][lab == c] = -math.log(gt_prob)
    return U


def messages(img, Q, pos_xy_std, bi_xy_std, bi_rgb_std, rows=None, S_given=None):
    """(M_pos, M_bil, S_pos, S_bil): M_m (C,H,W) = n_m(i) sum_j k_m(i,j) n_m(j) Q(:,j), S_m (H,W).
    rows: optional index tensor of query pixels -- then M (C, len(rows)) and S (len(rows),).  S_given: optional (S_pos, S_bil)
    of every pixel to take n_m(j) from (at full size the all-pairs S costs N^2 exps; S itself is then checked at `rows`)."""
    Q = torch.as_tensor(Q).to(F64)
    C, H, W = Q.shape
    N = H * W
    Qf = Q.reshape(C, N).T
    out = []
    for m, f in enumerate((_features(img, H, W, pos_xy_std), _features(img, H, W, bi_xy_std, bi_rgb_std))):
        if S_given is None:
            S = kernel_sums(f, torch.ones(N, 1, dtype=F64))[:, 0]
        else:
            S = torch.as_tensor(S_given[m]).to(F64).reshape(N)
        n = S.rsqrt()
        if rows is None:
            M = n[:, None] * kernel_sums(f, n[:, None] * Qf)
            out.append((M.T.reshape(C, H, W), S.reshape(H, W)))
        else:
            d2 = torch.cdist(f[rows], f, compute_mode="donot_use_mm_for_euclid_dist").square_()
            k = torch.exp(-0.5 * d2)
            M = n[rows, None] * (k @ (n[:, None] * Qf))
            out.append((M.T, k.sum(1)))
    (mp, sp), (mb, sb) = out
    return mp, mb, sp, sb


def inference(img, U, iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std):
    """Q (C,H,W) fp64 after iter_max mean-field updates from Q0 = softmax(-U)."""
    U = torch.as_tensor(U).to(F64)
    C, H, W = U.shape
    N = H * W
    fp, fb = _features(img, H, W, pos_xy_std), _features(img, H, W, bi_xy_std, bi_rgb_std)
    ones = torch.ones(N, 1, dtype=F64)
    npos, nbil = kernel_sums(fp, ones)[:, 0].rsqrt(), kernel_sums(fb, ones)[:, 0].rsqrt()
    Uf = U.reshape(C, N).T
    Q = torch.softmax(-Uf, 1)
    for _ in range(iter_max):
        m = pos_w * npos[:, None] * kernel_sums(fp, npos[:, None] * Q) + bi_w * nbil[:, None] * kernel_sums(fb, nbil[:, None] * Q)
        Q = torch.softmax(-Uf + m, 1)
    return Q.T.reshape(C, H, W)


def gauss_radius(std):
    """Truncation radius of the separable Gaussian pass: exp(-R^2 / (2 std^2)) <= 2^-30."""
    return int(math.ceil(std * math.sqrt(60.0 * math.log(2.0))))


def gauss_separable(V, std, R=None):
    """sum over |dx|, |dy| <= R of exp(-(dx^2 + dy^2) / (2 std^2)) V(:, y + dy, x + dx) for V (C,H,W), fp64."""
    V = torch.as_tensor(V).to(F64)
    C, H, W = V.shape
    R = gauss_radius(std) if R is None else R
    def one_d(n):
        d = torch.arange(n, dtype=F64)
        dd = d[:, None] - d[None, :]
        return torch.exp(-dd.square() / (2 * std * std)) * (dd.abs() <= R)
    Ky, Kx = one_d(H), one_d(W)
    return torch.einsum("yv,cvu,xu->cyx", Ky, V, Kx)
