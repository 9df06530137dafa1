"""Float64 restatement of the multi-bandwidth RBF MMD (include/weclip_hip.h wc_mmd_*), written from the
closed form, not from the reference's code.  With X = cat(source, target), N = 2 B rows, s = +1 on source and -1 on target rows:

    L2_ij = |x_i - x_j|^2
    bandwidth = fix_sigma, or sum_ij L2_ij / (N^2 - N) when fix_sigma is falsy;  then / kernel_mul^(kernel_num // 2)
    bw_b  = bandwidth * kernel_mul^b,  b = 0 .. kernel_num - 1
    K_ij  = sum_b exp(-L2_ij / bw_b)            W_ij = sum_b exp(-L2_ij / bw_b) / bw_b
    loss  = (1 / B^2) sum_ij s_i s_j K_ij
    grad_i = -(4 / B^2) s_i ((sum_j s_j W_ij) x_i - sum_j s_j W_ij x_j)        (bandwidth a constant)

and the two absolute scales of the kernels' error model:

    A    = (1 / B^2) sum_ij K_ij
    G_ic = (4 / B^2) (sum_j W_ij |x_ic| + sum_j W_ij |x_jc|)

Everything runs in row chunks, so the (N, N) matrix is only held when `want_K` asks for it; `device` moves the work (the GPU
tests run their large cases with fp64 stock ops on the device)."""
import torch

F64 = torch.float64


def bandwidth_bruteforce(X):
    """sum_ij L2_ij / (N^2 - N) from the all-pairs differences."""
    X = X.to(F64)
    N = X.shape[0]
    L2 = (X[:, None, :] - X[None, :, :]).square().sum(2)
    return L2.sum() / (N * N - N)


def bandwidth_centred(X):
    """The same number from the centred rows alone: sum_ij |c_i - c_j|^2 = 2 N sum_i |c_i|^2 when sum_i c_i = 0."""
    X = X.to(F64)
    N = X.shape[0]
    c = X - X.mean(0, keepdim=True)
    return 2.0 * c.square().sum() / (N - 1)


def _l2_rows(X, r0, r1):
    if X.shape[0] * (r1 - r0) * X.shape[1] <= (1 << 24):
        return (X[r0:r1, None, :] - X[None, :, :]).square().sum(2)
    # large chunks: the distance routine that sums squared differences too (no matrix product), without the expanded tensor
    return torch.cdist(X[r0:r1], X, compute_mode="donot_use_mm_for_euclid_dist").square()


def mmd(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None, want_K=False, want_grad=True, chunk=1024, device=None):
    """dict(loss, A, grad_source, grad_target, G_source, G_target, K, bandwidth), fp64 tensors (K only with want_K, the gradient
    entries only with want_grad)."""
    s64 = torch.as_tensor(source).detach().to(device=device, dtype=F64)
    t64 = torch.as_tensor(target).detach().to(device=device, dtype=F64)
    assert s64.dim() == 2 and s64.shape == t64.shape
    B, d = s64.shape
    X = torch.cat([s64, t64], 0)
    N = 2 * B
    Xc = X - X.mean(0, keepdim=True)                       # L2 is translation invariant; centred differences lose nothing
    bw = torch.as_tensor(float(fix_sigma), dtype=F64, device=X.device) if fix_sigma else bandwidth_centred(X)
    bw = bw / kernel_mul ** (kernel_num // 2)
    bws = [bw * kernel_mul ** b for b in range(kernel_num)]
    sign = torch.cat([torch.ones(B, dtype=F64, device=X.device), -torch.ones(B, dtype=F64, device=X.device)])
    absX = X.abs()
    loss = torch.zeros((), dtype=F64, device=X.device)
    A = torch.zeros((), dtype=F64, device=X.device)
    grad = torch.empty(N, d, dtype=F64, device=X.device) if want_grad else None
    G = torch.empty(N, d, dtype=F64, device=X.device) if want_grad else None
    Kfull = torch.empty(N, N, dtype=F64, device=X.device) if want_K else None
    for r0 in range(0, N, chunk):
        r1 = min(N, r0 + chunk)
        L2 = _l2_rows(Xc, r0, r1)
        idx = torch.arange(r0, r1, device=X.device)
        L2[idx - r0, idx] = 0.0
        K = torch.zeros_like(L2)
        W = torch.zeros_like(L2)
        for b in bws:
            e = torch.exp(-L2 / b)
            K += e
            W += e / b
        loss += (sign[r0:r1, None] * sign[None, :] * K).sum()
        A += K.sum()
        if want_K:
            Kfull[r0:r1] = K
        if want_grad:
            P = W * sign[None, :]
            grad[r0:r1] = (-4.0 / (B * B)) * sign[r0:r1, None] * (P.sum(1, keepdim=True) * Xc[r0:r1] - P @ Xc)   # (the mean drops out)
            G[r0:r1] = (4.0 / (B * B)) * (W.sum(1, keepdim=True) * absX[r0:r1] + W @ absX)
    out = {"loss": loss / (B * B), "A": A / (B * B), "K": Kfull, "bandwidth": bw * kernel_mul ** (kernel_num // 2)}
    if want_grad:
        out.update(grad_source=grad[:B], grad_target=grad[B:], G_source=G[:B], G_target=G[B:])
    return out
