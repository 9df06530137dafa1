"""Dense CRF post-processing (reference utils/dcrf.py: `DenseCRF`, `crf_inference`, `crf_inference_label`) on the GPU.

The reference wraps the third-party pydensecrf (a permutohedral-lattice approximation).  By default this module runs the
EXACT mean-field inference of the same fully connected CRF with Potts compatibility in HIP (csrc/dcrf.hip, C ABI
`wc_dcrf_*`; model and error bound in DESIGN.md "Dense CRF" and include/weclip_hip.h).  `bilateral="lattice"` computes the
bilateral message on the permutohedral lattice instead (csrc/dcrf_lattice.hip, `wc_dcrf_lattice_*`; pinned to the fp64
restatement tests/dcrf_lattice_ref.py, deterministic, O(N d^2) per pass where the exact sum is O(N^2)); the Gaussian
term, the unaries and the update are the same.  Parity with pydensecrf itself is unpinned.

numpy inputs give numpy outputs, as the reference returns them; torch CUDA tensors stay on the device.  Importing needs
no GPU; calling without one raises RuntimeError (there is no CPU path)."""
import numpy as np
import torch

from .. import _lib as L

F32 = torch.float32


def _image(img, H=None, W=None):
    """(H,W,3) HWC uint8 or float -> contiguous CUDA tensor (uint8 or f32) and the is_u8 flag."""
    t = torch.as_tensor(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
    if t.dim() != 3 or t.shape[2] != 3:
        raise RuntimeError(f"dense CRF: image must be (H, W, 3), got {tuple(t.shape)}")
    if H is not None and tuple(t.shape[:2]) != (H, W):
        raise RuntimeError(f"dense CRF: image {tuple(t.shape[:2])} does not match the label grid {(H, W)}")
    if t.dtype != torch.uint8:
        t = t.to(F32)
    return t.cuda().contiguous(), 1 if t.dtype == torch.uint8 else 0


def _workspace(C, H, W, device):
    import ctypes
    n = ctypes.c_long()
    L.lib().wc_dcrf_workspace_floats(C, H, W, ctypes.byref(n))
    return torch.empty(n.value, device=device, dtype=F32)


def unary_from_prob(probs):
    """U (C,H,W) = -ln clamp(probs, 1e-5, 1) (pydensecrf.utils.unary_from_softmax with its default clip)."""
    L.require_gpu()
    p = probs.to(F32).contiguous()
    C, H, W = p.shape
    U = torch.empty_like(p)
    L.lib().wc_dcrf_unary_prob(L.ptr(p, F32, "probs"), L.ptr(U), C, H, W, L.stream())
    return U


def unary_from_labels(labels, n_labels, gt_prob):
    """U (n_labels,H,W): -ln gt_prob at the given label, -ln((1 - gt_prob) / (n_labels - 1)) elsewhere."""
    L.require_gpu()
    lab = labels.long().contiguous()
    H, W = lab.shape
    U = torch.empty(n_labels, H, W, device=lab.device, dtype=F32)
    L.lib().wc_dcrf_unary_label(L.ptr(lab, torch.int64, "labels"), L.ptr(U), n_labels, H, W, float(gt_prob), L.stream())
    return U


def unary_from_logits(logits, out_hw):
    """U (C,H,W) of softmax(F.interpolate(logits, out_hw, bilinear, align_corners=False)), without the resized logits."""
    L.require_gpu()
    lg = logits.to(F32).contiguous()
    C, h, w = lg.shape
    H, W = out_hw
    U = torch.empty(C, H, W, device=lg.device, dtype=F32)
    L.lib().wc_dcrf_unary_logits(L.ptr(lg, F32, "logits"), L.ptr(U), C, h, w, H, W, L.stream())
    return U


BILATERAL = ("exact", "lattice")


def _bilateral(mode):
    if mode not in BILATERAL:
        raise ValueError(f"dense CRF: bilateral must be one of {BILATERAL}, got {mode!r}")
    return mode


class _Lattice(object):
    """The built lattice of one image: the structure buffer, M (read once from the device, with the flag), and the value
    rows and workspace for C labels."""

    def __init__(self, image, C, H, W, bi_xy_std, bi_rgb_std):
        import ctypes
        img, is_u8 = _image(image, H, W)
        nl, nw = ctypes.c_long(), ctypes.c_long()
        L.lib().wc_dcrf_lattice_workspace_bytes(C, H, W, ctypes.byref(nl), ctypes.byref(nw))
        self.lat = torch.empty(nl.value, device=img.device, dtype=torch.uint8)
        L.lib().wc_dcrf_lattice_build(L.ptr(img), is_u8, L.ptr(self.lat), H, W, float(bi_xy_std), float(bi_rgb_std), L.stream())
        meta = self.lat[:12].view(torch.int32).cpu()                 # the one host read of a call: M and the flag
        self.M, flag = int(meta[0]), int(meta[1])
        if flag:
            raise RuntimeError("dense CRF (lattice): image colours outside 0..256" if flag == 1 else
                               "dense CRF (lattice): a vertex key left its packing")
        CP = 32 * ((C + 31) // 32)
        self.vals = torch.empty(2 * (self.M + 1) * CP, device=img.device, dtype=F32)
        self.ws = torch.empty(nw.value // 4, device=img.device, dtype=F32)


def lattice_filter(image, values, bi_xy_std, bi_rgb_std):
    """The un-normalised permutohedral-lattice filter of values (C,H,W) under the bilateral features of image (H,W,3)."""
    L.require_gpu()
    V = values.to(F32).contiguous()
    C, H, W = V.shape
    lt = _Lattice(image, C, H, W, bi_xy_std, bi_rgb_std)
    out = torch.empty_like(V)
    L.lib().wc_dcrf_lattice_filter(L.ptr(lt.lat), L.ptr(V, F32, "values"), L.ptr(out), L.ptr(lt.vals), L.ptr(lt.ws), C, H, W,
                                   lt.M, L.stream())
    return out


def inference(image, unary, iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std, bilateral="exact"):
    """Q (C,H,W) f32 on the device: `iter_max` mean-field updates from softmax(-unary)."""
    _bilateral(bilateral)
    L.require_gpu()
    U = unary.to(F32).contiguous()
    C, H, W = U.shape
    if bilateral == "lattice":
        Q = torch.empty_like(U)
        lt = _Lattice(image, C, H, W, bi_xy_std, bi_rgb_std)
        L.lib().wc_dcrf_lattice_inference(L.ptr(lt.lat), L.ptr(U, F32, "unary"), L.ptr(Q), L.ptr(lt.vals), L.ptr(lt.ws), C, H, W,
                                          lt.M, int(iter_max), float(pos_w), float(pos_xy_std), float(bi_w), L.stream())
        return Q
    img, is_u8 = _image(image, H, W)
    Q = torch.empty_like(U)
    ws = _workspace(C, H, W, U.device)
    L.lib().wc_dcrf_inference(L.ptr(img), is_u8, L.ptr(U, F32, "unary"), L.ptr(Q), L.ptr(ws), C, H, W, int(iter_max),
                              float(pos_w), float(pos_xy_std), float(bi_w), float(bi_xy_std), float(bi_rgb_std), L.stream())
    return Q


def message(image, Q, pos_xy_std, bi_xy_std, bi_rgb_std, bilateral="exact"):
    """One message pass for a given Q (C,H,W): (M_pos, M_bil) (C,H,W) = n(i) sum_j k(i,j) n(j) Q(:,j) and S (2,H,W)."""
    _bilateral(bilateral)
    L.require_gpu()
    Q = Q.to(F32).contiguous()
    C, H, W = Q.shape
    mp, mb = torch.empty_like(Q), torch.empty_like(Q)
    S = torch.empty(2, H, W, device=Q.device, dtype=F32)
    if bilateral == "lattice":
        lt = _Lattice(image, C, H, W, bi_xy_std, bi_rgb_std)
        L.lib().wc_dcrf_lattice_message(L.ptr(lt.lat), L.ptr(Q, F32, "Q"), L.ptr(mp), L.ptr(mb), L.ptr(S), L.ptr(lt.vals),
                                        L.ptr(lt.ws), C, H, W, lt.M, float(pos_xy_std), L.stream())
        return mp, mb, S
    img, is_u8 = _image(image, H, W)
    ws = _workspace(C, H, W, Q.device)
    L.lib().wc_dcrf_message(L.ptr(img), is_u8, L.ptr(Q, F32, "Q"), L.ptr(mp), L.ptr(mb), L.ptr(S), L.ptr(ws), C, H, W,
                            float(pos_xy_std), float(bi_xy_std), float(bi_rgb_std), L.stream())
    return mp, mb, S


def _as_device(x):
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda(), True
    return x, False


class DenseCRF(object):
    """reference utils/dcrf.py `DenseCRF`: __call__(image (H,W,3), probmap (C,H,W)) -> Q (C,H,W) float32."""

    def __init__(self, iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std, bilateral="exact"):
        self.bilateral = _bilateral(bilateral)
        self.iter_max = iter_max
        self.pos_w = pos_w
        self.pos_xy_std = pos_xy_std
        self.bi_w = bi_w
        self.bi_xy_std = bi_xy_std
        self.bi_rgb_std = bi_rgb_std

    def with_unary(self, image, unary, bilateral=None):
        """The same inference from a ready unary (C,H,W) CUDA tensor (e.g. unary_from_logits) -> Q on the device."""
        return inference(image, unary, self.iter_max, self.pos_w, self.pos_xy_std, self.bi_w, self.bi_xy_std, self.bi_rgb_std,
                         bilateral=self.bilateral if bilateral is None else bilateral)

    def __call__(self, image, probmap):
        L.require_gpu()
        P, host = _as_device(probmap)
        Q = self.with_unary(image, unary_from_prob(P))
        return Q.cpu().numpy() if host else Q


def crf_inference(img, probs, t=10, scale_factor=1, labels=21, bilateral="exact"):
    """reference crf_inference: Gaussian sxy = 3/scale_factor (w 3), bilateral sxy = 80/scale_factor, srgb = 13 (w 10)."""
    _bilateral(bilateral)
    L.require_gpu()
    P, host = _as_device(probs)
    P = P.reshape(labels, *P.shape[-2:])
    Q = inference(img, unary_from_prob(P), t, 3, 3 / scale_factor, 10, 80 / scale_factor, 13, bilateral=bilateral)
    return Q.cpu().numpy() if host else Q


def crf_inference_label(img, labels, t=10, n_labels=21, gt_prob=0.7, bilateral="exact"):
    """reference crf_inference_label: unary from a label map, Gaussian sxy = 3 (w 3), bilateral sxy = 50, srgb = 5 (w 10)
    -> argmax (H,W)."""
    _bilateral(bilateral)
    L.require_gpu()
    lab, host = _as_device(labels)
    Q = inference(img, unary_from_labels(lab, n_labels, gt_prob), t, 3, 3, 10, 50, 5, bilateral=bilateral)
    pred = Q.argmax(0)
    return pred.cpu().numpy() if host else pred
