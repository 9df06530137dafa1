"""PyTorch custom-op registration of the hot-path operators (`torch.ops.weclip.*`).

BASELINE.json's north star asks for the HIP kernels to be "exposed to Python through PyTorch-ROCm custom ops so
WeCLIP_model.* and the segformer_head keep their nn.Module API".  This module registers the operator-level entry
points of libweclip_hip.so with the PyTorch dispatcher (`torch.library.custom_op`, CUDA/HIP device only) together
with shape-propagating fake kernels, so the ops can be called as `torch.ops.weclip.<name>`, show up under their own
names in the PyTorch profiler and can be traced (`torch.export` / `make_fx`) like any ATen op.  The nn.Modules of
this package call them at module granularity (PAR.forward, compute_trans_mat, the fused losses' forward,
confusion_hist, ...); inside a block the engines keep talking to the C ABI directly (vit_engine / head_engine:
one Python frame per launch matters there).

There is NO CPU kernel: a CPU tensor raises NotImplementedError from the dispatcher (no backend registered),
which is the "fail loudly" contract of the package.
"""
from typing import List, Optional, Tuple

import torch
from torch import Tensor

F32 = torch.float32
_LIB = "weclip"


def _par_module(dilations, num_iter):
    from .WeCLIP_model.PAR import PAR
    key = (tuple(dilations), int(num_iter))
    m = _par_cache.get(key)
    if m is None:
        m = _par_cache[key] = PAR(list(dilations), int(num_iter))
    return m


_par_cache = {}


@torch.library.custom_op(f"{_LIB}::par_forward", mutates_args=(), device_types="cuda")
def par_forward(imgs: Tensor, masks: Tensor, dilations: List[int], num_iter: int) -> Tensor:
    """PAR.forward (reference WeCLIP_model/PAR.py:64-92): refined masks (b, C, H, W)."""
    return _par_module(dilations, num_iter)._forward_impl(imgs, masks)


@par_forward.register_fake
def _(imgs, masks, dilations, num_iter):
    return masks.new_empty(masks.shape, dtype=F32)


@torch.library.custom_op(f"{_LIB}::par_labels", mutates_args=(), device_types="cuda")
def par_labels(masks: Tensor, valid_key: Tensor) -> Tensor:
    """valid_key[argmax_c masks] (reference `_refine_cams`, model_attn_aff_voc.py:49-57) -> (B, H, W) int64."""
    from .WeCLIP_model.PAR import refine_labels
    return refine_labels(masks.float().contiguous(), valid_key.long().contiguous())


@par_labels.register_fake
def _(masks, valid_key):
    B, _, H, W = masks.shape
    return masks.new_empty((B, H, W), dtype=torch.int64)


@torch.library.custom_op(f"{_LIB}::trans_mat", mutates_args=(), device_types="cuda")
def trans_mat(attn_weight: Tensor) -> Tensor:
    """compute_trans_mat (reference clip/clip_tool.py:64-80) of a batch of (hw, hw) affinities."""
    from . import cam_pipeline as CP
    w = attn_weight.detach().float().contiguous()
    return CP.trans_mat(w if w.dim() == 3 else w[None]).view(attn_weight.shape)


@trans_mat.register_fake
def _(attn_weight):
    return attn_weight.new_empty(attn_weight.shape, dtype=F32)


@torch.library.custom_op(f"{_LIB}::attention", mutates_args=(), device_types="cuda")
def attention(qkv16: Tensor, B: int, L: int, H: int, DH: int, want_mean: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """Flash attention forward + head-mean probabilities (reference clip/myAtt.py:21-64, 325-326) on the packed fp16
    in-projection output (B*L, 3*H*DH), q pre-scaled by log2(e)/sqrt(DH).  -> (O fp16 (B*L, E), LSE (B,H,L),
    mean (B,L,L); a (0,) tensor when want_mean is False)."""
    from . import ops
    o16, lse, mean = ops.attention(qkv16, B, L, H, DH, want_mean=want_mean)
    return o16, lse, mean if mean is not None else qkv16.new_empty((0,), dtype=F32)


@attention.register_fake
def _(qkv16, B, L, H, DH, want_mean):
    return (qkv16.new_empty((B * L, H * DH)), qkv16.new_empty((B, H, L), dtype=F32),
            qkv16.new_empty((B, L, L) if want_mean else (0,), dtype=F32))


@torch.library.custom_op(f"{_LIB}::linear_f16", mutates_args=(), device_types="cuda")
def linear_f16(x16: Tensor, w16: Tensor, bias: Tensor, act: int) -> Tensor:
    """y = act(x W^T + b) on the MFMA path (F.linear call sites of the reference): x16 (M, K), w16 (N, K) fp16,
    bias (N,) f32, act 0 none / 1 QuickGELU / 2 ReLU / 3 sigmoid -> (M, N) f32.  K % 64 == 0."""
    from . import ops
    M, K = x16.shape
    N = w16.shape[0]
    out = torch.empty(M, N, device=x16.device, dtype=F32)
    ops.gemm(x16.contiguous(), w16.contiguous(), M, N, K, bias=bias.float().contiguous(), out32=out, act=act)
    return out


@linear_f16.register_fake
def _(x16, w16, bias, act):
    return x16.new_empty((x16.shape[0], w16.shape[0]), dtype=F32)


@torch.library.custom_op(f"{_LIB}::layernorm", mutates_args=(), device_types="cuda")
def layernorm(x: Tensor, weight: Tensor, bias: Tensor, eps: float) -> Tensor:
    """Row LayerNorm with fp32 statistics (reference clip/model.py:177-183) -> f32, same shape."""
    from . import ops
    y, _ = ops.layernorm(x.float().contiguous().view(-1, x.shape[-1]), weight.float().contiguous(), bias.float().contiguous(),
                         eps=eps, want32=True, want16=False)
    return y.view(x.shape)


@layernorm.register_fake
def _(x, weight, bias, eps):
    return x.new_empty(x.shape, dtype=F32)


@torch.library.custom_op(f"{_LIB}::bilinear_resize", mutates_args=(), device_types="cuda")
def bilinear_resize(x: Tensor, out_h: int, out_w: int, align_corners: bool) -> Tensor:
    """F.interpolate(x, (out_h, out_w), 'bilinear', align_corners) of (N, C, H, W) f32 planes."""
    from .resize import bilinear_resize as br
    return br(x.float().contiguous(), (out_h, out_w), align_corners=align_corners)


@bilinear_resize.register_fake
def _(x, out_h, out_w, align_corners):
    return x.new_empty(x.shape[:-2] + (out_h, out_w), dtype=F32)


@torch.library.custom_op(f"{_LIB}::confusion_hist", mutates_args=(), device_types="cuda")
def confusion_hist(label_true: Tensor, label_pred: Tensor, num_classes: int) -> Tensor:
    """_fast_hist (reference utils/evaluate.py:10-16) -> (nc, nc) int64."""
    from .utils.evaluate import confusion_hist as ch
    return ch(label_true, label_pred, num_classes)


@confusion_hist.register_fake
def _(label_true, label_pred, num_classes):
    return label_true.new_empty((num_classes, num_classes), dtype=torch.int64)


@torch.library.custom_op(f"{_LIB}::seg_loss", mutates_args=(), device_types="cuda")
def seg_loss(seg_lowres: Tensor, label: Tensor, ignore_index: int) -> Tensor:
    """get_seg_loss(F.interpolate(seg, label.shape[1:]), label) (reference scripts/dist_clip_voc.py:105-113,250), forward
    value only (the differentiable form is utils.losses.get_seg_loss_fused)."""
    from .utils.losses import get_seg_loss_fused
    return get_seg_loss_fused(seg_lowres.detach(), label, ignore_index).detach()


@seg_loss.register_fake
def _(seg_lowres, label, ignore_index):
    return seg_lowres.new_empty((), dtype=F32)


@torch.library.custom_op(f"{_LIB}::ce_loss", mutates_args=(), device_types="cuda")
def ce_loss(seg_lowres: Tensor, label: Tensor, ignore_index: int) -> Tensor:
    """F.cross_entropy(F.interpolate(seg, label.shape[1:], bilinear), label, ignore_index) (the supervised variant's loss),
    forward value only (the differentiable form is utils.losses.get_ce_loss_fused)."""
    from .utils.losses import get_ce_loss_fused
    return get_ce_loss_fused(seg_lowres.detach(), label, ignore_index).detach()


@ce_loss.register_fake
def _(seg_lowres, label, ignore_index):
    return seg_lowres.new_empty((), dtype=F32)


@torch.library.custom_op(f"{_LIB}::aff_loss", mutates_args=(), device_types="cuda")
def aff_loss(attn_pred: Tensor, cam_label: Tensor, radius: int, ignore_index: int) -> Tensor:
    """get_aff_loss(attn_pred, cams_to_affinity_label(cam_label, radius mask)) (reference utils/losses.py:11-22,
    utils/camutils.py:226-247), forward value only (differentiable form: utils.losses.get_aff_loss_fused)."""
    from .utils.losses import get_aff_loss_fused
    return get_aff_loss_fused(attn_pred.detach(), cam_label, radius, ignore_index).detach()


@aff_loss.register_fake
def _(attn_pred, cam_label, radius, ignore_index):
    return attn_pred.new_empty((), dtype=F32)


# ---------------------------------------------------------------------------------------------------------------------
# Trainable operators: forward and backward are both registered ops, tied together with `register_autograd`
# ("ops used by trainable modules need ... register_autograd backward").  hip_functional.linear /
# layer_norm -- the nn.Linear / 1x1 nn.Conv2d / nn.LayerNorm layers of the module-by-module ViT-CoMer form -- call these.
GRAD_SCALE = 4096.0


@torch.library.custom_op(f"{_LIB}::linear", mutates_args=(), device_types="cuda")
def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor], act: int) -> Tensor:
    """y = act(x W^T + b) for fp32 x (M, K), W (N, K) [or a 1x1 conv kernel (N, K, 1, 1)], b (N) or None on the MFMA path
    (fp16 operands [hi + lo in `exact` precision], fp32 accumulate).  act 0 none / 2 ReLU.  K % 64 == 0."""
    from . import config, ops
    x = x.detach().float().contiguous()
    M, K = x.shape
    N = weight.shape[0]
    if K % 64:
        raise RuntimeError(f"weclip::linear: K = {K} must be a multiple of 64")
    ex = config.exact()
    y = torch.empty(M, N, device=x.device, dtype=F32)
    ops.gemm(ops.split_f16(x, with_lo=ex), ops.split_f16(weight.detach().float().reshape(N, K).contiguous(), with_lo=ex), M, N, K,
             bias=bias.detach().float().contiguous() if bias is not None else None, out32=y, act=act)
    return y


@linear.register_fake
def _(x, weight, bias, act):
    return x.new_empty((x.shape[0], weight.shape[0]), dtype=F32)


@torch.library.custom_op(f"{_LIB}::linear_bwd", mutates_args=(), device_types="cuda")
def linear_bwd(dy: Tensor, x: Tensor, weight: Tensor, y: Tensor, act: int, need_dx: bool, need_dw: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """Gradients of weclip::linear: (dx (M, K), dW (N, K), db (N)); a (0,) tensor where not needed.  The input gradient is
    one MFMA GEMM against the transposed weight, the weight + bias gradients the split-K row-major GEMM (csrc/gemm.hip
    gemm_km_kernel, bias = extra output column); gradients travel multiplied by 2^12 so they sit in fp16's normal range."""
    from . import _lib as L
    from . import config, ops
    from .grad_sink import slices
    M, K = x.shape
    N = weight.shape[0]
    dev = dy.device
    ex = config.exact()
    dy = dy.float().contiguous()
    if act == 2:
        dy = dy * (y > 0)
    Np = (N + 63) // 64 * 64
    if Np != N:                                   # the contraction dimension of dX = dY W must be a multiple of 64
        pad = torch.zeros(M, Np, device=dev, dtype=F32)
        pad[:, :N] = dy
        dy = pad
    _, dS = ops.colscale_split(dy, None, M, alpha=GRAD_SCALE, want32=False, with_lo=ex)
    w2 = weight.detach().float().reshape(N, K).contiguous()
    # one placeholder PER slot: outputs of a custom op may not alias each other
    dx, dw, db = (torch.empty((0,), device=dev, dtype=F32) for _ in range(3))
    if need_dx:
        wT, Kp = ops.transpose_f16(w2, N, K, with_lo=ex)          # (K, Np) fp16: W^T with the N columns zero padded
        dx = torch.empty(M, K, device=dev, dtype=F32)
        ops.gemm(dS, wT, M, K, Kp, out32=dx, scale=1.0 / GRAD_SCALE, scale_cols=K)
    if need_dw:
        xhi = ops.split_f16(x.detach().float().contiguous()).hi
        part, ns = ops.wgrad_partials(dS.hi, xhi, M, N, K, lda=Np, slices=slices(M, ops.wgrad_tiles(N, K), 512), bias=True)
        dw = torch.empty(N, K, device=dev, dtype=F32)
        db = torch.empty(N, device=dev, dtype=F32)
        L.lib().wc_sum_slices_wb(L.ptr(part, F32), L.ptr(dw, F32), L.ptr(db, F32), ns, N, K, 1.0 / GRAD_SCALE, L.stream())
    return dx, dw, db


@linear_bwd.register_fake
def _(dy, x, weight, y, act, need_dx, need_dw):
    N, K = weight.shape[0], x.shape[1]
    def e():
        return dy.new_empty((0,), dtype=F32)
    return (x.new_empty(x.shape, dtype=F32) if need_dx else e(), x.new_empty((N, K), dtype=F32) if need_dw else e(),
            x.new_empty((N,), dtype=F32) if need_dw else e())


def _linear_setup(ctx, inputs, output):
    x, weight, bias, act = inputs
    ctx.save_for_backward(x, weight, output if act == 2 else None)
    ctx.act, ctx.has_bias, ctx.wshape = act, bias is not None, weight.shape


def _linear_backward(ctx, dy):
    x, weight, y = ctx.saved_tensors
    need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
    dx, dw, db = torch.ops.weclip.linear_bwd(dy, x, weight, y if y is not None else dy.new_empty((0,)), ctx.act, need_dx, need_dw)
    return (dx if need_dx else None, dw.view(ctx.wshape) if need_dw else None, db if (need_dw and ctx.has_bias) else None, None)


torch.library.register_autograd(f"{_LIB}::linear", _linear_backward, setup_context=_linear_setup)


@torch.library.custom_op(f"{_LIB}::layer_norm", mutates_args=(), device_types="cuda")
def layer_norm(x: Tensor, weight: Tensor, bias: Tensor, eps: float) -> Tensor:
    """Row LayerNorm (fp32 statistics, reference clip/model.py:177-183) of x (rows, D) -> f32; differentiable
    (weclip::layer_norm_bwd through register_autograd)."""
    from . import ops
    y, _ = ops.layernorm(x.detach().float().contiguous(), weight.detach().float().contiguous(), bias.detach().float().contiguous(),
                         eps=eps, want32=True, want16=False)
    return y


@layer_norm.register_fake
def _(x, weight, bias, eps):
    return x.new_empty(x.shape, dtype=F32)


@torch.library.custom_op(f"{_LIB}::layer_norm_bwd", mutates_args=(), device_types="cuda")
def layer_norm_bwd(dy: Tensor, x: Tensor, weight: Tensor, eps: float) -> Tuple[Tensor, Tensor, Tensor]:
    """(dx, dgamma, dbeta) of weclip::layer_norm (csrc/train_ops.hip ln_bwd, fixed-order column reductions)."""
    from . import ops
    dx, _, dgb = ops.layernorm_bwd(dy.float().contiguous(), x.detach().float().contiguous(), weight.detach().float().contiguous(),
                                   want32=True, eps=eps)
    return dx, dgb[0].clone(), dgb[1].clone()


@layer_norm_bwd.register_fake
def _(dy, x, weight, eps):
    return x.new_empty(x.shape, dtype=F32), weight.new_empty(weight.shape, dtype=F32), weight.new_empty(weight.shape, dtype=F32)


def _ln_setup(ctx, inputs, output):
    x, weight, bias, eps = inputs
    ctx.save_for_backward(x, weight)
    ctx.eps = eps


def _ln_backward(ctx, dy):
    x, weight = ctx.saved_tensors
    dx, dg, db = torch.ops.weclip.layer_norm_bwd(dy, x, weight, ctx.eps)
    return dx, dg, db, None


torch.library.register_autograd(f"{_LIB}::layer_norm", _ln_backward, setup_context=_ln_setup)


@torch.library.custom_op(f"{_LIB}::dense_crf", mutates_args=(), device_types="cuda")
def dense_crf(image: Tensor, probs: Tensor, iter_max: int, pos_w: float, pos_xy_std: float, bi_w: float, bi_xy_std: float,
              bi_rgb_std: float) -> Tensor:
    """DenseCRF(iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std)(image, probs) (reference utils/dcrf.py) as the
    exact mean-field inference: image (H,W,3) uint8 / float, probs (C,H,W) -> Q (C,H,W) f32.  No autograd."""
    from .utils import dcrf
    return dcrf.inference(image, dcrf.unary_from_prob(probs), iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std)


@dense_crf.register_fake
def _(image, probs, iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std):
    return probs.new_empty(probs.shape, dtype=F32)


@torch.library.custom_op(f"{_LIB}::dense_crf_lattice", mutates_args=(), device_types="cuda")
def dense_crf_lattice(image: Tensor, probs: Tensor, iter_max: int, pos_w: float, pos_xy_std: float, bi_w: float,
                      bi_xy_std: float, bi_rgb_std: float) -> Tensor:
    """dense_crf with the bilateral message filtered on the permutohedral lattice (DenseCRF(..., bilateral="lattice")).
    No autograd."""
    from .utils import dcrf
    return dcrf.inference(image, dcrf.unary_from_prob(probs), iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std,
                          bilateral="lattice")


@dense_crf_lattice.register_fake
def _(image, probs, iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std):
    return probs.new_empty(probs.shape, dtype=F32)


@torch.library.custom_op(f"{_LIB}::encode_text", mutates_args=(), device_types="cuda")
def encode_text(text: Tensor, token_embedding: Tensor, positional_embedding: Tensor, blocks: List[Tensor], heads: int,
                ln_final_weight: Tensor, ln_final_bias: Tensor, text_projection: Tensor) -> Tensor:
    """CLIP.encode_text (reference clip/model.py:392-405) from the text tower's tensors: text (N, Lctx) int32 / int64 ids,
    blocks = 12 tensors per residual block in clip.text_engine.BLOCK_KEYS order -> (N, Ed) f32.  No autograd."""
    from .clip import text_engine as TE
    dev = token_embedding.device
    f = lambda t: t.detach().float().contiguous()
    with torch.no_grad():
        return TE.run(TE._ids(text, dev), f(token_embedding), f(positional_embedding), TE.packs_from_tensors(list(blocks), heads),
                      f(ln_final_weight), f(ln_final_bias), f(text_projection))


@encode_text.register_fake
def _(text, token_embedding, positional_embedding, blocks, heads, ln_final_weight, ln_final_bias, text_projection):
    return text_projection.new_empty((text.shape[0], text_projection.shape[1]), dtype=F32)


@torch.library.custom_op(f"{_LIB}::bilateral_filter_batch", mutates_args=(), device_types="cuda")
def bilateral_filter_batch(images: Tensor, segs: Tensor, sigma_rgb: float, sigma_xy: float) -> Tensor:
    """The exact batched bilateral filter behind the dense energy loss (reference utils/losses.py:75): images (N,3,H,W) on the
    0..255 scale, segs (N,K,H,W) -> AS (N,K,H,W) f32.  No autograd."""
    from .utils.losses import bilateral_filter_batch as bf
    return bf(images, segs, sigma_rgb, sigma_xy)


@bilateral_filter_batch.register_fake
def _(images, segs, sigma_rgb, sigma_xy):
    return segs.new_empty(segs.shape, dtype=F32)


@torch.library.custom_op(f"{_LIB}::dense_energy", mutates_args=(), device_types="cuda")
def dense_energy(images: Tensor, segmentations: Tensor, rois: Tensor, unlabel_region: Tensor, sigma_rgb: float,
                 sigma_xy: float) -> Tuple[Tensor, Tensor]:
    """DenseEnergyLossFunction.forward (reference utils/losses.py:55-84) -> (loss (1,), A (N,K,H,W) = Gate * AS).  Differentiable
    in `segmentations` through weclip::dense_energy_bwd (register_autograd); the gradient arriving at A is ignored, as the
    reference's backward sees the loss alone."""
    from .utils.losses import dense_energy_forward
    loss, A, _ = dense_energy_forward(images, segmentations, sigma_rgb, sigma_xy, rois, unlabel_region)
    return loss, A


@dense_energy.register_fake
def _(images, segmentations, rois, unlabel_region, sigma_rgb, sigma_xy):
    return segmentations.new_empty((1,), dtype=F32), segmentations.new_empty(segmentations.shape, dtype=F32)


@torch.library.custom_op(f"{_LIB}::dense_energy_bwd", mutates_args=(), device_types="cuda")
def dense_energy_bwd(grad_loss: Tensor, A: Tensor, rois: Tensor) -> Tensor:
    """Gradient of weclip::dense_energy with respect to the segmentations: -2 * grad_loss * A * ROI / N (reference
    utils/losses.py:87-91; csrc/energy.hip energy_bwd_kernel)."""
    from .utils.losses import dense_energy_backward
    return dense_energy_backward(grad_loss, A, rois)


@dense_energy_bwd.register_fake
def _(grad_loss, A, rois):
    return A.new_empty(A.shape, dtype=F32)


def _energy_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1], inputs[2])


def _energy_backward(ctx, grad_loss, grad_A):
    A, rois = ctx.saved_tensors
    return None, torch.ops.weclip.dense_energy_bwd(grad_loss, A, rois), None, None, None, None


torch.library.register_autograd(f"{_LIB}::dense_energy", _energy_backward, setup_context=_energy_setup)


@torch.library.custom_op(f"{_LIB}::energy_term", mutates_args=(), device_types="cuda")
def energy_term(img: Tensor, seg_lowres: Tensor, label: Tensor, img_box: Optional[Tensor], weight: float, sigma_rgb: float,
                sigma_xy: float, scale_factor: float, mean: List[float], std: List[float]) -> Tuple[Tensor, Tensor]:
    """utils.losses.get_energy_loss_fused (csrc/energy_prep.hip around the filter of csrc/energy.hip): the dense energy loss of
    the bilinearly up-sampled logits at scale_factor 1, 0.5 or 0.25 -> (weight * loss (1,), d(weight * loss) / d seg_lowres
    (N,K,h,w) for an upstream gradient of 1).  Differentiable in `seg_lowres` (register_autograd scales the second output; the
    gradient arriving at it is ignored); img_box (N,4) integer rows (y0, y1, x0, x1) on the device, or None."""
    from .utils.losses import energy_term as term
    return term(img, seg_lowres, label, img_box, weight, sigma_rgb, sigma_xy, scale_factor, list(mean), list(std))


@energy_term.register_fake
def _(img, seg_lowres, label, img_box, weight, sigma_rgb, sigma_xy, scale_factor, mean, std):
    return seg_lowres.new_empty((1,), dtype=F32), seg_lowres.new_empty(seg_lowres.shape, dtype=F32)


def _energy_term_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _energy_term_backward(ctx, grad_loss, grad_grad):
    (grad,) = ctx.saved_tensors
    return (None, grad * grad_loss) + (None,) * 8


torch.library.register_autograd(f"{_LIB}::energy_term", _energy_term_backward, setup_context=_energy_term_setup)


@torch.library.custom_op(f"{_LIB}::dense_energy_lattice", mutates_args=(), device_types="cuda")
def dense_energy_lattice(images: Tensor, segmentations: Tensor, rois: Tensor, unlabel_region: Tensor, sigma_rgb: float,
                         sigma_xy: float) -> Tuple[Tensor, Tensor]:
    """weclip::dense_energy with the permutohedral lattice as the bilateral filter (csrc/energy_lattice.hip, DESIGN.md section
    15.3; opt-in, about half the exact AS) -> (loss (1,), A (N,K,H,W) = Gate * AS).  Differentiable in `segmentations` through the
    same weclip::dense_energy_bwd."""
    from .utils.losses import dense_energy_forward
    loss, A, _ = dense_energy_forward(images, segmentations, sigma_rgb, sigma_xy, rois, unlabel_region, "lattice")
    return loss, A


@dense_energy_lattice.register_fake
def _(images, segmentations, rois, unlabel_region, sigma_rgb, sigma_xy):
    return segmentations.new_empty((1,), dtype=F32), segmentations.new_empty(segmentations.shape, dtype=F32)


torch.library.register_autograd(f"{_LIB}::dense_energy_lattice", _energy_backward, setup_context=_energy_setup)


@torch.library.custom_op(f"{_LIB}::energy_term_lattice", mutates_args=(), device_types="cuda")
def energy_term_lattice(img: Tensor, seg_lowres: Tensor, label: Tensor, img_box: Optional[Tensor], weight: float, sigma_rgb: float,
                        sigma_xy: float, scale_factor: float, mean: List[float], std: List[float]) -> Tuple[Tensor, Tensor]:
    """weclip::energy_term with the permutohedral lattice as the bilateral filter (csrc/energy_lattice.hip): same arguments, same
    outputs, same autograd."""
    from .utils.losses import energy_term as term
    return term(img, seg_lowres, label, img_box, weight, sigma_rgb, sigma_xy, scale_factor, list(mean), list(std), bilateral="lattice")


@energy_term_lattice.register_fake
def _(img, seg_lowres, label, img_box, weight, sigma_rgb, sigma_xy, scale_factor, mean, std):
    return seg_lowres.new_empty((1,), dtype=F32), seg_lowres.new_empty(seg_lowres.shape, dtype=F32)


torch.library.register_autograd(f"{_LIB}::energy_term_lattice", _energy_term_backward, setup_context=_energy_term_setup)


@torch.library.custom_op(f"{_LIB}::aff_propagate", mutates_args=(), device_types="cuda")
def aff_propagate(aff: Tensor, cams: Tensor, mask: Optional[Tensor], cls: Optional[Tensor], bkg_score: float,
                  with_bkg: bool) -> Tensor:
    """The random walk of the CAMs over the learned affinity (reference utils/camutils.py:249-317; csrc/camlabel.hip): aff
    (B,n,n), cams (B,C,n), mask (n,n) or None, cls (B,C) (needed with with_bkg) -> (B,C+with_bkg,n) f32.  `aff` is not modified.
    No autograd: the reference detaches."""
    from .utils.camutils import _aff_propagate as walk
    return walk(aff, cams, mask, cls, bkg_score, with_bkg)


@aff_propagate.register_fake
def _(aff, cams, mask, cls, bkg_score, with_bkg):
    return cams.new_empty((cams.shape[0], cams.shape[1] + (1 if with_bkg else 0), cams.shape[2]), dtype=F32)


@torch.library.custom_op(f"{_LIB}::panel_images", mutates_args=(), device_types="cuda")
def panel_images(imgs: Tensor, cam: Tensor) -> Tuple[Tensor, Tensor]:
    """tensorboard_image (reference utils/imutils.py:26-40; csrc/panels.hip): imgs (B,3,H,W) normalised, cam (B,C,h,w) -> the
    nrow=2 grids of the de-normalised images and of their jet overlay with max_c bilinear(cam), uint8 CHW."""
    from .utils import panels
    return panels.tensorboard_image(imgs, cam)


@panel_images.register_fake
def _(imgs, cam):
    from .utils.panels import grid_geometry
    g = grid_geometry(imgs.shape[0], imgs.shape[2], imgs.shape[3], 2)
    return (imgs.new_empty((3, g.canvas_h, g.canvas_w), dtype=torch.uint8), imgs.new_empty((3, g.canvas_h, g.canvas_w), dtype=torch.uint8))


@torch.library.custom_op(f"{_LIB}::panel_labels", mutates_args=(), device_types="cuda")
def panel_labels(labels: Tensor) -> Tensor:
    """tensorboard_label (reference utils/imutils.py:125-133; csrc/panels.hip): labels (B,H,W) int64 / uint8 -> the nrow=2 grid of
    their PASCAL VOC colours, uint8 CHW (B = 1: the bare (3,H,W) image)."""
    from .utils import panels
    if labels.dim() != 3:
        raise RuntimeError("panel_labels: labels must be (B, H, W)")
    geo = panels.grid_geometry(labels.shape[0], labels.shape[1], labels.shape[2], 2)
    lab = labels if labels.dtype in (torch.int64, torch.uint8) else labels.long()
    return panels.paint_labels(lab.contiguous(), panels._canvas(geo, labels.device), geo)


@panel_labels.register_fake
def _(labels):
    from .utils.panels import grid_geometry
    g = grid_geometry(labels.shape[0], labels.shape[1], labels.shape[2], 2)
    return labels.new_empty((3, g.canvas_h, g.canvas_w), dtype=torch.uint8)


@torch.library.custom_op(f"{_LIB}::panel_attn", mutates_args=(), device_types="cuda")
def panel_attn(attns: List[Tensor], size: List[int], n_pix: float, n_row: int) -> Tensor:
    """tensorboard_attn (reference utils/imutils.py:54-85; csrc/panels.hip): a list of (b,hw,hw) maps -> the viridis grid of
    their rows int(h * n_pix) * (w + 1), up-sampled (align_corners=True) to `size` and min-max normalised per image."""
    from .utils import panels
    return panels.tensorboard_attn(attns, size=list(size), n_pix=n_pix, n_row=n_row)


@panel_attn.register_fake
def _(attns, size, n_pix, n_row):
    from .utils.panels import grid_geometry
    g = grid_geometry(sum(a.shape[0] for a in attns), size[0], size[1], n_row, colmajor=True)
    return attns[0].new_empty((3, g.canvas_h, g.canvas_w), dtype=torch.uint8)



@torch.library.custom_op(f"{_LIB}::mmd_rbf", mutates_args=(), device_types="cuda")
def mmd_rbf(source: Tensor, target: Tensor, kernel_mul: float, kernel_num: int, fix_sigma: float,
            need_grad: bool) -> Tuple[Tensor, Tensor]:
    """utils.mmdloss.mmd_rbf (reference utils/mmdloss.py:38-59; csrc/mmd.hip): source, target (B, d) f32 or fp16 ->
    (loss () f32, d loss / d cat(source, target) (2B, d) f32 for an upstream gradient of 1; (0, d) without need_grad).
    fix_sigma 0.0: bandwidth from the data, on the device.  Differentiable in both inputs (register_autograd scales the second
    output and casts it to the inputs' dtype; the gradient arriving at it is ignored)."""
    from . import ops
    loss, grad = ops.mmd_rbf(source, target, kernel_mul, kernel_num, fix_sigma, need_grad)
    return loss, grad if grad is not None else source.new_empty((0, source.shape[1]), dtype=F32)


@mmd_rbf.register_fake
def _(source, target, kernel_mul, kernel_num, fix_sigma, need_grad):
    B, d = source.shape
    return source.new_empty((), dtype=F32), source.new_empty((2 * B if need_grad else 0, d), dtype=F32)


def _mmd_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.rows, ctx.dtype = inputs[0].shape[0], inputs[0].dtype


def _mmd_backward(ctx, grad_loss, grad_grad):
    (grad,) = ctx.saved_tensors
    if grad.shape[0] != 2 * ctx.rows:
        raise RuntimeError("weclip::mmd_rbf was called with need_grad=False: it kept no gradient")
    B = ctx.rows
    gs = (grad[:B] * grad_loss).to(ctx.dtype) if ctx.needs_input_grad[0] else None
    gt = (grad[B:] * grad_loss).to(ctx.dtype) if ctx.needs_input_grad[1] else None
    return gs, gt, None, None, None, None


torch.library.register_autograd(f"{_LIB}::mmd_rbf", _mmd_backward, setup_context=_mmd_setup)


@torch.library.custom_op(f"{_LIB}::rbf_kernel", mutates_args=(), device_types="cuda")
def rbf_kernel(source: Tensor, target: Tensor, kernel_mul: float, kernel_num: int, fix_sigma: float) -> Tensor:
    """utils.mmdloss.rbf_kernel (reference utils/mmdloss.py:4-35; csrc/mmd.hip): the (2B, 2B) f32 multi-bandwidth kernel matrix
    of cat(source, target), symmetric bit for bit.  No autograd."""
    from . import ops
    return ops.mmd_rbf_kernel(source, target, kernel_mul, kernel_num, fix_sigma)


@rbf_kernel.register_fake
def _(source, target, kernel_mul, kernel_num, fix_sigma):
    N = 2 * source.shape[0]
    return source.new_empty((N, N), dtype=F32)



@torch.library.custom_op(f"{_LIB}::cam_seed_sweep", mutates_args=(), device_types="cuda")
def cam_seed_sweep(cams: Tensor, first: Tensor, keys: Tensor, gt: Tensor, thresholds: List[float], num_classes: int,
                   kmax: int) -> Tensor:
    """The background-threshold sweep of `_fast_hist(gt, cam_to_label(cam))` (reference utils/camutils.py:8-16,
    utils/evaluate.py:9-16; csrc/camseed.hip) in one pass: cams (P, HW) fp16, first (B+1) / keys (P) int32 device tables, gt
    (B, HW) uint8, T ascending thresholds, kmax >= the most pairs of an image -> bins (nc, nc, T+1) int64 counts over
    (gt, class, number of thresholds below the pixel's maximum); clip.cam_seeds.confusion_from_bins turns them into the T
    confusion matrices.  The tables are device tensors here, so a class id outside [0, nc - 1) is skipped and raises the device
    flag of clip.cam_seeds.check_tables_in_range instead of a host error."""
    from .clip import cam_seeds as CS
    t = CS.PairTables.from_device(num_classes, first, keys, Kmax=kmax)
    return CS.sweep_bins(cams, None, gt, list(thresholds), num_classes, tables=t)


@cam_seed_sweep.register_fake
def _(cams, first, keys, gt, thresholds, num_classes, kmax):
    return cams.new_empty((num_classes, num_classes, len(thresholds) + 1), dtype=torch.int64)


@torch.library.custom_op(f"{_LIB}::cam_seed_labels", mutates_args=(), device_types="cuda")
def cam_seed_labels(cams: Tensor, first: Tensor, keys: Tensor, low_thre: float, high_thre: float) -> Tuple[Tensor, Tensor]:
    """The two slot maps of the per-image body of cam_to_fg_bg_label (reference utils/camutils.py:55-65; csrc/camseed.hip) at the
    image's own size: cams (P, HW) fp16, first (B+1) / keys (P) int32 -> (lab_low, lab_high) (B, HW) int64, slot 1 + rank of
    the winning class among the image's ids where the maximum exceeds the threshold, else 0."""
    from .clip import cam_seeds as CS
    return CS.seed_labels(cams, None, low_thre, high_thre, tables=CS.PairTables.from_device(CS.MAX_CLASSES, first, keys))


@cam_seed_labels.register_fake
def _(cams, first, keys, low_thre, high_thre):
    B = first.shape[0] - 1
    return cams.new_empty((B, cams.shape[1]), dtype=torch.int64), cams.new_empty((B, cams.shape[1]), dtype=torch.int64)


@torch.library.custom_op(f"{_LIB}::cam_seed_merge", mutates_args=(), device_types="cuda")
def cam_seed_merge(lab_low: Tensor, lab_high: Tensor, slot_class: Tensor, gt: Optional[Tensor],
                   num_classes: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The merge of cam_to_fg_bg_label (reference utils/camutils.py:77-79) + the `pseudo_scores` histogram
    (utils/evaluate.py:38-45) + the VOC colour image for the B images of a bucket in one launch (csrc/camseed.hip): slot maps
    (B, HW) int64, slot_class (B, S) int32, gt (B, HW) uint8 or None -> (label (B, HW) uint8, cmap (B, HW, 3) uint8, hist
    (nc, nc) int64, cover int64[2] = [labelled pixels with gt < nc, pixels with gt < nc]; zeros without gt)."""
    from .clip import cam_seeds as CS
    t = CS.PairTables.from_device(num_classes, slot_class=slot_class)
    label, cmap, hist, cover = CS.merge_labels(lab_low, lab_high, None, num_classes, gt=gt, want_cmap=True, tables=t)
    if hist is None:
        hist = lab_high.new_zeros((num_classes, num_classes))
        cover = lab_high.new_zeros((2,))
    return label, cmap, hist, cover


@cam_seed_merge.register_fake
def _(lab_low, lab_high, slot_class, gt, num_classes):
    return (lab_high.new_empty(lab_high.shape, dtype=torch.uint8), lab_high.new_empty(tuple(lab_high.shape) + (3,), dtype=torch.uint8),
            lab_high.new_empty((num_classes, num_classes)), lab_high.new_empty((2,)))


@torch.library.custom_op(f"{_LIB}::predict_finish", mutates_args=(), device_types="cuda")
def predict_finish(src: Tensor, image: Optional[Tensor], out_h: int, out_w: int, mode: int, alpha256: int,
                   ignore_below: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The per-image tail of the predict entry point in one launch (csrc/predict.hip; reference test_msc_flip_voc.py:92-96,
    :146-161, utils/imutils.py:136-154): src (C, Hs, Ws) f32 logits (mode 0) or probabilities on the output grid (mode 1), image
    (H, W, 3) uint8 or None -> (label (H, W) uint8 with 255 where the confidence is below ignore_below, its colour image (H, W, 3)
    uint8, confidence (H, W) uint8, overlay (H, W, 3) uint8 -- zeros without an image --, stats int64[2C + 1] = per label the
    pixel count, per label the confidence sum, the ignored pixels).  No autograd: every output is an integer map."""
    from . import predict as P
    C = src.shape[0]
    u8 = lambda *shape: torch.empty(shape, device=src.device, dtype=torch.uint8)      # noqa: E731
    pred, cmap, conf = u8(out_h, out_w), u8(out_h, out_w, 3), u8(out_h, out_w)
    overlay = u8(out_h, out_w, 3) if image is not None else torch.zeros(out_h, out_w, 3, device=src.device, dtype=torch.uint8)
    stats = torch.zeros(2 * C + 1, device=src.device, dtype=torch.int64)
    P.predict_finish(src, (out_h, out_w), image=image, pred_u8=pred, cmap_rgb=cmap, conf_u8=conf,
                     overlay_rgb=overlay if image is not None else None, stats=stats, mode=mode, alpha256=alpha256,
                     ignore_below=ignore_below)
    return pred, cmap, conf, overlay, stats


@predict_finish.register_fake
def _(src, image, out_h, out_w, mode, alpha256, ignore_below):
    u8 = lambda *shape: src.new_empty(shape, dtype=torch.uint8)                        # noqa: E731
    return (u8(out_h, out_w), u8(out_h, out_w, 3), u8(out_h, out_w), u8(out_h, out_w, 3),
            src.new_empty((2 * src.shape[0] + 1,), dtype=torch.int64))


OPS = ("par_forward", "par_labels", "trans_mat", "attention", "linear_f16", "layernorm", "bilinear_resize", "confusion_hist",
       "seg_loss", "ce_loss", "aff_loss", "linear", "linear_bwd", "layer_norm", "layer_norm_bwd", "dense_crf", "encode_text",
       "bilateral_filter_batch", "dense_energy", "dense_energy_bwd", "energy_term", "aff_propagate",
       "panel_images", "panel_labels", "panel_attn", "dense_crf_lattice", "dense_energy_lattice", "energy_term_lattice",
       "mmd_rbf", "rbf_kernel", "cam_seed_sweep", "cam_seed_labels", "cam_seed_merge", "predict_finish")
