"""The reference's utils/imutils.py on the device: the tensorboard image panels of a training run as uint8 CHW grids.

    from weclip_vit_comer_amd.utils import panels as imutils

Same function names, arguments and defaults as the reference module; tensors stay on the GPU and every function returns a
device uint8 grid (the reference returns host tensors).  The kernels of csrc/panels.hip paint each tile straight into the
canvas `torchvision.utils.make_grid(nrow, padding=2, pad_value=0)` would assemble; neither torchvision nor matplotlib is
imported (the jet / viridis tables are compiled in, csrc/cmap_tables.h).  A CPU tensor raises, as everywhere in this package;
`encode_cmap` and `colormap` are the reference's numpy helpers and stay on the host.

Beyond the reference: `tensorboard_label` also takes a batch (B, H, W) and then returns the nrow=2 grid of its B maps (the
reference handles one map and fails on a batch).

The module is NOT named utils/imutils.py: `utils.imutils` keeps resolving to the user's reference checkout.
"""
import collections
import ctypes

import numpy as np
import torch

from .. import _lib as L

F32 = torch.float32
U8 = torch.uint8
MEAN = [123.675, 116.28, 103.53]
STD = [58.395, 57.12, 57.375]
N_PIXS = [0.0, 0.3, 0.6, 0.9]
JET, VIRIDIS = 0, 1

Geometry = collections.namedtuple("Geometry", "canvas_h canvas_w oy ox xmaps pad colmajor")


def grid_geometry(B, H, W, nrow, padding=2, colmajor=False):
    """Where `torchvision.utils.make_grid(nrow=nrow, padding=padding)` puts B tiles of (H, W): xmaps = min(nrow, B) tiles per
    row, ymaps = ceil(B / xmaps) rows, tile k at (y * (H + padding) + padding, x * (W + padding) + padding), canvas
    (3, (H + padding) * ymaps + padding, (W + padding) * xmaps + padding); B == 1 is the bare image.  colmajor (the grid of
    `tensorboard_attn`, whose tiles are transposed before make_grid and whose grid is transposed after it): tile k sits in
    row k % xmaps and column k // xmaps, and the canvas has xmaps tile rows and ymaps tile columns."""
    B, H, W, nrow, padding = int(B), int(H), int(W), int(nrow), int(padding)
    if B < 1 or H < 1 or W < 1 or nrow < 1 or padding < 0:
        raise ValueError(f"grid_geometry: bad sizes B={B} H={H} W={W} nrow={nrow} padding={padding}")
    if B == 1:
        return Geometry(H, W, 0, 0, 1, 0, bool(colmajor))
    xmaps = min(nrow, B)
    ymaps = -(-B // xmaps)
    rows, cols = (xmaps, ymaps) if colmajor else (ymaps, xmaps)
    return Geometry((H + padding) * rows + padding, (W + padding) * cols + padding, padding, padding, xmaps, padding, bool(colmajor))


def _canvas(geo, device, out=None):
    """A zeroed (3, canvas_h, canvas_w) uint8 canvas, or `out` (the caller's, already zeroed where it must be)."""
    if out is None:
        return torch.zeros(3, geo.canvas_h, geo.canvas_w, device=device, dtype=U8)
    if out.dtype != U8 or tuple(out.shape) != (3, geo.canvas_h, geo.canvas_w):
        raise RuntimeError(f"panels: out must be uint8 (3, {geo.canvas_h}, {geo.canvas_w}), got {out.dtype} {tuple(out.shape)}")
    return out


def _f3(v):
    if len(v) != 3:
        raise ValueError("panels: mean / std need 3 values")
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def _geo_args(out, geo, k0=0):
    return (L.ptr(out, U8, "out"), out.shape[1], out.shape[2], geo.oy, geo.ox, geo.xmaps, geo.pad, int(geo.colmajor), int(k0), L.stream())


def _images4(imgs, name):
    if not isinstance(imgs, torch.Tensor) or imgs.dim() != 4 or imgs.shape[1] != 3:
        raise RuntimeError(f"{name}: imgs must be a (B, 3, H, W) tensor")
    return imgs.detach().float().contiguous()


def paint_images(imgs, out, geo, mean=MEAN, std=STD):
    """`wc_panel_images`: the de-normalised images (B,3,H,W) as tiles of the canvas `out` at `geo`."""
    L.require_gpu()
    B, _, H, W = imgs.shape
    L.lib().wc_panel_images(L.ptr(imgs, F32, "imgs"), _f3(mean), _f3(std), B, H, W, *_geo_args(out, geo))
    return out


def paint_labels(labels, out, geo):
    """`wc_panel_labels`: int64 or uint8 labels (B,H,W) as VOC-coloured tiles of the canvas `out` at `geo`."""
    L.require_gpu()
    if labels.dtype not in (torch.int64, U8):
        raise RuntimeError(f"panels: labels must be int64 or uint8, got {labels.dtype}")
    B, H, W = labels.shape
    L.lib().wc_panel_labels(L.ptr(labels, labels.dtype, "labels"), int(labels.dtype == U8), B, H, W, *_geo_args(out, geo))
    return out


def paint_heat(src, C, hw, size, out, geo, cmap, aligned=False, normalise=False, imgs=None, k0=0, mean=MEAN, std=STD):
    """`wc_panel_heat`: src = a float32 device tensor whose dim 0 is the image and whose LAST dims hold C maps of hw = (h, w)
    contiguously (dim 0 may be strided: a row view of an attention map is taken as it is); tiles k0, k0 + 1, ... of `out`."""
    L.require_gpu()
    h, w = hw
    B = src.shape[0]
    if src.dtype != F32 or not src.is_cuda:
        raise RuntimeError("panels: expected a float32 CUDA tensor")
    inner = src[0]
    if inner.numel() != C * h * w or not inner.is_contiguous() or (B > 1 and src.stride(0) < 0):
        raise RuntimeError(f"panels: every image must hold {C} contiguous maps of {h} x {w}")
    mm = torch.empty(3 * B, device=src.device, dtype=F32) if normalise else None
    L.lib().wc_panel_heat(ctypes.c_void_p(src.data_ptr()), src.stride(0) if B > 1 else 0, h * w, int(C), h, w, int(bool(aligned)),
                          L.ptr(mm, F32, "minmax"), int(cmap), L.ptr(imgs, F32, "imgs"), _f3(mean), _f3(std), B, int(size[0]),
                          int(size[1]), *_geo_args(out, geo, k0))
    return out


# ---------------------------------------------------------------------------------------------- the reference's names
def encode_cmap(label):
    """utils/imutils.py:7-9 (numpy, host): label array -> (..., 3) uint8 colours; labels are read as int16, as there."""
    return colormap()[np.asarray(label).astype(np.int16)]


def colormap(N=256, normalized=False):
    """utils/imutils.py:136-154: the PASCAL VOC label colours (numpy, host)."""
    v = np.arange(N, dtype=np.int64)
    cmap = np.zeros((N, 3), dtype=np.int64)
    for j in range(8):
        for ch in range(3):
            cmap[:, ch] |= ((v >> ch) & 1) << (7 - j)
        v = v >> 3
    return cmap.astype("float32") / 255 if normalized else cmap.astype("uint8")


def denormalize_img(imgs=None, mean=MEAN, std=STD):
    """utils/imutils.py:11-18: (B,3,H,W) normalised float images -> uint8 (B,3,H,W), x * std + mean truncated toward zero."""
    imgs = _images4(imgs, "denormalize_img")
    B, _, H, W = imgs.shape
    out = torch.empty(B, 3, H, W, device=imgs.device, dtype=U8)
    one = Geometry(H, W, 0, 0, 1, 0, False)
    for b in range(B):                                   # a (3,H,W) canvas per image: the batch layout is not a grid
        paint_images(imgs[b:b + 1], out[b], one, mean, std)
    return out


def denormalize_img2(imgs=None):
    """utils/imutils.py:20-24."""
    return denormalize_img(imgs) / 255.0


def tensorboard_image(imgs=None, cam=None, out=None):
    """utils/imutils.py:26-40 -> (grid of the images, grid of the jet overlay of max_c bilinear(cam)), nrow = 2.
    out: optional pair of zeroed canvases to paint into."""
    imgs = _images4(imgs, "tensorboard_image")
    if not isinstance(cam, torch.Tensor) or cam.dim() != 4 or cam.shape[0] != imgs.shape[0]:
        raise RuntimeError("tensorboard_image: cam must be (B, C, h, w) with the images' batch size")
    cam = cam.detach().float().contiguous()
    B, _, H, W = imgs.shape
    geo = grid_geometry(B, H, W, 2)
    grid_imgs = paint_images(imgs, _canvas(geo, imgs.device, out and out[0]), geo)
    grid_cam = paint_heat(cam, cam.shape[1], cam.shape[2:], (H, W), _canvas(geo, imgs.device, out and out[1]), geo, JET, imgs=imgs)
    return grid_imgs, grid_cam


def tensorboard_edge(edge=None, n_row=2):
    """utils/imutils.py:42-51: channel 0 of edge (B,C,h,w), up-sampled to 224 x 224, viridis."""
    if not isinstance(edge, torch.Tensor) or edge.dim() != 4:
        raise RuntimeError("tensorboard_edge: edge must be (B, C, h, w)")
    e0 = edge.detach().float()[:, 0].contiguous()
    geo = grid_geometry(e0.shape[0], 224, 224, n_row)
    return paint_heat(e0, 1, e0.shape[1:], (224, 224), _canvas(geo, e0.device), geo, VIRIDIS)


def attn_row(hw, n_pix):
    """The row of an (hw, hw) attention map that tensorboard_attn shows for n_pix (utils/imutils.py:60,64) -> (row, h)."""
    h = w = int(np.sqrt(hw))
    return int(h * n_pix) * (w + 1), h


def attn_rows_grid(rows, size=[224, 224], n_row=4, out=None):
    """The grid of tensorboard_attn from the rows it reads: `rows` = a list of (b, h*w) float32 device tensors (dim 0 may be
    strided), each an already selected row per image."""
    tiles = sum(int(r.shape[0]) for r in rows)
    geo = grid_geometry(tiles, size[0], size[1], n_row, colmajor=True)
    canvas = _canvas(geo, rows[0].device, out)
    k0 = 0
    for r in rows:
        h = int(np.sqrt(r.shape[1]))
        if h * h != r.shape[1]:
            raise RuntimeError(f"tensorboard_attn: {r.shape[1]} tokens are not a square grid")
        paint_heat(r, 1, (h, h), size, canvas, geo, VIRIDIS, aligned=True, normalise=True, k0=k0)
        k0 += int(r.shape[0])
    return canvas


def tensorboard_attn(attns=None, size=[224, 224], n_pix=0, n_row=4):
    """utils/imutils.py:54-85: per (b, hw, hw) map of the list the row int(h * n_pix) * (w + 1) as an (h, w) image, up-sampled
    with align_corners=True, min-max normalised per image, viridis; tiles run down the columns first."""
    rows = []
    for attn in attns:
        if not isinstance(attn, torch.Tensor) or attn.dim() != 3 or attn.shape[1] != attn.shape[2]:
            raise RuntimeError("tensorboard_attn: every map must be (b, hw, hw)")
        a = attn.detach().float()
        if not a.is_contiguous():
            a = a.contiguous()
        rows.append(a[:, attn_row(a.shape[1], n_pix)[0], :])
    return attn_rows_grid(rows, size, n_row)


def tensorboard_attn2(attns=None, size=[224, 224], n_pixs=N_PIXS, n_row=4, with_attn_pred=True):
    """utils/imutils.py:87-123: head 0 of the top layers (and attn_pred) at four n_pix, then every head of the last two."""
    if with_attn_pred:
        top, last = attns[:-3], attns[-3:-1]
    else:
        top, last = attns[:-2], attns[-2:]
    top_layers = [t[:, 0, ...] for t in top]
    if with_attn_pred:
        top_layers.append(attns[-1])
    grids = [tensorboard_attn(top_layers, n_pix=n_pixs[i], n_row=n_row) for i in range(4)]
    last_layer = [a[:, i, :, :] for a in last for i in range(a.shape[1])]
    grids += [tensorboard_attn(last_layer, n_pix=n_pixs[i], n_row=2 * n_row) for i in range(4)]
    return grids


def tensorboard_label(labels=None, out=None):
    """utils/imutils.py:125-133: one label map (H,W) (any singleton dims squeezed) -> its VOC colours (3,H,W); a batch
    (B,H,W) -> the nrow=2 grid of its maps.  int64 or uint8; other integer types are widened."""
    if not isinstance(labels, torch.Tensor):
        raise RuntimeError("tensorboard_label: expected a CUDA tensor")
    lab = labels.detach().squeeze()
    if lab.dim() == 2:
        lab = lab[None]
    if lab.dim() != 3:
        raise RuntimeError("tensorboard_label: labels must squeeze to (H, W) or (B, H, W)")
    if lab.dtype not in (torch.int64, U8):
        lab = lab.long()
    lab = lab.contiguous()
    geo = grid_geometry(lab.shape[0], lab.shape[1], lab.shape[2], 2)
    return paint_labels(lab, _canvas(geo, lab.device, out), geo)


# ---------------------------------------------------------------------------------------------- the train step's snapshot
class StepSnapshot:
    """Caller-owned buffers that `wc_panel_snapshot` fills inside a (captured) train step: `seg` (B,C,hs,ws) f32, `label`
    (B,H,W) uint8 and, with attention, `rows` (B,4,hw) f32 = attn_pred's rows for n_pix 0, 0.3, 0.6, 0.9.  Buffers are created
    by the first `take` of a shape (the eager first step of a batch signature, never inside a capture); `calls` counts takes."""

    def __init__(self):
        self.seg = self.label = self.rows = None
        self.calls = 0

    def _fit(self, seg, label, attn):
        dev = seg.device
        if self.seg is None or self.seg.shape != seg.shape:
            self.seg = torch.zeros(seg.shape, device=dev, dtype=F32)
        if self.label is None or self.label.shape != label.shape:
            self.label = torch.zeros(label.shape, device=dev, dtype=U8)
        if attn is not None and (self.rows is None or tuple(self.rows.shape) != (attn.shape[0], 4, attn.shape[1])):
            self.rows = torch.zeros(attn.shape[0], 4, attn.shape[1], device=dev, dtype=F32)

    def take(self, seg, label, attn=None):
        """seg (B,C,hs,ws) f32, label (B,H,W) int64, attn (B,hw,hw) f32 or None, all contiguous.  One launch, no host read."""
        L.require_gpu()
        if attn is not None and (attn.dim() != 3 or attn.shape[1] != attn.shape[2]):
            raise RuntimeError("StepSnapshot: attn must be (B, hw, hw)")
        self._fit(seg, label, attn)
        hw = 0 if attn is None else int(attn.shape[1])
        rows4 = L.int_array([attn_row(hw, p)[0] for p in N_PIXS]) if attn is not None else None
        L.lib().wc_panel_snapshot(L.ptr(seg, F32, "seg"), seg.numel(), L.ptr(label, torch.int64, "label"), label.numel(),
                                  L.ptr(attn, F32, "attn"), 0 if attn is None else int(attn.shape[0]), hw, rows4,
                                  L.ptr(self.seg, F32), L.ptr(self.label, U8), L.ptr(self.rows if attn is not None else None, F32),
                                  L.stream())
        self.calls += 1
        return self
