"""Inputs of the camutils fixtures (tests/golden/camutils_ref.npz), rebuilt bit for bit wherever they are needed.

Random f32 tensors do not compress, and the fixture has to stay small, so the inputs are not stored: they are functions of a
case's shape and a seed, made with integer hashing and correctly rounded float64 +, -, *, / only (no libm call), so every
platform rebuilds the same bits.  The fixture stores a checksum of every input (`check`), the one table that needs exp (the
sigmoid behind `aff`), and the reference's outputs.  Used by tests/golden/make_camutils_golden.py and by the camutils tests."""
import zlib

import numpy as np
import torch

THRE = (0.35, 0.45, 0.55)               # low_thre, bkg_score, high_thre of the lineage's configs
DILATIONS, NUM_ITER = [1, 2, 4, 8, 12, 24], 10     # the PAR of the lineage's training scripts


class _NS:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def make_cfg(scale=1.0, ignore_index=255):
    return _NS(cam=_NS(low_thre=scale * THRE[0], bkg_score=scale * THRE[1], high_thre=scale * THRE[2]),
               dataset=_NS(ignore_index=ignore_index))


def noise(shape, seed):
    """float64 in [0, 1) on a 2^-16 grid from splitmix64 of (seed, element index)."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.full(1, seed, np.uint64) * np.uint64(0xD1B54A32D192ED03)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return ((z >> np.uint64(48)).astype(np.float64) / 65536.0).reshape(shape)


def smooth(lead, H, W, seed, cell=8):
    """float64 (*lead, H, W) in [0, 1): bilinear interpolation of a noise grid with one knot every `cell` pixels."""
    gh, gw = H // cell + 2, W // cell + 2
    g = noise(tuple(lead) + (gh, gw), seed)
    ys, xs = np.arange(H), np.arange(W)
    y0, x0 = ys // cell, xs // cell
    fy, fx = ((ys % cell) / cell)[:, None], (xs % cell) / cell
    a, b = g[..., y0, :][..., :, x0], g[..., y0, :][..., :, x0 + 1]
    c, d = g[..., y0 + 1, :][..., :, x0], g[..., y0 + 1, :][..., :, x0 + 1]
    return (1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c + fx * d)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _cls(B, C, present):
    m = torch.zeros(B, C)
    for b, ks in enumerate(present):
        m[b, list(ks)] = 1
    return m


def check(*tensors):
    """crc32 over the bytes of the tensors: the fixture records it, the tests compare it."""
    c = 0
    for t in tensors:
        c = zlib.crc32(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes(), c)
    return c


# ---- cam_to_label / ignore_img_box: both sizes odd; full, clipped and inset boxes; one image without classes
def label_case():
    B, C, H, W = 3, 20, 33, 47
    q = np.floor(noise((B, C, H, W), 11) * 65536.0)
    cam = (q * 32 + np.arange(C)[None, :, None, None]) / 2.0 ** 21          # distinct per class: no ties
    return dict(cam=_t(cam), cls=_cls(B, C, [(1, 7, 19), (), (0, 3, 4, 11, 12)]), box=[[0, 33, 0, 47], [5, 40, 10, 60], [4, 29, 6, 41]])


# ---- random walk
WALK_GRIDS = [(7, 9), (20, 20)]
WALK_C = [5, 20, 80]
WALK_PRESENT = {5: [(), (0, 2, 4), (0, 1, 2, 3, 4)], 20: [(), (2, 9, 19), (0, 5, 6, 13, 17)], 80: [(), (1, 40, 79), (0, 31, 32, 63, 64)]}
# the un-normalised walk is recorded for every combination too; at n = 400 only every 7th column is kept
WALK_STRIDE = {63: 1, 400: 7}


def walk_case(h, w, C, sigmoid_table):
    """aff = sigmoid(noise in [-4, 4)) through the fixture's 256-entry table, one column of image 1 zeroed."""
    B, n = 3, h * w
    idx = np.floor(noise((B, n, n), 100 + n) * 256.0).astype(np.int64)
    aff = np.asarray(sigmoid_table, dtype=np.float32)[idx]
    aff[1, :, 5] = 0
    return dict(aff=_t(aff), cams=_t(noise((B, C, h, w), 200 + n + C)), cls=_cls(B, C, WALK_PRESENT[C]))


def sigmoid_table():
    x = (np.arange(256) - 127.5) / 32.0
    return (1.0 / (1.0 + np.exp(-x))).astype(np.float32)


# ---- the two refine_* functions
REFINE_SHAPES = [(3, 5, 32, 48), (3, 20, 34, 46), (2, 80, 32, 32)]
REFINE_PRESENT = {5: [(0, 2, 4), (1,), (0, 1, 2, 3)], 20: [(3, 8, 15), (0, 1, 5, 12, 19), (7,)], 80: [(3, 10, 11, 40, 79), (0,)]}
CAM_SCALE = 8.0


def refine_case(i):
    B, C, H, W = REFINE_SHAPES[i]
    img = 30.0 + 170.0 * smooth((B, 3), H, W, 300 + i) + 25.0 * noise((B, 3, H, W), 310 + i)
    cams = CAM_SCALE * smooth((B, C), H, W, 320 + i, cell=6)
    full, inset, clipped = [0, H, 0, W], [2, H - 5, 3, W - 6], [6, H + 9, 8, W + 20]
    shifted = [4, H - 3, 5, W - 4]                       # the inset box's size at another place
    box_bkg = [full, inset, clipped][:B] if B == 3 else [full, clipped]
    box_cls = [inset, shifted, clipped] if B == 3 else [full, inset]
    return dict(images=_t(img), cams=_t(cams), cls=_cls(B, C, REFINE_PRESENT[C]), box_bkg=box_bkg, box_cls=box_cls,
                cfg=make_cfg(CAM_SCALE))


# ---- multi-scale CAMs: a model that is a pure function of its input
MSC_SCALES = (1.0, 0.5, 1.5)


def msc_inputs():
    return _t(2.0 * smooth((2, 3), 32, 48, 400) - 1.0 + 0.25 * noise((2, 3, 32, 48), 401))


def msc_model(x, cam_only=True):
    """Average pool to 1/16, a fixed channel mix to 4 CAM channels, and an (n, n) outer product as the affinity."""
    import torch.nn.functional as F
    p = F.avg_pool2d(x.float(), 16)
    mix = torch.tensor([[1.0, -0.5, 0.25], [-0.75, 1.0, 0.5], [0.5, 0.5, -1.0], [0.25, -1.0, 0.75]], device=x.device)
    cam = torch.einsum("kc,bchw->bkhw", mix, p)
    t = p.mean(1).flatten(1)
    return cam, t[:, :, None] * t[:, None, :]


# ---- the lineage's lines :310-339 end to end, on refine case 1 with a 7 x 9 token grid
CHAIN_GRID = (7, 9)
CHAIN_RADIUS = 3


def chain_case(sigmoid_table):
    r = refine_case(1)
    B, n = 3, CHAIN_GRID[0] * CHAIN_GRID[1]
    idx = np.floor(noise((B, n, n), 500) * 256.0).astype(np.int64)
    r["aff"] = _t(np.asarray(sigmoid_table, dtype=np.float32)[idx])
    r["box"] = [r["box_bkg"][0]] + r["box_cls"][1:]      # full, inset, clipped (CAMs and thresholds keep the scale of 8)
    return r


def run_chain(M, par, c, mask, amask, resize, aff_label_fn, grid=CHAIN_GRID):
    """Lines :310-339 with the functions of module `M` (the restatement, or the package on the GPU); `resize(x, size)` is the
    bilinear (align_corners=False) resize of that side.  The walks get `aff` itself, not a clone."""
    cfg, box, cls = c["cfg"], c["box"], c["cls"]
    H, W = c["cams"].shape[2:]
    valid_cam, pseudo_label = M.cam_to_label(c["cams"], cls_label=cls, img_box=box, ignore_mid=True, cfg=cfg)
    resized = resize(valid_cam, grid)
    ones = torch.ones(cls.shape[0], 1, dtype=cls.dtype, device=cls.device)
    lab = {}
    for name, thre in (("l", cfg.cam.low_thre), ("h", cfg.cam.high_thre)):
        a = M.propagte_aff_cam_with_bkg(resized, aff=c["aff"], mask=mask, cls_labels=cls, bkg_score=thre)
        r = M.refine_cams_with_cls_label(par, c["images"], cams=resize(a, (H, W)), labels=torch.cat([ones, cls], 1), img_box=box)
        lab[name] = r.argmax(dim=1)
    out = lab["h"].clone()
    out[lab["h"] == 0] = cfg.dataset.ignore_index
    out[(lab["h"] + lab["l"]) == 0] = 0
    out = M.ignore_img_box(out, img_box=box, ignore_index=cfg.dataset.ignore_index)
    rpl = M.refine_cams_with_bkg_v2(par, c["images"], cams=c["cams"], cls_labels=cls, cfg=cfg, img_box=box)
    return dict(pseudo_label=pseudo_label, aff_label_map=out, refined_pseudo_label=rpl,
                affinity_label=aff_label_fn(rpl, mask=amask, ignore_index=cfg.dataset.ignore_index))


def unpack(bits, shape):
    return torch.from_numpy(np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(bool))


def affinity_sure(sure, H, W):
    """(B, n, n): both source pixels of a token pair are sure (nearest sampling to the 1/16 grid, as cams_to_affinity_label)."""
    ys = (torch.arange(H // 16) * (H / (H // 16))).long()
    xs = (torch.arange(W // 16) * (W / (W // 16))).long()
    s = sure[:, ys][:, :, xs].reshape(sure.shape[0], -1)
    return s[:, :, None] & s[:, None, :]
