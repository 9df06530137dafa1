"""Generate tests/golden/panels_ref.npz: inputs and outputs of the reference's utils/imutils.py (the tensorboard image panels) for
tests/test_panels_gpu.py.  Build container only: it needs the reference checkout and matplotlib.

    python tests/golden/make_panels_golden.py

The UNMODIFIED reference module is imported from the checkout (oracle/refharness.REF).  torchvision is not installed here, so a
minimal `torchvision.utils.make_grid` stand-in -- a restatement of its documentation: xmaps = min(nrow, B), ymaps = ceil(B /
xmaps), tile k at (y * (H + padding) + padding, x * (W + padding) + padding), a one-channel input repeated to three, a batch
of one returned bare -- is placed in sys.modules first; matplotlib is the real one.  Data only is stored: the inputs and what
the reference returned.

Heat-map panels (jet / viridis) index their table with int(x * 256), which flips when the fp32 interpolation differs in its
last bit, so next to each such panel the file holds
  <case>/unsure  (h, w) bool: x * 256 lies within `delta` of an integer in [0, 256] (further out the entry is 0 or 255 whatever the
                 last bit), delta = 4 x the largest 256 * |x32 - x64| seen over all cases (x32: what the reference passed to the
                 colormap, x64: the same pipeline in fp64)
  <case>/alt     (n, 2, 3) uint8: at the n unsure pixels (np.nonzero order) the reference's output had the index been k - 1 / k + 1
A test demands equality at every other pixel.  The generator asserts that at most 1 % of a panel is unsure and tries further
seeds otherwise.  Panels of 224 x 224 tiles are stored sub-sampled (`<case>/sub` = (row step, column step)) to keep the file small.
"""
import importlib.util
import math
import os
import sys
import types

os.environ.setdefault("MPLBACKEND", "Agg")
import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "panels_ref.npz")
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
N_PIXS = [0.0, 0.3, 0.6, 0.9]
CAP = 0.01


def make_grid(tensor, nrow=8, padding=2, pad_value=0):
    if tensor.dim() == 4 and tensor.size(1) == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    n, c, h, w = tensor.shape
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(n / xmaps))
    grid = tensor.new_full((c, (h + padding) * ymaps + padding, (w + padding) * xmaps + padding), pad_value)
    for k in range(n):
        y, x = divmod(k, xmaps)
        grid[:, y * (h + padding) + padding:y * (h + padding) + padding + h, x * (w + padding) + padding:x * (w + padding) + padding + w] = tensor[k]
    return grid


def load_reference():
    from oracle import refharness
    tv, tvu = types.ModuleType("torchvision"), types.ModuleType("torchvision.utils")
    tvu.make_grid = make_grid
    tv.utils = tvu
    sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tvu
    spec = importlib.util.spec_from_file_location("reference_imutils", os.path.join(refharness.REF, "utils", "imutils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Plt:
    """Stands where the reference module holds `plt`: get_cmap(name) is matplotlib's colormap, which records the array it is
    called with and, with shift != 0, looks every in-range index up at index + shift (clipped to the table)."""

    def __init__(self, shift=0):
        self.shift, self.seen = shift, []

    def get_cmap(self, name):
        import matplotlib
        cm = matplotlib.colormaps[name]

        def call(X):
            X = np.asarray(X)
            self.seen.append(X.copy())
            out = cm(X)
            if self.shift:
                xa = X.astype(np.float32) * np.float32(256)
                xa[xa == 256] = 255
                plain = np.isfinite(xa) & (xa >= 0) & (xa < 256)
                k = np.clip(np.where(plain, xa, 0).astype(np.int64) + self.shift, 0, 255)
                out[plain] = cm(k)[plain]
            return out
        return call


def run(ref, fn, shift=0):
    """fn(ref) with the recording / shifting colormap -> (result, the arrays the colormap saw)."""
    plt = Plt(shift)
    real, ref.plt = ref.plt, plt
    try:
        return fn(ref), plt.seen
    finally:
        ref.plt = real


def tiles_to_grid(mask, nrow, transposed=False):
    """(n, H, W) bool per-tile masks -> the (h, w) mask of the grid the reference assembled."""
    t = torch.from_numpy(mask.astype(np.uint8))[:, None]
    if transposed:                                        # tensorboard_attn: tiles transposed before make_grid, the grid after it
        return make_grid(t.permute(0, 1, 3, 2), nrow=nrow).permute(0, 2, 1)[0].numpy().astype(bool)
    return make_grid(t, nrow=nrow)[0].numpy().astype(bool)


# ---- the fp64 form of what the reference passes to the colormap -----------------------------------------------------
def x64_cam(cam, size):
    return F.interpolate(cam.double(), size=size, mode="bilinear", align_corners=False).max(dim=1)[0].numpy()


def x64_edge(edge):
    return F.interpolate(edge.double(), size=[224, 224], mode="bilinear", align_corners=False)[:, 0].numpy()


def x64_attn(attns, size, n_pix):
    out = []
    for a in attns:
        b, hw, _ = a.shape
        h = w = int(np.sqrt(hw))
        x = F.interpolate(a.double()[:, int(h * n_pix) * (w + 1), :].reshape(b, 1, h, w), size=size, mode="bilinear", align_corners=True)[:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            for i in range(b):
                x[i] = x[i] - x[i].min()
                x[i] = x[i] / x[i].max()
        out.append(x.numpy())
    return np.concatenate(out, 0)


class Heat:
    """One heat-map panel: call(ref) -> the grid; x64: (n, H, W); nrow / transposed: how its tiles form the grid; pick: which of the
    colormap calls made by `call` are this panel's (tensorboard_attn2 renders all eight grids at once)."""

    def __init__(self, name, call, x64, nrow, transposed=False, sub=None, pick=slice(None)):
        self.name, self.call, self.x64, self.nrow, self.transposed, self.sub, self.pick = name, call, x64, nrow, transposed, sub, pick


def measure(ref, heats):
    """-> delta = 4 x max 256 |x32 - x64| over every heat panel."""
    worst = 0.0
    for h in heats:
        _, seen = run(ref, h.call)
        x32 = np.concatenate([s.reshape((-1,) + s.shape[-2:]) for s in seen[h.pick]], 0).astype(np.float64)
        ok = np.isfinite(x32) & np.isfinite(h.x64)
        assert np.array_equal(np.isnan(x32), np.isnan(h.x64)), h.name
        worst = max(worst, float((256 * np.abs(x32 - h.x64))[ok].max()))
    return 4 * worst


def record(ref, h, delta, out):
    grid, seen = run(ref, h.call)
    x32 = np.concatenate([s.reshape((-1,) + s.shape[-2:]) for s in seen[h.pick]], 0).astype(np.float64) * 256
    with np.errstate(invalid="ignore"):
        near = np.isfinite(x32) & (np.abs(x32 - np.round(x32)) <= delta) & (x32 >= -delta) & (x32 <= 256 + delta)
    frac = near.mean()
    if frac > CAP:
        print(f"  {h.name}: {frac:.3%} of the panel is unsure")
        return False
    unsure = tiles_to_grid(near, h.nrow, h.transposed)
    lo, hi = run(ref, h.call, -1)[0].numpy(), run(ref, h.call, +1)[0].numpy()
    g = grid.numpy()
    assert g.dtype == np.uint8 and unsure.shape == g.shape[1:], (h.name, g.shape, unsure.shape)
    if h.sub:
        sy, sx = h.sub
        g, lo, hi, unsure = g[:, ::sy, ::sx], lo[:, ::sy, ::sx], hi[:, ::sy, ::sx], unsure[::sy, ::sx]
        out[h.name + "/sub"] = np.array(h.sub)
    out[h.name + "/ref"] = np.ascontiguousarray(g)
    out[h.name + "/unsure"] = np.ascontiguousarray(unsure)
    out[h.name + "/alt"] = np.stack([lo[:, unsure].T, hi[:, unsure].T], 1).astype(np.uint8)
    out[h.name + "/unsure_fraction"] = np.array(frac)
    return True


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    d = {}
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    for B in (1, 3, 4):
        u8 = torch.randint(0, 256, (B, 3, 20, 28), generator=g)
        d[f"img_B{B}/imgs"] = ((u8.float() - mean) / std)                   # normalised uint8: the truncation cases occur
        cam = torch.rand(B, 2, 5, 7, generator=g)
        if B > 1:                                                           # (a corner value reaches 2 x 2 pixels as it is; the 560
            cam[1, 0, 0, 0], cam[1, 1, 0, 0] = 0.0, 0.0                     #  pixels of B = 1 have room for one such corner under the cap)
        cam[0, 0, 4, 6] = 1.0                                               # exactly 1; above: exactly 0 in both channels, so the max is 0
        cam[0, 1, 2, 3] = -0.25                                             # below 0 (the other channel wins)
        cam[0, 0, 2, 0], cam[0, 1, 2, 0] = -0.5, -0.125                     # below 0 after the max
        cam[0, 0, 0, 6] = 1.75                                              # above 1
        cam[B - 1, 1, 4, 0] = float("nan")
        d[f"img_B{B}/cam"] = cam
    lab = torch.randint(0, 21, (20, 28), generator=g)
    lab[:, :2] = 255
    lab[7, :] = 255
    d["label/labels"] = lab
    a16 = torch.rand(2, 16, 16, generator=g)
    a25 = torch.rand(2, 25, 25, generator=g)
    a25[1, 0, :] = 0.0                                                      # a constant row: 0 / 0 (zero: every interpolation of it is exact)
    d["attn/a16"], d["attn/a25"] = a16, a25
    for i, shape in enumerate([(2, 2, 16, 16), (2, 2, 25, 25), (2, 2, 16, 16), (2, 2, 16, 16), (2, 2, 25, 25)]):
        d[f"attn2/l{i}"] = torch.rand(*shape, generator=g)
    d["attn2/l5"] = torch.rand(2, 16, 16, generator=g)
    d["edge/edge"] = torch.rand(2, 2, 6, 9, generator=g)
    return d


def heats_of(d):
    hs = []
    for B in (1, 3, 4):
        imgs, cam = d[f"img_B{B}/imgs"], d[f"img_B{B}/cam"]
        hs.append(Heat(f"img_B{B}/grid_cam", lambda r, i=imgs, c=cam: r.tensorboard_image(i.clone(), c.clone())[1],
                       x64_cam(cam, [20, 28]), 2))
    attns = [d["attn/a16"], d["attn/a25"]]
    for n_row in (2, 4):
        for j, n_pix in enumerate(N_PIXS):
            hs.append(Heat(f"attn/row{n_row}_pix{j}", lambda r, p=n_pix, n=n_row: r.tensorboard_attn([a.clone() for a in attns], size=[24, 36], n_pix=p, n_row=n),
                           x64_attn(attns, [24, 36], n_pix), n_row, transposed=True))
    l = [d[f"attn2/l{i}"] for i in range(6)]
    top = [t[:, 0] for t in l[:3]] + [l[5]]
    last = [a[:, i] for a in l[3:5] for i in range(a.shape[1])]
    for j, n_pix in enumerate(N_PIXS):
        hs.append(Heat(f"attn2/grid{j}", lambda r, j=j: r.tensorboard_attn2([a.clone() for a in l])[j],
                       x64_attn(top, [224, 224], n_pix), 4, transposed=True, sub=(7, 5), pick=slice(4 * j, 4 * j + 4)))
        hs.append(Heat(f"attn2/grid{4 + j}", lambda r, j=j: r.tensorboard_attn2([a.clone() for a in l])[4 + j],
                       x64_attn(last, [224, 224], n_pix), 8, transposed=True, sub=(7, 5), pick=slice(16 + 4 * j, 20 + 4 * j)))
    hs.append(Heat("edge/grid", lambda r: r.tensorboard_edge(d["edge/edge"].clone()), x64_edge(d["edge/edge"]), 2, sub=(3, 5)))
    return hs


def main():
    ref = load_reference()
    for seed in range(20, 40):
        d = inputs(seed)
        hs = heats_of(d)
        delta = measure(ref, hs)
        out = {k: v.numpy() for k, v in d.items()}
        if not all(record(ref, h, delta, out) for h in hs):
            print(f"seed {seed}: a panel has more than {CAP:.0%} unsure pixels, trying the next")
            continue
        for B in (1, 3, 4):
            imgs = d[f"img_B{B}/imgs"]
            out[f"img_B{B}/grid_imgs"] = ref.tensorboard_image(imgs.clone(), d[f"img_B{B}/cam"].clone())[0].numpy()
            out[f"img_B{B}/denorm"] = ref.denormalize_img(imgs.clone()).numpy()
        out["label/grid"] = ref.tensorboard_label(d["label/labels"].numpy()).numpy()
        out["delta"], out["seed"] = np.array(delta), np.array(seed)
        np.savez_compressed(OUT, **out)
        worst = max(float(out[h.name + "/unsure_fraction"]) for h in hs)
        print(f"wrote {OUT}: seed {seed}, delta {delta:.3e}, {len(hs)} heat panels, worst unsure fraction {worst:.4%}, "
              f"{os.path.getsize(OUT)} bytes")
        return 0
    raise SystemExit("no seed kept every panel within the cap")


if __name__ == "__main__":
    raise SystemExit(main())
