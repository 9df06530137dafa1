"""GPU tests of csrc/panels.hip through `weclip_vit_comer_amd.utils.panels` against tests/golden/panels_ref.npz, which holds what
the reference's utils/imutils.py returned for the same inputs (tests/golden/make_panels_golden.py; torchvision's make_grid is a
restatement of its documentation there).

Image and label panels: equality.  Jet / viridis panels: the table index int(x * 256) flips when the fp32 interpolation differs
in its last bit, so the fixture marks the pixels whose x * 256 lies within delta of an integer (`unsure`, at most 1 % of a panel;
delta = 4 x the largest 256 * |fp32 - fp64| the generator saw) and stores the reference's output for the two neighbouring
indices there: equality at every other pixel, one of the three values at an unsure one.
"""
import os

import numpy as np
import pytest
import torch

import weclip_vit_comer_amd  # noqa: F401
from weclip_vit_comer_amd.utils import panels as P

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_PIXS = [0.0, 0.3, 0.6, 0.9]


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLD, "panels_ref.npz")))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_heat(ref, case, got):
    """got: the device grid of `case`.  Equality at the sure pixels, the reference's k - 1 / k / k + 1 output at the unsure ones."""
    want, unsure, alt = ref[case + "/ref"], ref[case + "/unsure"], ref[case + "/alt"]
    got = got.cpu().numpy()
    if case + "/sub" in ref:
        sy, sx = ref[case + "/sub"]
        got = got[:, ::sy, ::sx]
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.shape, want.shape)
    assert unsure.mean() <= 0.01
    sure_bad = (got != want).any(0) & ~unsure
    print(f"{case}: {int((got != want).any(0).sum())} of {unsure.size} pixels differ, {int(unsure.sum())} unsure, {int(sure_bad.sum())} sure ones differ")
    assert not sure_bad.any(), np.argwhere(sure_bad)[:8]
    g = got[:, unsure].T                                                   # (n, 3), np.nonzero order
    ok = (g == want[:, unsure].T).all(1) | (g == alt[:, 0]).all(1) | (g == alt[:, 1]).all(1)
    assert ok.all(), (np.argwhere(unsure)[~ok][:8], g[~ok][:8])


# ---------------------------------------------------------------------------------------------- images, overlay, labels
@pytest.mark.parametrize("B", [1, 3, 4])
def test_image_grid_and_denormalize_equal_the_reference(ref, B):
    imgs, cam = _cuda(ref[f"img_B{B}/imgs"]), _cuda(ref[f"img_B{B}/cam"])
    grid_imgs, _ = P.tensorboard_image(imgs, cam)
    assert grid_imgs.dtype == torch.uint8 and grid_imgs.is_cuda
    assert torch.equal(grid_imgs.cpu(), torch.from_numpy(ref[f"img_B{B}/grid_imgs"]))
    assert torch.equal(P.denormalize_img(imgs).cpu(), torch.from_numpy(ref[f"img_B{B}/denorm"]))
    # `/ 255.0` of a device tensor is ATen's multiplication by the rounded reciprocal: within one fp32 ulp of the host's division
    assert torch.allclose(P.denormalize_img2(imgs).cpu(), torch.from_numpy(ref[f"img_B{B}/denorm"]) / 255.0, rtol=2.0 ** -23, atol=0)


@pytest.mark.parametrize("B", [1, 3, 4])
def test_cam_overlay_grid(ref, B):
    imgs, cam = _cuda(ref[f"img_B{B}/imgs"]), _cuda(ref[f"img_B{B}/cam"])
    _check_heat(ref, f"img_B{B}/grid_cam", P.tensorboard_image(imgs, cam)[1])


def test_label_panel_equals_the_reference(ref):
    lab = _cuda(ref["label/labels"])
    want = torch.from_numpy(ref["label/grid"])
    assert (lab == 255).any() and want.shape == (3, 20, 28)
    for t in (lab, lab.to(torch.uint8), lab[None], lab.int()):
        assert torch.equal(P.tensorboard_label(t).cpu(), want)
    # 255 is (224, 224, 192)
    y, x = (lab == 255).nonzero()[0].tolist()
    assert P.tensorboard_label(lab)[:, y, x].tolist() == [224, 224, 192]


def test_label_batch_is_the_grid_of_its_maps(ref):
    """Beyond the reference: (B, H, W) labels -> make_grid(nrow=2) of the per-map panels."""
    lab = _cuda(ref["label/labels"])
    batch = torch.stack([lab, lab.flip(0), lab.flip(1)])
    got = P.tensorboard_label(batch).cpu()
    geo = P.grid_geometry(3, 20, 28, 2)
    want = torch.zeros(3, geo.canvas_h, geo.canvas_w, dtype=torch.uint8)
    for k in range(3):
        y, x = divmod(k, 2)
        want[:, 2 + y * 22:2 + y * 22 + 20, 2 + x * 30:2 + x * 30 + 28] = P.tensorboard_label(batch[k]).cpu()
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- attention, edge
@pytest.mark.parametrize("n_row", [2, 4])
@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_attention_grid(ref, n_row, j):
    attns = [_cuda(ref["attn/a16"]), _cuda(ref["attn/a25"])]
    got = P.tensorboard_attn(attns, size=[24, 36], n_pix=N_PIXS[j], n_row=n_row)
    _check_heat(ref, f"attn/row{n_row}_pix{j}", got)
    if j == 0:                                                             # a25[1]'s row 0 is constant: 0 / 0, a black tile (tile 3)
        geo = P.grid_geometry(4, 24, 36, n_row, colmajor=True)
        ty, tx = 3 % geo.xmaps, 3 // geo.xmaps
        tile = got[:, 2 + ty * 26:2 + ty * 26 + 24, 2 + tx * 38:2 + tx * 38 + 36]
        assert tile.shape == (3, 24, 36) and int(tile.max()) == 0


def test_attn2_grids(ref):
    attns = [_cuda(ref[f"attn2/l{i}"]) for i in range(6)]
    grids = P.tensorboard_attn2(attns)
    assert len(grids) == 8
    assert tuple(grids[0].shape) == (3, 226 * 4 + 2, 226 * 2 + 2) and tuple(grids[4].shape) == (3, 226 * 8 + 2, 226 + 2)
    for j in range(8):
        _check_heat(ref, f"attn2/grid{j}", grids[j])


def test_edge_grid(ref):
    got = P.tensorboard_edge(_cuda(ref["edge/edge"]))
    assert tuple(got.shape) == (3, 228, 454)
    _check_heat(ref, "edge/grid", got)


# ---------------------------------------------------------------------------------------------- robustness
def _lut():
    """Entries 0 and 255 and the entry of x = 0.5 of the compiled tables, read through the kernel itself at h = w = 1."""
    out = {}
    for cmap in (P.JET, P.VIRIDIS):
        src = torch.tensor([0.0, 1.0, 0.5], device="cuda").view(3, 1)
        geo = P.Geometry(1, 3, 0, 0, 3, 0, False)
        out[cmap] = P.paint_heat(src, 1, (1, 1), (1, 1), torch.zeros(3, 1, 3, device="cuda", dtype=torch.uint8), geo, cmap)[:, 0].T.cpu()
    return out


def test_nan_and_out_of_range_values_are_exact():
    lut = _lut()
    assert lut[P.JET][0].tolist() == [0, 0, 127] and lut[P.JET][1].tolist() == [127, 0, 0]        # jet(0) = (0, 0, .5), jet(1) = (.5, 0, 0)
    assert lut[P.VIRIDIS][0].tolist() == [68, 1, 84] and lut[P.VIRIDIS][1].tolist() == [253, 231, 36]
    vals = [float("nan"), -3.0, -1e-9, 7.5, 1.0, 0.0]
    want = [None, 0, 0, 1, 1, 0]                                            # None: the "bad" colour (0, 0, 0)
    for cmap in (P.JET, P.VIRIDIS):
        # constant 3 x 5 maps up-sampled (align_corners=False) to 7 x 9: every pixel keeps the value's class
        src = torch.tensor(vals, device="cuda").view(-1, 1, 1, 1).expand(-1, 1, 3, 5).contiguous()
        geo = P.grid_geometry(len(vals), 7, 9, 4)
        got = P.paint_heat(src, 1, (3, 5), (7, 9), torch.zeros(3, geo.canvas_h, geo.canvas_w, device="cuda", dtype=torch.uint8), geo, cmap).cpu()
        for k, w in enumerate(want):
            y, x = divmod(k, 4)
            tile = got[:, 2 + y * 9:2 + y * 9 + 7, 2 + x * 11:2 + x * 11 + 9]
            colour = torch.zeros(3, dtype=torch.uint8) if w is None else lut[cmap][w]
            assert torch.equal(tile, colour.view(3, 1, 1).expand(3, 7, 9)), (cmap, vals[k])


def test_overlay_of_a_nan_map_is_half_the_image(ref):
    imgs = _cuda(ref["img_B3/imgs"])
    cam = torch.full((3, 2, 5, 7), float("nan"), device="cuda")
    cam[:, 0] = 0.3                                                        # a NaN in any channel wins the max, as torch.max
    _, grid_cam = P.tensorboard_image(imgs, cam)
    img_grid = torch.from_numpy(ref["img_B3/grid_imgs"])
    assert torch.equal(grid_cam.cpu(), (img_grid.double() * 0.5).to(torch.uint8))


def test_constant_and_nan_attention_tiles_are_black():
    a = torch.rand(3, 16, 16, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    a[1, 0, :] = 0.0                                                       # constant: 0 / 0
    a[2, 0, 5] = float("nan")                                              # min and max are NaN: every pixel is
    got = P.tensorboard_attn([a], size=[10, 12], n_pix=0, n_row=4).cpu()
    assert tuple(got.shape) == (3, 3 * 12 + 2, 14 + 2)                      # three tiles down ONE column
    assert int(got[:, 2:12].max()) > 0
    assert int(got[:, 14:24].max()) == 0 and int(got[:, 26:36].max()) == 0
    # the normalised tile holds viridis(0) at its minimum and viridis(1) at its maximum
    lut = _lut()[P.VIRIDIS]
    flat = got[:, 2:12, 2:14].reshape(3, -1).T
    assert (flat == lut[0]).all(1).any() and (flat == lut[1]).all(1).any()


@pytest.mark.parametrize("colmajor", [False, True])
def test_pitch_and_origin_leave_every_other_byte_untouched(ref, colmajor):
    """Tiles painted into a larger canvas at an offset origin: bytes outside the tiles keep the sentinel."""
    imgs, cam = _cuda(ref["img_B3/imgs"]), _cuda(ref["img_B3/cam"])
    lab = _cuda(ref["label/labels"])
    labs = torch.stack([lab, lab.flip(0), lab.flip(1)])
    tight = P.grid_geometry(3, 20, 28, 2, colmajor=colmajor)
    geo = tight._replace(canvas_h=tight.canvas_h + 9, canvas_w=tight.canvas_w + 13, oy=5, ox=7)
    inside = torch.zeros(geo.canvas_h, geo.canvas_w, dtype=torch.bool)
    for k in range(3):
        a, b = k % geo.xmaps, k // geo.xmaps
        ty, tx = (a, b) if colmajor else (b, a)
        inside[5 + ty * 22:5 + ty * 22 + 20, 7 + tx * 30:7 + tx * 30 + 28] = True
    blank = lambda g: torch.full((3, g.canvas_h, g.canvas_w), 0x5A, device="cuda", dtype=torch.uint8)      # noqa: E731
    t0 = tight._replace(oy=2, ox=2)
    paints = [lambda c, g: P.paint_images(imgs, c, g),
              lambda c, g: P.paint_labels(labs, c, g),
              lambda c, g: P.paint_heat(cam, 2, (5, 7), (20, 28), c, g, P.JET, imgs=imgs),
              lambda c, g: P.paint_heat(cam[:, 0], 1, (5, 7), (20, 28), c, g, P.VIRIDIS, aligned=True, normalise=True)]
    for paint in paints:
        big, small = paint(blank(geo), geo).cpu(), paint(blank(t0), t0).cpu()
        assert (big[:, ~inside] == 0x5A).all()
        assert torch.equal(big[:, 3:3 + tight.canvas_h, 5:5 + tight.canvas_w][:, inside[3:3 + tight.canvas_h, 5:5 + tight.canvas_w]],
                           small[:, inside[3:3 + tight.canvas_h, 5:5 + tight.canvas_w]])
    # a tile that would leave the canvas is refused, nothing is written
    c = blank(tight)
    with pytest.raises(RuntimeError, match="do not fit"):
        P.paint_images(imgs, c, tight._replace(oy=5))              # 5 + 22 + 20 > 46
    with pytest.raises(RuntimeError, match="do not fit"):
        P.paint_labels(labs, c, tight._replace(xmaps=3) if not colmajor else tight._replace(xmaps=1))
    assert (c == 0x5A).all()


# ---------------------------------------------------------------------------------------------- the step snapshot
def _snap_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    seg = torch.randn(2, 21, 4, 4, generator=g)
    lab = torch.randint(0, 21, (2, 32, 32), generator=g)
    lab[:, :3] = 255
    lab[1, 5, 7] = 255
    attn = torch.rand(2, 16, 16, generator=g)
    return seg.cuda(), lab.cuda(), attn.cuda()


def _snap_expect(seg, lab, attn):
    rows = [int(4 * p) * 5 for p in N_PIXS]
    assert rows == [0, 5, 10, 15]
    return seg, lab.to(torch.uint8), attn[:, rows, :]


def test_snapshot_equals_torch_indexing_and_casts():
    seg, lab, attn = _snap_inputs(1)
    snap = P.StepSnapshot().take(seg, lab, attn)
    want = _snap_expect(seg, lab, attn)
    assert torch.equal(snap.seg, want[0]) and torch.equal(snap.label, want[1]) and torch.equal(snap.rows, want[2])
    assert snap.label.dtype == torch.uint8 and (snap.label == 255).any()
    # without attention (the supervised variant), and a label count that is no multiple of 4
    s2 = P.StepSnapshot().take(seg, lab[:, :31, :31].contiguous())
    assert s2.rows is None and torch.equal(s2.label, lab[:, :31, :31].to(torch.uint8)) and torch.equal(s2.seg, seg)
    # values beyond a byte keep their low byte, torch's cast
    wide = lab.clone()
    wide[0, 0, :4] = torch.tensor([256, 511, -1, 1000], device="cuda")
    assert torch.equal(P.StepSnapshot().take(seg, wide).label, wide.to(torch.uint8))
    with pytest.raises(RuntimeError, match="hw, hw"):
        P.StepSnapshot().take(seg, lab, attn[:, :8])
    with pytest.raises(RuntimeError, match="aligned"):                     # a label map that starts off a 16-byte boundary
        P.StepSnapshot().take(seg, lab.flatten()[1:1 + 2 * 32 * 31].view(2, 32, 31))


def test_snapshot_in_a_captured_graph_follows_its_inputs():
    seg, lab, attn = _snap_inputs(2)
    snap = P.StepSnapshot().take(seg, lab, attn)                           # creates the buffers and warms the library up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        snap.take(seg, lab, attn)
    for seed in (3, 4):
        for dst, src in zip((seg, lab, attn), _snap_inputs(seed)):
            dst.copy_(src)
        snap.seg.fill_(-1), snap.label.fill_(7), snap.rows.fill_(-1)
        g.replay()
        want = _snap_expect(*_snap_inputs(seed))
        assert torch.equal(snap.seg, want[0]) and torch.equal(snap.label, want[1]) and torch.equal(snap.rows, want[2])


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="CUDA"):
        P.tensorboard_label(torch.zeros(4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="CUDA"):
        P.tensorboard_image(torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 2, 2))
    with pytest.raises(RuntimeError, match="CUDA"):
        P.tensorboard_attn([torch.zeros(1, 4, 4)])


def test_registered_ops_equal_the_module(ref):
    import weclip_vit_comer_amd.torch_ops as TO
    assert {"panel_images", "panel_labels", "panel_attn"} <= set(TO.OPS)
    imgs, cam = _cuda(ref["img_B3/imgs"]), _cuda(ref["img_B3/cam"])
    a, b = torch.ops.weclip.panel_images(imgs, cam)
    wa, wb = P.tensorboard_image(imgs, cam)
    assert torch.equal(a, wa) and torch.equal(b, wb)
    lab = _cuda(ref["label/labels"])
    assert torch.equal(torch.ops.weclip.panel_labels(lab[None]), P.tensorboard_label(lab))
    attns = [_cuda(ref["attn/a16"]), _cuda(ref["attn/a25"])]
    assert torch.equal(torch.ops.weclip.panel_attn(attns, [24, 36], 0.3, 2), P.tensorboard_attn(attns, size=[24, 36], n_pix=0.3, n_row=2))
    with pytest.raises(NotImplementedError):
        torch.ops.weclip.panel_labels(lab[None].cpu())
