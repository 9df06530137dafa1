"""GPU tests of csrc/evalfinish.hip through the C ABI: `wc_eval_finish` against the parent's kernels (`wc_resize_argmax`,
`wc_confusion_hist`) bit for bit, against ATen up to near-ties, its NULL combinations and argument errors, the colour map
against the table recorded from the reference's `colormap()` (tests/golden/voc_cmap.npz), and `wc_label_finish`."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# name: (C, Hs, Ws, Hl, Wl, nc, out-of-range CAM cells, raises the flag)
CASES = {
    "voc21": (21, 5, 7, 70, 90, 21, False, False),
    "voc21_badcam": (21, 5, 7, 70, 90, 21, True, True),
    "coco81": (81, 9, 4, 131, 69, 81, False, False),          # three 81x81 LDS histograms = 78,732 bytes > 64 KiB
    "one_partial_group": (1, 3, 3, 3, 5, 1, False, False),
    "identity": (21, 8, 8, 8, 8, 21, False, False),
    "pred_beyond_nc": (5, 4, 6, 33, 17, 3, False, True),      # predictions 3, 4 >= nc = 3: skipped, flag raised
}
ANCHORS = {0: (0, 0, 0), 1: (128, 0, 0), 2: (0, 128, 0), 15: (192, 128, 128), 255: (224, 224, 192)}
_cache = {}


def _lib():
    from weclip_vit_comer_amd import _lib as L
    return L


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _zeros(nc):
    return torch.zeros(nc, nc, device="cuda", dtype=torch.int64)


def _flag():
    return torch.zeros(1, device="cuda", dtype=torch.int32)


def _finish(c, seg1="seg1", msc="msc", cam="cam", gt="gt", maps=True, hists=None, flag=None):
    """One wc_eval_finish call on case dict c; string arguments name c's tensors, None passes NULL.  -> outputs dict."""
    L = _lib()
    C, Hs, Ws, Hl, Wl, nc = c["dims"]
    get = lambda k: None if k is None else c[k]      # noqa: E731
    out = {"flag": flag if flag is not None else _flag()}
    if maps:
        out["pred1"] = torch.full((Hl, Wl), 7, device="cuda", dtype=torch.uint8)
        out["predm"] = torch.full((Hl, Wl), 7, device="cuda", dtype=torch.uint8) if msc else None
        out["cmap"] = torch.full((Hl, Wl, 3), 7, device="cuda", dtype=torch.uint8)
    h = hists if hists is not None else {"hist": _zeros(nc), "msc_hist": _zeros(nc) if msc else None,
                                         "cam_hist": _zeros(nc) if cam else None}
    out.update(h)
    L.lib().wc_eval_finish(_p(get(seg1)), _p(get(msc)), _p(get(cam)), _p(get(gt)), _p(out.get("pred1")), _p(out.get("predm")),
                           _p(out.get("cmap")), _p(h.get("hist")), _p(h.get("msc_hist")), _p(h.get("cam_hist")), _p(out["flag"]),
                           C, Hs, Ws, Hl, Wl, nc, L.stream())
    return out


def _ref_hist(L, gt, pred, nc, flag, hist=None):
    hist = _zeros(nc) if hist is None else hist
    L.lib().wc_confusion_hist(_p(gt), _p(pred), _p(hist), _p(flag), gt.numel(), nc, L.stream())
    return hist


def _case(name):
    """Inputs of a case and what the parent's kernels make of them, computed once and shared (never modified)."""
    if name in _cache:
        return _cache[name]
    L = _lib()
    C, Hs, Ws, Hl, Wl, nc, bad_cam, raises = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    c = {"dims": (C, Hs, Ws, Hl, Wl, nc), "raises": raises}
    c["seg1"] = torch.randn(C, Hs, Ws, generator=g).cuda()
    c["msc"] = torch.randn(C, Hs, Ws, generator=g).cuda()
    gt = torch.randint(0, nc, (Hl, Wl), generator=g)
    gt[torch.rand(Hl, Wl, generator=g) < 0.03] = nc + 2          # a class id the histogram does not hold
    if Hl > 4 and Wl > 4:
        gt[0], gt[-1], gt[:, 0], gt[:, -1] = 255, 255, 255, 255
    else:
        gt[0, 0] = 255
    cam = torch.randint(0, nc, (Hl, Wl), generator=g)
    if bad_cam:
        cam[5, 7], cam[33, 41], cam[20, 3] = nc, -1, 1000
        assert 0 <= gt[5, 7] < nc or 0 <= gt[33, 41] < nc or 0 <= gt[20, 3] < nc
    c["gt"], c["cam"] = gt.cuda(), cam.cuda()
    for k in ("seg1", "msc"):
        pred = torch.empty(Hl, Wl, device="cuda", dtype=torch.int64)
        L.lib().wc_resize_argmax(_p(c[k]), _p(pred), C, Hs, Ws, Hl, Wl, L.stream())
        c["p_" + k] = pred
    c["ref_flag"] = _flag()
    c["ref_hist"] = _ref_hist(L, c["gt"], c["p_seg1"], nc, c["ref_flag"])
    c["ref_msc_hist"] = _ref_hist(L, c["gt"], c["p_msc"], nc, c["ref_flag"])
    c["ref_cam_hist"] = _ref_hist(L, c["gt"], c["cam"], nc, c["ref_flag"])
    _cache[name] = c
    return c


@pytest.fixture(scope="module")
def table(golden):
    t = torch.from_numpy(golden("voc_cmap.npz")["cmap"]).cuda()
    assert tuple(t.shape) == (256, 3) and t.dtype == torch.uint8
    return t


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equal_with_the_parents_kernels(name, table):
    """pred1_u8 / predm_u8 == wc_resize_argmax cast to uint8; the three histograms == wc_confusion_hist on those maps, from zero
    and accumulated over two calls; the colour image == table[prediction]; the flag is raised exactly where the case says."""
    c = _case(name)
    nc = c["dims"][5]
    out = _finish(c)
    assert torch.equal(out["pred1"], c["p_seg1"].to(torch.uint8)) and torch.equal(out["predm"], c["p_msc"].to(torch.uint8))
    assert torch.equal(out["cmap"], table[c["p_msc"]])
    for k in ("hist", "msc_hist", "cam_hist"):
        assert torch.equal(out[k], c["ref_" + k]), k
    valid = int(((c["gt"] >= 0) & (c["gt"] < nc)).sum())
    if not c["raises"]:
        assert int(out["hist"].sum()) == int(out["msc_hist"].sum()) == int(out["cam_hist"].sum()) == valid > 0
    assert int(out["flag"].item()) == int(c["ref_flag"].item()) == int(c["raises"])
    again = _finish(c, hists={k: out[k] for k in ("hist", "msc_hist", "cam_hist")})
    for k in ("hist", "msc_hist", "cam_hist"):
        assert torch.equal(again[k], 2 * c["ref_" + k]), k


@pytest.mark.parametrize("name", ["voc21", "coco81"])
def test_null_combinations(name, table):
    c = _case(name)
    nc = c["dims"][5]
    # no msc: the colour image is the scale-1 prediction's
    out = _finish(c, msc=None)
    assert torch.equal(out["pred1"], c["p_seg1"].to(torch.uint8)) and torch.equal(out["cmap"], table[c["p_seg1"]])
    assert torch.equal(out["hist"], c["ref_hist"]) and torch.equal(out["cam_hist"], c["ref_cam_hist"])
    # no cam
    out = _finish(c, cam=None)
    assert torch.equal(out["hist"], c["ref_hist"]) and torch.equal(out["msc_hist"], c["ref_msc_hist"])
    assert torch.equal(out["predm"], c["p_msc"].to(torch.uint8))
    # no gt: the maps are written, the histograms (passed all the same) are untouched
    out = _finish(c, gt=None)
    assert torch.equal(out["pred1"], c["p_seg1"].to(torch.uint8)) and torch.equal(out["predm"], c["p_msc"].to(torch.uint8))
    assert torch.equal(out["cmap"], table[c["p_msc"]])
    assert int(out["hist"].sum()) == int(out["msc_hist"].sum()) == int(out["cam_hist"].sum()) == 0
    out = _finish(c, gt=None, cam=None, hists={"hist": None, "msc_hist": None, "cam_hist": None})
    assert torch.equal(out["predm"], c["p_msc"].to(torch.uint8)) and int(out["flag"].item()) == 0
    # no output maps: only the histograms
    out = _finish(c, maps=False)
    for k in ("hist", "msc_hist", "cam_hist"):
        assert torch.equal(out[k], c["ref_" + k]), k
    assert int(out["hist"].sum()) == int(((c["gt"] >= 0) & (c["gt"] < nc)).sum())


@pytest.mark.parametrize("name", ["voc21", "coco81", "identity"])
def test_against_aten(name):
    """F.interpolate(bilinear, align_corners=False).argmax may differ from the kernel only at pixels whose top-2 gap is below 1e-4:
    the mismatch fraction is at most that near-tie fraction, which normal logits keep far below 1 %."""
    c = _case(name)
    out = _finish(c, gt=None, cam=None, hists={"hist": None, "msc_hist": None, "cam_hist": None})
    Hl, Wl = c["dims"][3:5]
    for key, got in (("seg1", out["pred1"]), ("msc", out["predm"])):
        up = F.interpolate(c[key][None], size=(Hl, Wl), mode="bilinear", align_corners=False)[0]
        top = up.topk(2, dim=0).values
        ties = ((top[0] - top[1]) < 1e-4).float().mean().item()
        mism = (up.argmax(0) != got.long()).float().mean().item()
        print(f"{name} {key}: mismatch vs ATen {mism:.4%}, near-tie fraction {ties:.4%}")
        assert mism <= ties <= 0.01


def test_colour_anchors_and_every_label_through_label_finish(table):
    L = _lib()
    for v, rgb in ANCHORS.items():
        assert tuple(table[v].tolist()) == rgb
    H, W, nc = 23, 29, 21
    pred = (torch.arange(H * W) % 256).view(H, W).cuda()                    # every label 0..255, rows of odd length
    gt = (torch.arange(H * W) % 23).view(H, W).cuda()                       # 21, 22: outside [0, nc)
    gt[0] = 255
    u8 = torch.full((H, W), 9, device="cuda", dtype=torch.uint8)
    rgb = torch.full((H, W, 3), 9, device="cuda", dtype=torch.uint8)
    hist, flag, ref_flag = _zeros(nc), _flag(), _flag()
    L.lib().wc_label_finish(_p(pred), _p(gt), _p(u8), _p(rgb), _p(hist), _p(flag), H, W, nc, L.stream())
    assert torch.equal(u8, pred.to(torch.uint8)) and torch.equal(rgb, table[pred])
    for v, colour in ANCHORS.items():
        assert tuple(rgb.view(-1, 3)[v].tolist()) == colour
    assert torch.equal(hist, _ref_hist(L, gt, pred, nc, ref_flag)) and int(hist.sum()) > 0
    assert int(flag.item()) == int(ref_flag.item()) == 1                    # labels >= nc at counted pixels


def test_label_finish_in_range_and_beyond_255(table):
    L = _lib()
    H, W, nc = 37, 18, 81
    g = torch.Generator().manual_seed(5)
    pred = torch.randint(0, nc, (H, W), generator=g).cuda()
    gt = torch.randint(0, nc, (H, W), generator=g)
    gt[:, :2] = 255
    gt = gt.cuda()
    u8 = torch.empty(H, W, device="cuda", dtype=torch.uint8)
    rgb = torch.empty(H, W, 3, device="cuda", dtype=torch.uint8)
    hist, flag, ref_flag = _zeros(nc), _flag(), _flag()
    ref = _ref_hist(L, gt, pred, nc, ref_flag)
    for n in (1, 2):                                                        # from zero, then accumulated
        L.lib().wc_label_finish(_p(pred), _p(gt), _p(u8), _p(rgb), _p(hist), _p(flag), H, W, nc, L.stream())
        assert torch.equal(hist, n * ref)
    assert torch.equal(u8, pred.to(torch.uint8)) and torch.equal(rgb, table[pred]) and int(flag.item()) == 0
    # without gt: maps only; without maps: histogram only
    L.lib().wc_label_finish(_p(pred), None, _p(u8), None, None, _p(flag), H, W, nc, L.stream())
    only = _zeros(nc)
    L.lib().wc_label_finish(_p(pred), _p(gt), None, None, _p(only), _p(flag), H, W, nc, L.stream())
    assert torch.equal(only, ref) and int(flag.item()) == 0
    # a value beyond 255 (and a negative one) raises the flag and is written as 255
    wild = pred.clone()
    wild[3, 5], wild[30, 17] = 300, -1
    L.lib().wc_label_finish(_p(wild), None, _p(u8), _p(rgb), None, _p(flag), H, W, nc, L.stream())
    expect = wild.clone()
    expect[3, 5], expect[30, 17] = 255, 255
    assert torch.equal(u8, expect.to(torch.uint8)) and torch.equal(rgb, table[expect]) and int(flag.item()) == 1


def test_argument_errors_launch_nothing():
    L = _lib()
    raw = L.lib().cdll
    C, Hs, Ws, Hl, Wl, nc = 257, 2, 2, 6, 6, 300
    seg = torch.zeros(C, Hs, Ws, device="cuda")
    u8 = torch.full((Hl, Wl), 7, device="cuda", dtype=torch.uint8)
    flag = _flag()
    s = L.stream()
    none = None
    assert raw.wc_eval_finish(_p(seg), none, none, none, _p(u8), none, none, none, none, none, _p(flag), C, Hs, Ws, Hl, Wl, nc, s) == 1
    assert b"256" in raw.wc_last_error()
    assert raw.wc_eval_finish(none, none, none, none, _p(u8), none, none, none, none, none, _p(flag), 4, Hs, Ws, Hl, Wl, nc, s) == 1
    assert raw.wc_eval_finish(_p(seg), none, none, none, _p(u8), none, none, none, none, none, none, 4, Hs, Ws, Hl, Wl, nc, s) == 1
    # predm_u8 without msc; cam + gt without cam_hist
    assert raw.wc_eval_finish(_p(seg), none, none, none, none, _p(u8), none, none, none, none, _p(flag), 4, Hs, Ws, Hl, Wl, nc, s) == 1
    lab = torch.zeros(Hl, Wl, device="cuda", dtype=torch.int64)
    assert raw.wc_eval_finish(_p(seg), none, _p(lab), _p(lab), none, none, none, none, none, none, _p(flag), 4, Hs, Ws, Hl, Wl, nc, s) == 1
    assert raw.wc_label_finish(none, none, _p(u8), none, none, _p(flag), Hl, Wl, nc, s) == 1
    assert raw.wc_label_finish(_p(lab), none, _p(u8), none, none, none, Hl, Wl, nc, s) == 1
    assert raw.wc_label_finish(_p(lab), _p(lab), _p(u8), none, none, _p(flag), Hl, Wl, nc, s) == 1      # gt without hist
    with pytest.raises(RuntimeError, match="code 1"):
        L.lib().wc_label_finish(None, None, _p(u8), None, None, _p(flag), Hl, Wl, nc, s)
    torch.cuda.synchronize()
    assert bool((u8 == 7).all()) and int(flag.item()) == 0
