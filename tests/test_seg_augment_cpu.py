"""CPU checks of the label-aware input pipeline (data.DeviceSegAugment, csrc/augment_seg.hip): the host draw order and record
packing against the reference fixture's recorded draws, the OpenCV HSV restatement's properties, the integer acceptance rule,
the tests' own chain restatement against the fixture, and the ISA scan of the new kernel file."""
import os
import sys

import numpy as np
import pytest

import photo_ref
import segaug_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(g):
    for i in range(int(g["n_cases"])):
        yield i, int(g["group"][i]), g[f"image_{i}"], g[f"label_{i}"], [str(n) for n in g[f"draw_names_{i}"]], g[f"draw_vals_{i}"]


def _aug(group, crop):
    from weclip_vit_comer_amd.data import DeviceSegAugment
    return DeviceSegAugment(crop_size=crop, rescale_range=(0.5, 2.0) if group == 2 else None)


def test_draw_order_and_record_packing_follow_the_reference(golden):
    g = golden("seg_augment_ref.npz")
    crop = int(g["crop"])
    seen_filler = 0
    for i, group, img, lab, names, vals in _cases(g):
        aug = _aug(group, crop)
        H, W = lab.shape
        d, filled = segaug_ref.replay_draw(aug, names, vals, H, W)        # Replay asserts every generator method name in order
        seen_filler += filled
        assert aug.draw_names[:len(names)] == names
        assert aug.draw_names[len(names):] == ["randrange"] * filled and len(d[11]) == 10
        assert [list(c) for c in d[11][:len(g[f"cand_{i}"])]] == g[f"cand_{i}"].tolist()
        rec, cand = aug.pack([d])
        assert rec.shape == (1, 16) and cand.shape == (1, 10, 2) and rec.dtype == cand.dtype
        r = rec[0].numpy()
        assert r[0:1].view(np.float32)[0] == np.float32(d[0]) and r[1:7].tolist() == list(d[1:7]) and r[10] == d[10]
        assert r[7:10].view(np.float32).tolist() == [np.float32(v) for v in d[7:10]] and not r[11:].any()
        assert cand[0].tolist() == [list(c) for c in d[11]]
        # a short candidate list is filled up with its last entry
        short = d[:11] + (d[11][:3],)
        assert aug.pack([short])[1][0].tolist() == [list(c) for c in d[11][:3]] + [list(d[11][2])] * 7
    assert seen_filler > 0


def test_chain_restatement_equals_the_reference_fixture(golden):
    """tests/segaug_ref.chain (what the GPU tests compare with beyond the fixture's sizes) against the reference's outputs."""
    g = golden("seg_augment_ref.npz")
    crop = int(g["crop"])
    for i, group, img, lab, names, vals in _cases(g):
        for filler in ("min", "max"):
            d, _ = segaug_ref.replay_draw(_aug(group, crop), names, vals, *lab.shape, filler=filler)
            out, ol, box, chosen, ok = segaug_ref.chain(img, lab, d, crop)
            assert np.array_equal(out, g[f"out_{i}"]), i
            assert np.array_equal(ol, g[f"out_label_{i}"]) and np.array_equal(box, g[f"img_box_{i}"]), i
            assert chosen == len(g[f"cand_{i}"]) - 1


def test_hsv_restatement_properties():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    hsv = photo_ref.bgr2hsv(grey)
    assert not hsv[:, 0].any() and not hsv[:, 1].any() and np.array_equal(hsv[:, 2], grey[:, 0])
    assert np.array_equal(photo_ref.hsv2bgr(hsv), grey)
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)       # blue, green, red as BGR
    assert photo_ref.bgr2hsv(prim).tolist() == [[120, 255, 255], [60, 255, 255], [0, 255, 255]]
    assert np.array_equal(photo_ref.hsv2bgr(photo_ref.bgr2hsv(prim)), prim)
    # the hue wrap of PhotoMetricDistortion.hue: (h + delta) % 180 stays in [0, 180) for every 8-bit hue and delta
    h = np.arange(180)[:, None]
    d = np.arange(-18, 18)[None, :]
    w = (h + d) % 180
    assert w.min() == 0 and w.max() == 179 and w[0, 0] == 162 and w[179, 35] == 16
    assert photo_ref.bgr2hsv(photo_ref.all_colours()[::4097])[:, 0].max() < 180


def test_hsv_round_trip_error_over_all_colours():
    """BGR -> HSV -> BGR over all 2^24 colours with the 8-bit restatement.  Measured once with this file: maximum absolute
    channel error MAX_ERR, fraction of colours that survive exactly EXACT (the 8-bit HSV grid is coarser than RGB)."""
    rgb = photo_ref.all_colours()
    back = photo_ref.hsv2bgr(photo_ref.bgr2hsv(rgb))
    err = np.abs(back.astype(np.int16) - rgb.astype(np.int16)).max(axis=1)
    exact = float((err == 0).mean())
    print(f"8-bit HSV round trip: max |err| {err.max()}, exact {exact:.6f}")
    assert int(err.max()) == MAX_ERR and abs(exact - EXACT) < 1e-6


MAX_ERR, EXACT = 5, 0.310528


def test_integer_acceptance_rule_equals_the_float_ratio():
    """4 * max < 3 * sum  <=>  np.max(cnt) / np.sum(cnt) < 0.75 for every (max, sum) up to crop^2 = 4096."""
    s = np.arange(1, 4097, dtype=np.int64)[None, :]
    m = np.arange(1, 4097, dtype=np.int64)[:, None]
    valid = m <= s
    assert np.array_equal(((4 * m < 3 * s) & valid), ((m / s < 0.75) & valid))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_seg_augment_kernels_issue_their_loads_together(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_scan
    rows = isa_scan.report([os.path.join(ROOT, "weclip-vit-comer_amd", "csrc", "augment_seg.hip")], threshold=4, out_dir=str(tmp_path))
    bad = [(alone, loads, name) for alone, loads, f, name, _ in rows if not any(a in name for a in ALLOWED)]
    assert not bad, "loads waited for one at a time (see tools/isa_scan.py): %s" % bad


ALLOWED = {}
