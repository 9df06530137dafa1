"""CPU checks of the image panels (weclip_vit_comer_amd.utils.panels, csrc/panels.hip): the host colour table, the grid geometry
against hand-derived cases, the committed colour-table header against its generator, the no-CPU-fallback error, the new C
entries' declarations and the driver's --panel_iters argument."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import weclip_vit_comer_amd  # noqa: F401
from weclip_vit_comer_amd import _lib
from weclip_vit_comer_amd.utils import panels as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_colormap_equals_the_recorded_reference_table():
    table = np.load(os.path.join(ROOT, "tests", "golden", "voc_cmap.npz"))["cmap"]
    cmap = P.colormap()
    assert cmap.dtype == np.uint8 and np.array_equal(cmap, table)
    assert np.array_equal(P.colormap(N=21), table[:21])
    norm = P.colormap(normalized=True)
    assert norm.dtype == np.float32 and np.array_equal(norm, table.astype("float32") / 255)
    lab = np.array([[0, 1, 255], [15, 20, 2]], dtype=np.uint8)
    assert np.array_equal(P.encode_cmap(lab), table[lab.astype(np.int16)])
    assert P.encode_cmap(lab)[0, 2].tolist() == [224, 224, 192]


def test_grid_geometry_hand_derived():
    # make_grid(nrow=2, padding=2) of (20, 28) tiles.  B = 1: the bare image
    assert P.grid_geometry(1, 20, 28, 2) == (20, 28, 0, 0, 1, 0, False)
    # B = 3: xmaps 2, ymaps 2 (ragged last row): (22 * 2 + 2, 30 * 2 + 2), tiles at (2, 2), (2, 32), (24, 2)
    assert P.grid_geometry(3, 20, 28, 2) == (46, 62, 2, 2, 2, 2, False)
    assert P.grid_geometry(4, 20, 28, 2) == (46, 62, 2, 2, 2, 2, False)
    # nrow larger than the batch: one row of B tiles
    assert P.grid_geometry(3, 20, 28, 8) == (24, 92, 2, 2, 3, 2, False)
    # tensorboard_attn (tiles transposed before make_grid, the grid after it): 5 tiles with n_row 4 -> xmaps 4, ymaps 2, and the
    # canvas has FOUR tile rows and TWO tile columns
    assert P.grid_geometry(5, 24, 36, 4, colmajor=True) == (26 * 4 + 2, 38 * 2 + 2, 2, 2, 4, 2, True)
    assert P.grid_geometry(1, 24, 36, 4, colmajor=True) == (24, 36, 0, 0, 1, 0, True)
    with pytest.raises(ValueError):
        P.grid_geometry(0, 20, 28, 2)
    # the row tensorboard_attn shows: int(h * n_pix) * (w + 1)
    assert [P.attn_row(16, p)[0] for p in P.N_PIXS] == [0, 5, 10, 15]
    assert [P.attn_row(25, p)[0] for p in P.N_PIXS] == [0, 6, 18, 24]
    assert [P.attn_row(1024, p)[0] for p in P.N_PIXS] == [0, 9 * 33, 19 * 33, 28 * 33]


def test_committed_colour_tables_equal_the_generator():
    pytest.importorskip("matplotlib")
    spec = importlib.util.spec_from_file_location("make_cmap_tables", os.path.join(ROOT, "tools", "make_cmap_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.HEADER) as f:
        assert f.read() == mod.render()
    jet = mod.table("jet")
    assert jet.shape == (256, 3) and jet[0].tolist() == [0.0, 0.0, 127.5] and jet[255].tolist() == [127.5, 0.0, 0.0]


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        match = "CUDA"
    else:
        match = "GPU"
    with pytest.raises(RuntimeError, match=match):
        P.tensorboard_label(torch.zeros(4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=match):
        P.tensorboard_image(torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 2, 2))
    with pytest.raises(RuntimeError, match=match):
        P.tensorboard_attn([torch.zeros(1, 4, 4)])
    with pytest.raises(RuntimeError, match=match):
        P.StepSnapshot().take(torch.zeros(1, 2, 2, 2), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_panel_entries_are_declared_and_refuse_bad_arguments():
    protos = {name: args for name, _, args in _lib.parse_header()}
    grid = ["out", "canvas_h", "canvas_w", "oy", "ox", "xmaps", "pad", "colmajor", "k0", "stream"]
    assert [n for _, n in protos["wc_panel_images"]] == ["img", "mean3", "std3", "B", "H", "W"] + grid
    assert [n for _, n in protos["wc_panel_labels"]] == ["label", "is_u8", "B", "H", "W"] + grid
    assert [n for _, n in protos["wc_panel_heat"]] == ["src", "sB", "sC", "C", "h", "w", "aligned", "minmax", "cmap", "img", "mean3",
                                                       "std3", "B", "H", "W"] + grid
    assert [n for _, n in protos["wc_panel_snapshot"]] == ["seg", "n_seg", "label", "n_label", "attn", "B", "hw", "rows4", "seg_out",
                                                           "label_out", "rows_out", "stream"]
    lib = _lib.lib()
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.wc_panel_images(None, None, None, 1, 4, 4, None, 4, 4, 0, 0, 1, 0, 0, 0, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.wc_panel_snapshot(None, 0, None, 0, None, 0, 0, None, None, None, None, None)
    if torch.cuda.is_available():                         # made-up pointers stay off a machine whose launches would run
        return                                            # (tests/test_panels_gpu.py checks the same refusals on real tensors)
    import ctypes
    p = ctypes.c_void_p(64)
    with pytest.raises(RuntimeError, match="do not fit"):
        lib.wc_panel_labels(p, 1, 3, 20, 28, p, 46, 59, 2, 2, 2, 2, 0, 0, None)      # tile 1 ends at column 2 + 30 + 28 = 60
    with pytest.raises(RuntimeError, match="outside"):
        lib.wc_panel_snapshot(p, 4, p, 4, p, 1, 16, _lib.int_array([0, 5, 10, 16]), p, p, p, None)
    with pytest.raises(RuntimeError, match="aligned"):
        lib.wc_panel_snapshot(p, 4, ctypes.c_void_p(72), 4, None, 0, 0, None, p, p, None, None)


def test_panel_iters_argument():
    from weclip_vit_comer_amd import train as T
    assert T.build_parser().parse_args(["--config", "c.yaml"]).panel_iters == 0
    assert T.build_parser().parse_args(["--config", "c.yaml", "--panel_iters", "200", "--dataset", "seg"]).panel_iters == 200
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--config", "c.yaml", "--panel_iters", "often"])
