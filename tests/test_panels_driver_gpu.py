"""GPU tests of `train.py --panel_iters` on the tiny synthetic CLIP and the VOC trees of the existing driver tests (their helpers
are imported, not restated): 4 iterations at crop 64 with panels every 2, HIP graph on and off, for --dataset voc and seg, each
next to two runs without the flag.  The files and their grid shapes, the image / label / prediction / confidence / attention
panels against `utils.panels` on the kept batch and snapshot, the training thread's synchronisation warnings iteration by
iteration, model.iter_num, the trainable parameters, and that nothing happens without the flag."""
import os

import numpy as np
import pytest
import torch

import test_seg_train_driver_gpu as SD
import test_train_driver_gpu as TD

pytestmark = pytest.mark.gpu
KINDS = {"voc": TD, "seg": SD}
CASES = [(kind, graph) for kind in ("voc", "seg") for graph in (True, False)]


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("panels_driver"))
    return {kind: (tmp,) + mod._write_voc(os.path.join(tmp, kind)) for kind, mod in KINDS.items()}


@pytest.fixture(scope="module")
def once():
    o = TD._Once()
    yield o
    o.clear()


def _run(tree, kind, graph, panels, tag):
    """One Trainer over 4 iterations, `fit(until=n)` one iteration at a time under the sync counter.  `tag` tells repeated runs apart."""
    from weclip_vit_comer_amd import _lib as L
    from weclip_vit_comer_amd import train as T
    mod = KINDS[kind]
    tmp, root, lists = tree
    path, cfg = mod._cfg(tmp, root, lists, max_iters=4, log_iters=2, work=f"{kind}{int(graph)}{tag}")
    more = ["--graph" if graph else "--no-graph"] + (["--panel_iters", "2"] if panels else [])
    if kind == "voc":
        more = ["--dataset", "voc"] + more
    fns, calls = L.lib()._fn, [0]
    real = fns["wc_panel_snapshot"]

    def counted(*a):
        calls[0] += 1
        return real(*a)
    fns["wc_panel_snapshot"] = counted
    try:
        tr = T.Trainer(cfg, mod._args(path, *more), model=mod._model(), timestamp="t")
        syncs, kept = [], None
        for n in range(1, 5):
            with mod._Syncs() as s:
                tr.fit(until=n)
            syncs.append(s.n)
            if panels and n == 2:
                snap = tr.snapshot
                kept = {"imgs": tr._last_inputs.clone(), "seg": snap.seg.clone(), "label": snap.label.clone(),
                        "rows": None if snap.rows is None else snap.rows.clone()}
        assert tr.panel_writer is None                                     # fit() closed the trainer at max_iters
    finally:
        fns["wc_panel_snapshot"] = real
    return {"params": mod._params(tr.model), "iter_num": tr.model.iter_num, "syncs": syncs, "kept": kept, "work": cfg.work_dir.dir,
            "calls": calls[0], "trainer": tr}


def _runs(trees, once, kind, graph):
    """(run with --panel_iters 2, plain run, plain run again), computed once and in the order plain, panels, plain: whatever a
    process initialises lazily in its first trainer (one synchronisation warning in the first iteration) lands in a plain run."""
    plain = once(_run, trees[kind], kind, graph, False, "a")
    run = once(_run, trees[kind], kind, graph, True, "p")
    return run, plain, once(_run, trees[kind], kind, graph, False, "b")


def _png(work, n, name):
    from PIL import Image
    return torch.from_numpy(np.array(Image.open(os.path.join(work, "panels", f"iter_{n}_{name}.png")).convert("RGB"))).permute(2, 0, 1)


def _names(kind):
    return ["images", "gt_label", "prediction", "seg_conf"] if kind == "seg" else \
        ["images", "pseudo_label", "prediction", "seg_conf"] + [f"attn_pred_{j}" for j in range(4)]


@pytest.mark.parametrize("kind,graph", CASES)
def test_panel_files_and_their_contents(trees, once, kind, graph):
    from weclip_vit_comer_amd.msc_flip import resize_argmax
    from weclip_vit_comer_amd.utils import panels as P
    run = _runs(trees, once, kind, graph)[0]
    files = sorted(os.listdir(os.path.join(run["work"], "panels")))
    assert files == sorted(f"iter_{n}_{name}.png" for n in (2, 4) for name in _names(kind))
    for n in (2, 4):
        for name in _names(kind):
            # B = 2 tiles of 64 x 64 side by side; attention: 2 tiles of 224 x 224 down one column
            assert tuple(_png(run["work"], n, name).shape) == ((3, 454, 228) if name.startswith("attn") else (3, 68, 134)), name
    k = run["kept"]
    assert run["calls"] >= 1 and tuple(k["imgs"].shape) == (2, 3, 64, 64) and k["label"].dtype == torch.uint8
    conf = torch.softmax(k["seg"], dim=1)[:, 1:].contiguous()
    grid_imgs, grid_conf = P.tensorboard_image(k["imgs"], conf)
    assert torch.equal(_png(run["work"], 2, "images"), grid_imgs.cpu())
    assert torch.equal(_png(run["work"], 2, "seg_conf"), grid_conf.cpu())
    pred = torch.stack([resize_argmax(k["seg"][b].contiguous(), (64, 64)) for b in range(2)])
    assert torch.equal(_png(run["work"], 2, "prediction"), P.tensorboard_label(pred).cpu())
    assert torch.equal(_png(run["work"], 2, _names(kind)[1]), P.tensorboard_label(k["label"]).cpu())
    if kind == "voc":
        assert tuple(k["rows"].shape) == (2, 4, 16)
        for j in range(4):
            assert torch.equal(_png(run["work"], 2, f"attn_pred_{j}"), P.attn_rows_grid([k["rows"][:, j]], n_row=4).cpu())
    # the panels are pictures of something: the images differ between iterations
    assert not torch.equal(_png(run["work"], 2, "images"), _png(run["work"], 4, "images"))
    assert int(_png(run["work"], 2, "images").max()) > 0
    follows = "gt_label" if kind == "seg" else "attn_pred_0"               # painted from the snapshot alone: it followed the step
    assert not torch.equal(_png(run["work"], 2, follows), _png(run["work"], 4, follows))


@pytest.mark.parametrize("kind,graph", CASES)
def test_panels_leave_the_training_alone(trees, once, kind, graph):
    """Against two runs without the flag (same seeds): no more synchronisation warnings in any iteration than either, the same
    model.iter_num, and trainable parameters that differ from a plain run's by no more than two plain runs differ from each
    other (both printed; bit-equality when the plain runs are bit-equal)."""
    run, plain, again = _runs(trees, once, kind, graph)
    print(f"{kind} graph {graph}: sync warnings per iteration: panels {run['syncs']}, plain {plain['syncs']} and {again['syncs']}")
    assert all(p <= min(q, r) for p, q, r in zip(run["syncs"], plain["syncs"], again["syncs"]))
    assert run["iter_num"] == plain["iter_num"] == again["iter_num"]
    d_plain = (plain["params"] - again["params"]).abs().max().item()
    d_panel = (run["params"] - plain["params"]).abs().max().item()
    print(f"{kind} graph {graph}: max |parameter difference| plain vs plain {d_plain:.3e}, panels vs plain {d_panel:.3e}")
    if d_plain == 0.0:
        assert torch.equal(run["params"], plain["params"])
    else:
        assert d_panel <= d_plain


@pytest.mark.parametrize("kind,graph", CASES)
def test_without_the_flag_nothing_happens(trees, once, kind, graph):
    """No panels/ directory, no snapshot object, and `wc_panel_snapshot` was never called: the step launches what the parent's
    does (torch exposes no node count of a captured graph to compare)."""
    plain = _runs(trees, once, kind, graph)[1]
    tr = plain["trainer"]
    assert not os.path.exists(os.path.join(plain["work"], "panels"))
    assert tr.snapshot is None and tr.step.panels is None and tr.panel_iters == 0
    assert plain["calls"] == 0
    if graph:
        assert any(e["graph"] is not None for e in tr.step._graphs.values())
