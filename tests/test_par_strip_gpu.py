"""The strip-walking form of the 16-bit PAR sweep (par_strip_kernel, csrc/par.hip) against the tile form it replaces at full
size (par_iter_kernel<CG, true, true, 8, 12>, kept in the library as the comparator) and against the fp64 evaluation of
tests/par_ref.py.

Both forms run the same FMA chain per pixel, so the masks must be bit-identical.  The shapes are the smallest at which a ring
row, a segment boundary or a clamp can go wrong: one pixel; shorter than the 24-row halo; one row / one column past it; exactly
one strip wide; a ragged second strip; more rows than the 64-row ring.  The planner gives images this small segments of at most
32 rows (4 steps), so seg_rows is set as well: 32 for interior segment boundaries at small sizes; 72 and 128 on the two tall
shapes, so that a workgroup walks 9 and 16 steps -- the ring row of the window's top wraps (twice at 128), the tap rows wrap
within a step, and the last segment is ragged (130 = 72 + 58 = 128 + 2; 257 = 3 x 72 + 41 = 2 x 128 + 1)."""
import pytest
import torch

from tests import par_ref as R
from tests import test_par_kernels_gpu as K

pytestmark = pytest.mark.gpu

DIL6 = R.DIL6
SHAPES = ((1, 1), (20, 20), (24, 25), (25, 64), (37, 100), (130, 70), (257, 129))
FORMS = (1,)
TILE, STRIP = "par_iter_kernel<{}, true, true, 8, 12>", "par_strip_kernel<{}>"


def _cg(C):
    return 2 if C <= 2 else (3 if C == 3 else 4)


class sweep_form:
    """Process-wide form of the 16-bit sweep for the calls inside the block; the default afterwards."""

    def __init__(self, form, seg_rows=0):
        self.args = (form, seg_rows)

    def __enter__(self):
        K._L().lib().wc_par_sweep_form(*self.args)

    def __exit__(self, *exc):
        K._L().lib().wc_par_sweep_form(-1, 0)


def _forward(form, seg_rows, imgd, md, n_iter, group):
    with sweep_form(form, seg_rows):
        return K.gpu_forward(imgd, md, DIL6, n_iter, group, True)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_bit_identical_to_the_tile_form(form, H, W):
    for B, group in ((5, 2), (2, 7)):
        imgd = K._dev(R.images("synth", B, H, W, seed=5))
        for C in (1, 2, 3, 4, 5):
            md = K._dev(R.masks("dense", B, C, H, W, seed=6))
            for n_iter in (1, 2, 3):
                want, names = _forward(0, 0, imgd, md, n_iter, group)
                assert TILE.format(_cg(C)) in names, names
                for seg_rows in (0, 32) + ((72, 128) if H > 64 else ()):
                    got, names = _forward(form, seg_rows, imgd, md, n_iter, group)
                    if form == 1:
                        assert STRIP.format(_cg(C)) in names, names
                    assert not any("8, 12>" in n for n in names), names
                    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
                        f"form {form} seg_rows {seg_rows} C={C} n_iter={n_iter} B={B} group={group} {H}x{W}: " \
                        f"{int((got != want).sum())} of {got.numel()} elements differ from the tile form"


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_against_fp64(form, H, W):
    """One sweep against the fp64 evaluation, inside the bound tests/test_par_kernels_gpu.py::test_h16_forward uses."""
    B = 2
    r = K.ref("synth", B, H, W, DIL6)
    imgd = K._dev(r.img)
    for C in (1, 2, 3, 4, 5):
        m = R.masks("dense", B, C, H, W, seed=3)
        out, _ = _forward(form, 0, imgd, K._dev(m), 1, B)
        want = R.sweep_terms(r.aff, m, DIL6)[0]
        K._check(f"par_strip form {form}", f"C={C} {H}x{W}", out, want, R.h16_bound(r.aff, r.amax, r.e, m, DIL6))


def test_default_form_by_work():
    """Unset, a launch with at least one 64-row segment of a strip per CU runs the strip walk and a smaller one the tile form;
    dilations above the 24-pixel halo run the tile form whatever is set."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    need = -(-cus // 3)                                                # 129 x 64: three 64-row segments of one strip per image
    for B, want in ((need - 1, TILE), (need, STRIP)):
        imgd = K._dev(R.images("synth", 1, 129, 64, seed=1)).expand(B, 3, 129, 64).contiguous()
        md = K._dev(R.masks("dense", 1, 3, 129, 64, seed=2)).expand(B, 3, 129, 64).contiguous()
        _, names = K.gpu_forward(imgd, md, DIL6, 1, B, True)
        assert want.format(3) in names, (B, names)
    far = (1, 2, 4, 8, 12, 25)
    with sweep_form(1):
        _, names = K.gpu_forward(imgd[:1].contiguous(), md[:1].contiguous(), far, 1, 1, True)
    assert TILE.format(3) in names, names


def test_graph_capture_replays_the_eager_result():
    """The ring needs more than 64 KiB of LDS, reserved at the first eager call: a captured sweep must replay what the eager call
    gives, on the masks present at replay."""
    L = K._L()
    B, C, H, W, n_iter = 2, 3, 130, 70, 3
    imgd = K._dev(R.images("synth", B, H, W, seed=7))
    m = [K._dev(R.masks("dense", B, C, H, W, seed=s)) for s in (8, 9)]
    dil = L.int_array(DIL6)
    ws = K.ws_floats(B, B, 48, H, W, True)
    md, out, tmp = torch.empty_like(m[0]), torch.empty_like(m[0]), torch.empty_like(m[0])
    aff = torch.empty(ws, dtype=torch.float32, device="cuda")

    def run():
        L.lib().wc_par_forward_h(K._p(imgd), K._p(md), K._p(out), K._p(tmp), K._p(aff), B, C, H, W, dil, 6, n_iter, B, L.stream())

    with sweep_form(1):
        eager = []
        for mk in m:
            md.copy_(mk)
            run()
            eager.append(out.clone())
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run()
        for mk, want in zip(m, eager):
            md.copy_(mk)
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "graph replay differs from the eager call"
    assert not torch.equal(eager[0], eager[1])
