"""wc_box_mask (one thread per pixel, edge-pixel box atomics, difference-array fill) against wc_box_mask_single (256 threads, every
pixel walks every box): mask_out, V and nbox are equal, and the boxes written are the same SET (their order comes from an atomic
counter in either form).  Everything is integer or a copy: no tolerance.

Per map size (32 x 32 = 1024 threads, 14 x 14 = a partial last wave, 20 x 31 = odd width) one launch of either form over these
maps, one pair each: a constant map, an all-zero map, a single pixel, a full map, isolated dots on a stride-2 grid (256 components
at 32 x 32 and 160 at 20 x 31: more than maxbox = 64, so only nbox and the mask are compared there), a one-pixel-wide spiral (the
longest label chain), two blobs that touch only diagonally (one component under 8-connectivity), a component alone in the last
column and row (an empty box), two smooth random maps, and a copy of the diagonal pair with pair_slot = -1 (writes nothing to V)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
MAXBOX = 64
NAMES = ("constant", "zero", "single pixel", "full", "dots", "spiral", "diagonal blobs", "last corner", "smooth 0", "smooth 1",
         "diagonal blobs, slot -1")


def _spiral(h, w):
    m = torch.zeros(h, w)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1.0
    while True:
        for _ in range(2):                      # straight on, else one turn to the right
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            free = 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= fy < h and 0 <= fx < w and m[fy, fx])
            if free:
                break
            dy, dx = dx, -dy
        else:
            return m
        y, x = ny, nx
        m[y, x] = 1.0


def _maps(h, w):
    from tests import affinity_ref as R
    g = torch.Generator().manual_seed(h * 100 + w)
    z = lambda: torch.zeros(h, w)
    single = z()
    single[h // 2, w // 3] = 0.9
    dots = z()
    dots[::2, ::2] = 0.5 + 0.5 * torch.rand((h + 1) // 2, (w + 1) // 2, generator=g)
    diag = z()
    diag[2:5, 2:5] = 1.0
    diag[5:8, 5:8] = 0.8
    corner = z()
    corner[h - 1, w - 1] = 1.0
    corner[1:3, 1:4] = 0.7
    smooth = R.cams_input(2, h, w, seed=h + w).reshape(2, h, w)
    maps = [torch.full((h, w), 0.5), z(), single, torch.ones(h, w), dots, _spiral(h, w), diag, corner, smooth[0], smooth[1], diag]
    return torch.stack(maps).reshape(len(maps), h * w)


def _run(fn, cams, pair_img, pair_slot, B, K, h, w):
    from weclip_vit_comer_amd import _lib as L
    Pn, hw = cams.shape
    outs = [torch.empty(n, dtype=dt, device="cuda") for n, dt in ((B * hw * K, F32), (Pn * hw, F32), (Pn * MAXBOX * 4, I32), (Pn, I32))]
    for t in outs:
        t.view(U8).fill_(255)                   # what a form leaves unwritten stays 0xFF in both
    V, mask, boxes, nbox = outs
    getattr(L.lib(), fn)(L.ptr(cams), L.ptr(pair_img), L.ptr(pair_slot), L.ptr(V), L.ptr(mask), L.ptr(boxes), L.ptr(nbox), MAXBOX,
                         Pn, h, w, K, 0.4, L.stream())
    torch.cuda.synchronize()
    return V.cpu().view(I32), mask.cpu().reshape(Pn, hw), boxes.cpu().reshape(Pn, MAXBOX, 4), nbox.cpu()


@pytest.mark.parametrize("h,w", [(32, 32), (14, 14), (20, 31)])
def test_wide_box_mask_equals_the_single_form(h, w):
    cams = _maps(h, w)
    Pn = cams.shape[0]
    assert Pn == len(NAMES)
    pair_img = torch.arange(Pn, dtype=I32)
    pair_img[-1] = 0                            # the padding pair points at image 0 and must leave it alone
    pair_slot = torch.zeros(Pn, dtype=I32)
    pair_slot[-1] = -1
    args = (cams.cuda(), pair_img.cuda(), pair_slot.cuda(), Pn - 1, 1, h, w)
    V, mask, boxes, nbox = _run("wc_box_mask", *args)
    V1, mask1, boxes1, nbox1 = _run("wc_box_mask_single", *args)
    assert torch.equal(nbox, nbox1), (nbox.tolist(), nbox1.tolist())
    assert torch.equal(V, V1), "V differs"
    for p, name in enumerate(NAMES):
        assert torch.equal(mask[p], mask1[p]), f"{name}: mask differs at {int((mask[p] != mask1[p]).sum())} pixels"
        n = int(nbox[p])
        if n <= MAXBOX:
            got, want = (sorted(tuple(int(v) for v in b[p, k]) for k in range(n)) for b in (boxes, boxes1))
            assert got == want, f"{name}: boxes differ"
            assert int((boxes[p, n:] != -1).sum()) == 0, f"{name}: something written behind the {n} boxes"
    # the maps are what their names say (and the comparison is not between two empty results)
    n = dict(zip(NAMES, nbox.tolist()))
    assert n["constant"] == n["full"] == n["single pixel"] == n["spiral"] == n["diagonal blobs"] == 1 and n["zero"] == 0
    assert n["dots"] == ((h + 1) // 2) * ((w + 1) // 2) and n["last corner"] == 2
    assert float(mask[NAMES.index("full")].sum()) == (h - 1) * (w - 1)
