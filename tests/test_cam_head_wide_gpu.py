"""wc_cam_head (three wide launches: y per (image, 64 columns), soft-max part per pair, df per (pair, 64 rows)) against
wc_cam_head_single (one workgroup per pair): every output element keeps its accumulation order, so probs and df are
bit-identical -- torch.equal, no tolerance.

Shapes: the ViT-B/16 224 x 224 head (L = 197: 13 pooled chunks, the 8-unrolled chunk loop plus its remainder; E = 768, Ed = 512)
with two classes on one image and one on the other; text counts that differ per pair under a larger Tmax; ragged widths that
reach the E % 16 remainder rows, the partial last column chunk and the scalar Ed % 4 != 0 path of the df stage; E = 104, Ed = 132,
which adds the 4-row tail behind the 64-row groups of the y stage and a partial column chunk on the 16-byte df path; one pair."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32

CASES = {
    "vit-b16 two classes + one": dict(B=2, pair_img=[0, 0, 1], L=197, E=768, Ed=512, n_text=[6, 6, 6], Tmax=6),
    "n_text differs, Tmax above": dict(B=2, pair_img=[0, 0, 1], L=197, E=768, Ed=512, n_text=[3, 8, 5], Tmax=8),
    "ragged E=72 Ed=20": dict(B=2, pair_img=[0, 1, 1], L=37, E=72, Ed=20, n_text=[4, 2, 4], Tmax=4),
    "ragged E=104 Ed=132": dict(B=2, pair_img=[1, 0, 1], L=50, E=104, Ed=132, n_text=[3, 5, 2], Tmax=5),
    "one pair": dict(B=1, pair_img=[0], L=197, E=768, Ed=512, n_text=[7], Tmax=7),
}


def _inputs(B, pair_img, L, E, Ed, n_text, Tmax, seed=0):
    g = torch.Generator().manual_seed(seed)
    P = len(pair_img)
    rows = 11
    text = torch.randn(rows, Ed, generator=g)
    text = text / text.norm(dim=1, keepdim=True)
    idx = torch.stack([torch.randperm(rows, generator=g)[:Tmax] for _ in range(P)]).to(I32)
    cls = torch.tensor([int(torch.randint(0, n, (1,), generator=g)) for n in n_text], dtype=I32)
    d = dict(x2=torch.randn(B, L, E, generator=g), lnw=1 + 0.1 * torch.randn(E, generator=g), lnb=0.1 * torch.randn(E, generator=g),
             proj=torch.randn(E, Ed, generator=g) / E ** 0.5, text=text, idx=idx, n_text=torch.tensor(n_text, dtype=I32),
             img=torch.tensor(pair_img, dtype=I32), cls=cls)
    return {k: v.contiguous().cuda() for k, v in d.items()}, P


def _run(fn, d, B, P, L, E, Ed, Tmax):
    from weclip_vit_comer_amd import _lib as Lb
    dev = "cuda"
    partial = torch.empty(B * ((L + 15) // 16) * E, device=dev, dtype=F32)
    probs = torch.zeros(P, Tmax, device=dev, dtype=F32)
    df = torch.full((P, E), float("nan"), device=dev, dtype=F32)
    y = torch.full((B, Ed), float("nan"), device=dev, dtype=F32)
    dy = torch.full((P, Ed), float("nan"), device=dev, dtype=F32)
    getattr(Lb.lib(), fn)(Lb.ptr(d["x2"], F32), Lb.ptr(d["lnw"], F32), Lb.ptr(d["lnb"], F32), Lb.ptr(d["proj"], F32),
                          Lb.ptr(d["text"], F32), Lb.ptr(d["idx"], I32), Lb.ptr(d["n_text"], I32), Lb.ptr(d["img"], I32),
                          Lb.ptr(d["cls"], I32), 100.0, Lb.ptr(partial), Lb.ptr(probs), Lb.ptr(df), Lb.ptr(y), Lb.ptr(dy),
                          B, P, L, E, Ed, Tmax, Lb.stream())
    torch.cuda.synchronize()
    return probs.cpu(), df.cpu()


@pytest.mark.parametrize("name", list(CASES))
def test_wide_head_is_bit_identical_to_the_single_form(name):
    c = CASES[name]
    d, P = _inputs(**c)
    dims = (c["B"], P, c["L"], c["E"], c["Ed"], c["Tmax"])
    probs, df = _run("wc_cam_head", d, *dims)
    probs1, df1 = _run("wc_cam_head_single", d, *dims)
    assert torch.equal(probs, probs1), f"probs differ: max |d| {(probs - probs1).abs().max().item():.3g}"
    assert torch.equal(df, df1), f"df differs: max |d| {(df - df1).abs().max().item():.3g}"
    # the comparison is not between two empty results
    assert bool(torch.isfinite(df).all()) and float(df.abs().max()) > 0
    for p, n in enumerate(c["n_text"]):
        assert abs(float(probs[p, :n].sum()) - 1.0) < 1e-5 and float(probs[p, n:].abs().sum()) == 0.0
