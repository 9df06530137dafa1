"""Every kernel path of csrc/norm.hip and csrc/train_ops.hip against the fp64 reference of tests/trainops_ref.py, through the C ABI
(WeightCache.refresh and PolyWarmupAdamW.step, which own host logic, through themselves).

Around every call: each output and workspace is filled with 0xFF bytes (NaN) and carries a 256-element sentinel tail behind exactly
its documented size (LayerNorm backward: `part` as include/weclip_hip.h documents it); afterwards every output element is finite,
every sentinel untouched, every input bit-unchanged, every element inside the bound derived in tests/trainops_ref.py (or bit-equal
where that file says so), and a second call on fresh buffers gives the same bits.  LayerNorm rows have a mean offset and scales
over two decades, the last live row and the last four columns carry the largest dy, the gammas are sign-mixed: a wrong edge row or
column is a large error.

Cases -> paths, by the host dispatch rules:
    wc_layernorm        D <= 256: layernorm_kernel<1>: D = 4 (one live lane, all others load from the clamped index; rows 1 and 5),
                        252 (ragged), 256 (full); D <= 1024: <4>: 260 (ragged), 768, 1024 (limit); else <16>: 1028, 4096 (limit).
                        rows 5, 7, 6, 3 are no multiples of the 4 rows of a block.  Each with ldx = D and ldx = D + 8 (NaN in the
                        gap) and with the outputs y32 / y16 / y16 + lo / all three.
    wc_layernorm_bwd[_h] D <= 256: ln_bwd_kernel<4>: D = 4, 64, 252, 256; else <16>: 260, 320 (a partly filled group of four slots:
                        lanes 16 .. 63 of the second slot group are outside the row), 768, 1024 (limit).  rows 1, 15, 16, 17
                        (one group less one row, one group, one group plus a row whose 15 clamped duplicates must not count), 333;
                        rows = 768 * 16 + 37 > 768 groups: the grid-stride loop (D = 8 and 260).  fp32 and fp16 dy, add or NULL,
                        dx32 / dx16 / both.
    wc_layernorm_bwd2_h ln_bwd_kernel<4, true>: D = 4, 192, 256, the same rows.
    wc_colsum           colsum_partial_kernel<float | __half>: (1, 1); (257, 300, ld 304): two row blocks, two column blocks;
                        colsum_final_kernel: nblk = 50 > 48 enters the unrolled loop once and the remainder loop, nblk = 130 two
                        unrolled rounds.
    wc_transpose_f16    transpose_f16_kernel<float | __half>: one element; one full tile; (65, 63): two row tiles, ragged columns;
                        (75, 130) x 2 batches with the skipped-CLS source layout; oR = R and R + 5.
    wc_sigmoid_gram_bwd n % 4 == 0 (4, 64, 68, 128, 196): the vector path; else (1, 63, 130) element-wise; n > 64 (68, 128, 130,
                        196): off-diagonal tile pairs, both transposed stores.
    wc_colscale_split   C % 4 == 0 and aligned: colscale_split_kernel<4> ((80, 64)); else <1>: (1, 1), (9, 6), and (80, 64) with x
                        at a 4-byte offset.
    wc_convert_weights  (64, 64): vector rows, vector transposed; (330, 456): 6 x 8 = 48 tiles over 32 blocks (the tile loop), the
                        last row tile has r0 + 64 > R: element-wise transposed stores next to vector ones; (7, 5), (1, 21):
                        element-wise both ways; with a (3, 3) they hold 65 halves, so that (128, 64) behind them starts 2 bytes
                        past a multiple of 8 in the flat row-major buffers (asserted): C % 4 == 0 but element-wise rows, next to
                        vector transposed stores; [(68, 128), (60, 128)] stacked at row offsets 0 and 68 of one transposed copy
                        (vector rows: it lies before the odd tensors).
    wc_adamw_multi      n % 4 == 0 and 16-byte pointers: the vector form (4; 65 536 = one sweep of 64 blocks x 1024; 2 x 65 536 +
                        148: three sweeps); else the scalar form (2 x 16 384 + 5: three sweeps of 64 x 256; 4096 with grad at a
                        4-byte offset).
"""
import functools

import pytest
import torch

from tests import trainops_ref as R

pytestmark = pytest.mark.gpu

F64, F32, F16, I16, I64, U8 = torch.float64, torch.float32, torch.float16, torch.int16, torch.int64, torch.uint8
TAIL = 256
ALPHA, OUT_SCALE = R.LN_ALPHA, R.LN_OUT_SCALE


def _L():
    from weclip_vit_comer_amd import _lib as L
    return L


def _p(t):
    return _L().ptr(t)


def _dev(x):
    return x.contiguous().cuda()


def _buf(n, dtype, zero=False):
    """n elements of 0xFF bytes (zero: of zeros) and a tail of TAIL elements of 0xFF bytes."""
    t = torch.empty(n + TAIL, dtype=dtype, device="cuda")
    t.view(U8).fill_(255)
    if zero:
        t[:n] = 0
    return t


def _bits(t):
    return t.contiguous().view(-1).view(U8)


def _run(name, inputs, launch):
    """launch() -> {output: (buffer of n + TAIL elements, n) or None} on fresh buffers.  Runs it twice: sentinels, inputs
    bit-unchanged, the second call bit-identical.  -> {output: the n elements on the host, or None}."""
    keep = [t.clone() for t in inputs]
    a, b = launch(), launch()
    torch.cuda.synchronize()
    out = {}
    for k, v in a.items():
        if v is None:
            out[k] = None
            continue
        t, n = v
        assert t.numel() == n + TAIL
        bad = int((_bits(t[n:]) != 255).sum())
        assert bad == 0, f"{name}: {bad} bytes written behind the {n} elements of {k}"
        assert torch.equal(_bits(t), _bits(b[k][0])), f"{name}: a second call gives other bits in {k}"
        out[k] = t[:n].cpu()
    for t, k in zip(inputs, keep):
        assert torch.equal(_bits(t), _bits(k)), f"{name}: an input changed"
    return out


WORST = {}          # path -> worst err / bound seen


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """Prints the worst err / bound per path after the module (visible with -s)."""
    yield
    print()
    for k in sorted(WORST):
        print(f"WORST {k}: {WORST[k]:.3g}")


def _check(path, what, got, ref, bound):
    got = got.double().reshape(ref.shape)
    n = int((~torch.isfinite(got)).sum())
    assert n == 0, f"{path} {what}: {n} elements not written (still NaN) or not finite"
    err = (got - ref).abs()
    bound = bound.expand_as(err)
    ratio = (err / bound.clamp(min=1e-300)).max().item() if err.numel() else 0.0
    if (err > bound).any():
        i = int(torch.argmax((err - bound).reshape(-1)))
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ref.shape))
        raise AssertionError(f"{path} {what}: {int((err > bound).sum())} of {err.numel()} elements outside the bound, worst "
                             f"err / bound {ratio:.3g}; at {idx}: got {got.reshape(-1)[i]:.9g} ref {ref.reshape(-1)[i]:.9g}")
    WORST[path] = max(WORST.get(path, 0.0), ratio)


_INT = {F16: I16, F32: torch.int32}


def _same_bits(path, what, got, ref):
    got, ref = got.reshape(ref.shape).contiguous(), ref.contiguous()
    assert got.dtype == ref.dtype
    ne = (got.view(_INT[got.dtype]) != ref.view(_INT[ref.dtype])).reshape(-1)
    if ne.any():
        i = int(ne.nonzero()[0])
        raise AssertionError(f"{path} {what}: {int(ne.sum())} of {ne.numel()} elements differ in their bits, first at flat index "
                             f"{i}: got {got.reshape(-1)[i].item()!r} ref {ref.reshape(-1)[i].item()!r}")


def _check_pair(path, what, hi, lo, ref, b32):
    """fp16 hi (and lo) of an fp32 value within b32 of ref."""
    _check(path + " fp16", what, hi, ref, R.h_bound(ref, b32))
    if lo is not None:
        _check(path + " hi+lo", what, hi.double() + lo.double().reshape(hi.shape), ref, R.hl_bound(ref, b32))


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm forward

def ln_path(D):
    return f"layernorm_kernel<{1 if D <= 256 else (4 if D <= 1024 else 16)}>"


@pytest.mark.parametrize("rows,D", R.LN_FWD_SHAPES)
def test_layernorm_forward(rows, D):
    i = R.ln_inputs(rows, D)
    y, A = R.ln_fwd(i["x"], i["w"], i["b"])
    b32 = R.K["ln_y"] * R.EPS * A
    wd, bd = _dev(i["w"]), _dev(i["b"])
    n = rows * D
    first = None
    for ldx in (D, D + 8):
        xs = torch.full((rows, ldx), float("nan"))
        xs[:, :D] = i["x"]
        xd = _dev(xs)
        for outs in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 1, 1)):
            def launch():
                o = [(_buf(n, dt), n) if on else None for on, dt in zip(outs, (F32, F16, F16))]
                _L().lib().wc_layernorm(_p(xd), ldx, _p(wd), _p(bd), R.LN_EPS, *[_p(v[0]) if v else None for v in o], rows, D,
                                        _L().stream())
                return dict(zip(("y32", "y16", "lo"), o))
            r = _run("wc_layernorm", [xd, wd, bd], launch)
            what = f"{rows}x{D} ldx={ldx} outs={outs}"
            if r["y32"] is not None:
                _check(ln_path(D), what, r["y32"], y, b32)
            if r["y16"] is not None:
                _check_pair(ln_path(D), what, r["y16"], r["lo"], y, b32)
            if outs == (1, 1, 1):
                hi, lo = R.split16(r["y32"])
                _same_bits(ln_path(D), what + " y16 vs fp16(y32)", r["y16"], hi)
                _same_bits(ln_path(D), what + " lo vs fp16(y32 - hi)", r["lo"], lo)
                if first is None:
                    first = r
                for k in r:          # the row stride and the set of outputs change no bit
                    _same_bits(ln_path(D), what + f" {k} vs ldx = D", r[k], first[k])
            elif first is not None:
                for k in r:
                    if r[k] is not None:
                        _same_bits(ln_path(D), what + f" {k} vs all outputs", r[k], first[k])


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward

def lnb_path(D, two=False):
    return "ln_bwd_kernel<4, true>" if two else f"ln_bwd_kernel<{4 if D <= 256 else 16}>"


@functools.lru_cache(maxsize=4)
def _ln_case(rows, D):
    i = R.ln_inputs(rows, D)
    return i, {k: _dev(v) for k, v in i.items()}, {k: _dev(i[k].half()) for k in ("dy", "dyb")}


@functools.lru_cache(maxsize=8)
def _ln_ref(rows, D, two, add):
    i = _ln_case(rows, D)[0]
    return R.ln_bwd([i["dy"], i["dyb"]][:1 + two], [i["w"], i["wb"]][:1 + two], i["x"], i["add"] if add else None, alpha=ALPHA)


def gpu_ln_bwd(rows, D, f16, add, want32, want16, which="dy"):
    """One norm (gradient `which` with its gamma) -> {dx32, dx16, dgb (2, D)}."""
    _, d, h = _ln_case(rows, D)
    w = d["w" if which == "dy" else "wb"]
    dy = h[which] if f16 else d[which]
    n, npart = rows * D, (rows + 15) // 16 * 2 * D            # part as the header documents it
    fn = _L().lib().wc_layernorm_bwd_h if f16 else _L().lib().wc_layernorm_bwd

    def launch():
        dx32, dx16 = (_buf(n, F32), n) if want32 else None, (_buf(n, F16), n) if want16 else None
        part, dgb = _buf(npart, F32), _buf(2 * D, F32)
        fn(_p(dy), _p(d["x"]), _p(w), _p(d["add"]) if add else None, R.LN_EPS, _p(dx32[0]) if dx32 else None,
           _p(dx16[0]) if dx16 else None, OUT_SCALE, _p(part), _p(dgb), ALPHA, rows, D, _L().stream())
        return {"dx32": dx32, "dx16": dx16, "part": (part, npart), "dgb": (dgb, 2 * D)}
    return _run("wc_layernorm_bwd" + ("_h" if f16 else ""), [dy, d["x"], w, d["add"]], launch)


def _check_dx(path, what, r, ref):
    b32 = R.K["ln_dx"] * R.EPS * ref["A_dx"]
    if r["dx32"] is not None:
        _check(path + " dx", what, r["dx32"], ref["dx"], b32)
    if r["dx16"] is not None:
        _check(path + " dx fp16", what, r["dx16"], OUT_SCALE * ref["dx"], R.dx16_bound(ref["dx"], b32))
    if r["dx32"] is not None and r["dx16"] is not None:
        _same_bits(path, what + " dx16 vs fp16(out_scale dx32)", r["dx16"], (r["dx32"] * torch.tensor(OUT_SCALE, dtype=F32)).half())


def _check_dgb(path, what, dgb, ref, k=0):
    D = dgb.numel() // 2
    _check(path + " dgamma", what, dgb[:D], ref["dgamma"][k], R.K["ln_dgamma"] * R.EPS * ref["A_dgamma"][k])
    _check(path + " dbeta", what, dgb[D:], ref["dbeta"][k], R.K["ln_dbeta"] * R.EPS * ref["A_dbeta"][k])


def _one_norm(rows, D, combos):
    first = {}
    for f16, add, want32, want16 in combos:
        r = gpu_ln_bwd(rows, D, f16, add, want32, want16)
        ref = _ln_ref(rows, D, False, add)
        what = f"{rows}x{D} {'fp16' if f16 else 'fp32'} dy add={add} dx32={want32} dx16={want16}"
        _check_dx(lnb_path(D), what, r, ref)
        _check_dgb(lnb_path(D), what, r["dgb"], ref)
        # the form of dy (the values are the same), add and the set of outputs change no bit of what they share
        f = first.setdefault(add, {})
        for k in ("dx32", "dx16"):
            if r[k] is not None:
                _same_bits(lnb_path(D), what + f" {k} vs the first call", r[k], f.setdefault(k, r[k]))
        _same_bits(lnb_path(D), what + " dgb vs the first call", r["dgb"], first.setdefault("dgb", r["dgb"]))


ALL_COMBOS = [(f16, add, w32, w16) for f16 in (False, True) for add in (True, False) for w32, w16 in ((1, 0), (0, 1), (1, 1))]


@pytest.mark.parametrize("D", R.LN_BWD_D)
def test_layernorm_backward_one_norm(D):
    for rows in R.LN_BWD_ROWS:
        _one_norm(rows, D, ALL_COMBOS)


@pytest.mark.parametrize("rows,D", R.LN_BWD_GRID)
def test_layernorm_backward_one_norm_grid_stride(rows, D):
    assert (rows + 15) // 16 > 768
    _one_norm(rows, D, [(False, True, 1, 1), (True, False, 1, 1), (True, True, 0, 1), (False, False, 1, 0)])


@pytest.mark.parametrize("D", R.LN_BWD2_D)
@pytest.mark.parametrize("rows", R.LN_BWD_ROWS + (R.LN_GRID_ROWS,))
def test_layernorm_backward_two_norms(rows, D):
    _, d, h = _ln_case(rows, D)
    n, npart = rows * D, min((rows + 15) // 16, 2048) * 4 * D
    combos = ALL_COMBOS[6:] if rows < 1000 else [(True, True, 1, 1), (True, False, 0, 1)]
    for _, add, want32, want16 in combos:
        def launch():
            dx32, dx16 = (_buf(n, F32), n) if want32 else None, (_buf(n, F16), n) if want16 else None
            part, ga, gb = _buf(npart, F32), _buf(2 * D, F32), _buf(2 * D, F32)
            _L().lib().wc_layernorm_bwd2_h(_p(h["dy"]), _p(d["w"]), _p(h["dyb"]), _p(d["wb"]), _p(d["x"]), _p(d["add"]) if add else None,
                                           R.LN_EPS, _p(dx32[0]) if dx32 else None, _p(dx16[0]) if dx16 else None, OUT_SCALE, _p(part),
                                           _p(ga), _p(gb), ALPHA, rows, D, _L().stream())
            return {"dx32": dx32, "dx16": dx16, "part": (part, npart), "dgba": (ga, 2 * D), "dgbb": (gb, 2 * D)}
        r = _run("wc_layernorm_bwd2_h", [h["dy"], h["dyb"], d["w"], d["wb"], d["x"], d["add"]], launch)
        ref = _ln_ref(rows, D, True, add)
        what = f"{rows}x{D} add={add} dx32={want32} dx16={want16}"
        _check_dx(lnb_path(D, True), what, r, ref)
        _check_dgb(lnb_path(D, True), what, r["dgba"], ref, 0)
        _check_dgb(lnb_path(D, True), what, r["dgbb"], ref, 1)
    # the four column sums are those of the one-norm kernel, bit for bit (the same summation order per norm)
    one_a = gpu_ln_bwd(rows, D, True, False, 0, 1, "dy")["dgb"]
    one_b = gpu_ln_bwd(rows, D, True, False, 0, 1, "dyb")["dgb"]
    _same_bits(lnb_path(D, True), f"{rows}x{D} dgba vs the one-norm kernel", r["dgba"], one_a)
    _same_bits(lnb_path(D, True), f"{rows}x{D} dgbb vs the one-norm kernel", r["dgbb"], one_b)


# ---------------------------------------------------------------------------------------------------------------------
# column sum

@pytest.mark.parametrize("Rr,C,ld", R.COLSUM_SHAPES)
def test_colsum(Rr, C, ld):
    src = R.colsum_input(Rr, C, ld)
    nblk = (Rr + 255) // 256
    for f32 in (True, False):
        sd = _dev(src if f32 else src.half())
        path = f"colsum_partial_kernel<{'float' if f32 else '__half'}>"
        for alpha, round16 in R.colsum_cases(Rr):
            s, A = R.colsum(src[:, :C], alpha)
            b32 = R.K["colsum"] * R.EPS * A
            def launch():
                part, out = _buf(nblk * C, F32), _buf(C, F32)
                _L().lib().wc_colsum(_p(sd), 1 if f32 else 0, ld, _p(part), _p(out), Rr, C, alpha, round16, _L().stream())
                return {"part": (part, nblk * C), "out": (out, C)}
            r = _run("wc_colsum", [sd], launch)
            what = f"R={Rr} C={C} ld={ld} alpha={alpha} round16={round16}"
            assert torch.isfinite(r["part"]).all(), f"{path} {what}: partial sums not written"
            if round16:
                _check(path + " round16", what, r["out"], s, R.h_bound(s, b32))
                _same_bits(path, what + " out is an fp16 value", r["out"], r["out"].half().float())
            else:
                _check(path, what, r["out"], s, b32)


# ---------------------------------------------------------------------------------------------------------------------
# transpose: bit-exact

@pytest.mark.parametrize("Rr,C,batch", R.TRANSPOSE_SHAPES)
def test_transpose(Rr, C, batch):
    full = R.weight_values((batch, Rr + 1, C), seed=3)
    full[:, 0] = float("nan")                                     # the CLS row of every batch, skipped through src and sSrc
    for f32 in (True, False):
        fd = _dev(full if f32 else full.half()).view(-1)
        srcd = fd[C:]
        live = (full if f32 else full.half())[:, 1:]
        for oR in (Rr, Rr + 5):
            ldo = ((batch - 1) * oR + Rr + 63) // 64 * 64
            for scale in (1.0, 0.25):
                hi, lo = R.transpose(live, oR, scale)
                want = [torch.zeros(C, ldo, dtype=F16) for _ in range(2)]
                want[0][:, :hi.shape[1]], want[1][:, :lo.shape[1]] = hi, lo
                for with_lo in (True, False):
                    def launch():
                        h, l = _buf(C * ldo, F16, zero=True), _buf(C * ldo, F16, zero=True) if with_lo else None
                        _L().lib().wc_transpose_f16(_p(srcd), 1 if f32 else 0, C, (Rr + 1) * C, _p(h), _p(l) if with_lo else None, ldo, oR,
                                                    batch, Rr, C, scale, _L().stream())
                        return {"hi": (h, C * ldo), "lo": (l, C * ldo) if with_lo else None}
                    r = _run("wc_transpose_f16", [fd], launch)
                    path = f"transpose_f16_kernel<{'float' if f32 else '__half'}>"
                    what = f"R={Rr} C={C} batch={batch} oR={oR} scale={scale}"
                    _same_bits(path, what + " hi", r["hi"], want[0])
                    WORST.setdefault(path + " (bit-equal)", 0.0)
                    if with_lo:
                        _same_bits(path, what + " lo", r["lo"], want[1])


# ---------------------------------------------------------------------------------------------------------------------
# sigmoid-Gram backward

@pytest.mark.parametrize("n", R.GRAM_N)
def test_sigmoid_gram_backward(n):
    B = 2
    dAP, AP = R.gram_inputs(B, n)
    dd, ad = _dev(dAP), _dev(AP)
    path = "sigmoid_gram_bwd_kernel (" + ("vector" if n % 4 == 0 else "element-wise") + (", off-diagonal tiles)" if n > 64 else ")")
    c64 = (n + 63) // 64 * 64
    for ldo in (c64, c64 + 64) if n in (63, 64) else (c64,):
        for scale in (1.0, 0.5):
            S, A = R.gram(dAP, AP, scale)
            b32 = R.K["gram"] * R.EPS * A
            for with_lo in (True, False):
                def launch():
                    h, l = _buf(B * n * ldo, F16), _buf(B * n * ldo, F16) if with_lo else None
                    _L().lib().wc_sigmoid_gram_bwd(_p(dd), _p(ad), _p(h), _p(l) if with_lo else None, B, n, ldo, scale, _L().stream())
                    return {"hi": (h, B * n * ldo), "lo": (l, B * n * ldo) if with_lo else None}
                r = _run("wc_sigmoid_gram_bwd", [dd, ad], launch)
                what = f"n={n} ldo={ldo} scale={scale} lo={with_lo}"
                hi = r["hi"].view(B, n, ldo)
                lo = r["lo"].view(B, n, ldo) if with_lo else None
                _check_pair(path, what, hi[:, :, :n], lo[:, :, :n] if with_lo else None, S, b32)
                for name, t in (("hi", hi), ("lo", lo)):
                    if t is None:
                        continue
                    assert (t[:, :, n:].contiguous().view(I16) == -1).all(), f"{path} {what}: {name} columns [n, ldo) written"
                    _same_bits(path, what + f" {name} symmetric", t[:, :, :n].contiguous(), t[:, :, :n].transpose(1, 2).contiguous())


# ---------------------------------------------------------------------------------------------------------------------
# column-scale split

@pytest.mark.parametrize("rows,C,rpb,off", R.COLSCALE_SHAPES)
def test_colscale_split(rows, C, rpb, off):
    x, cs = R.colscale_inputs(rows, C, rpb)
    n = rows * C
    xbuf = torch.zeros(n + 4, device="cuda")
    xd = xbuf[off:off + n]
    xd.copy_(x.view(-1))
    csd = _dev(cs)
    vec = C % 4 == 0 and off == 0
    path = f"colscale_split_kernel<{4 if vec else 1}>"
    for use_cs in (True, False):
        for alpha in (1.0, -0.5):
            y, A = R.colscale(x, cs if use_cs else None, rpb, alpha)
            exact = not use_cs and alpha == 1.0
            b32 = R.K["colscale"] * R.EPS * A
            for w32 in (True, False):
                for with_lo in (True, False):
                    def launch():
                        o, h, l = _buf(n, F32) if w32 else None, _buf(n, F16), _buf(n, F16) if with_lo else None
                        _L().lib().wc_colscale_split(_p(xd), _p(csd) if use_cs else None, _p(o) if w32 else None, _p(h),
                                                     _p(l) if with_lo else None, rows, C, rpb, alpha, _L().stream())
                        return {"out32": (o, n) if w32 else None, "hi": (h, n), "lo": (l, n) if with_lo else None}
                    r = _run("wc_colscale_split", [xbuf, csd], launch)
                    what = f"{rows}x{C} rpb={rpb} off={off} cs={use_cs} alpha={alpha} out32={w32} lo={with_lo}"
                    if w32:
                        _check(path, what, r["out32"], y, b32)
                        h, l = R.split16(r["out32"])
                        _same_bits(path, what + " hi vs fp16(out32)", r["hi"], h)
                        if with_lo:
                            _same_bits(path, what + " lo vs fp16(out32 - hi)", r["lo"], l)
                    _check_pair(path, what, r["hi"].view(rows, C), r["lo"].view(rows, C) if with_lo else None, y, b32)
                    if exact:
                        h, l = R.split16(x)
                        _same_bits(path, what + " hi", r["hi"], h.view(-1))
                        if w32:
                            _same_bits(path, what + " out32", r["out32"], x.view(-1))
                        if with_lo:
                            _same_bits(path, what + " lo", r["lo"], l.view(-1))


# ---------------------------------------------------------------------------------------------------------------------
# weight conversion, through WeightCache.refresh: bit-exact

# in the order of the flat row-major buffers: "sq", "big" and "stack" start at multiples of 8 bytes (vector rows); "odd", "row" and
# "odd3" hold 35 + 21 + 9 = 65 halves, so that "after" starts 2 bytes past a multiple of 8 (35 + 21 alone is a multiple of 4
# halves: without "odd3" it would be aligned again)
WEIGHTS = (("sq", [(64, 64)]), ("big", [(330, 456)]), ("stack", [(68, 128), (60, 128)]), ("odd", [(7, 5)]), ("row", [(1, 21)]),
           ("odd3", [(3, 3)]), ("after", [(128, 64)]))


@pytest.mark.parametrize("exact", [True, False])
def test_weight_conversion(exact):
    from weclip_vit_comer_amd import ops
    host = {n: [R.weight_values(s, seed=k) for k, s in enumerate(shapes)] for n, shapes in WEIGHTS}
    dev = {n: [_dev(t) for t in ts] for n, ts in host.items()}
    named = [(n, dev[n][0] if len(dev[n]) == 1 else dev[n]) for n, _ in WEIGHTS]
    lo_names = ("after",)
    wc = ops.WeightCache()

    def check(tag):
        torch.cuda.synchronize()
        for n, _ in WEIGHTS:
            hi, lo, hiT, loT = R.convert_weights(host[n])
            w, (wT, ldT) = wc.w(n), wc.wT(n)
            what = f"{tag} {n} exact={exact}"
            assert ldT == hiT.shape[1] and tuple(wT.hi.shape) == tuple(hiT.shape)
            _same_bits("convert_weights_kernel", what + " hi", w.hi.cpu(), hi)
            _same_bits("convert_weights_kernel", what + " hiT (padding zero)", wT.hi.cpu(), hiT)
            assert (w.lo is not None) == (exact or n in lo_names) and (wT.lo is not None) == exact
            if w.lo is not None:
                _same_bits("convert_weights_kernel", what + " lo", w.lo.cpu(), lo)
            if wT.lo is not None:
                _same_bits("convert_weights_kernel", what + " loT (padding zero)", wT.lo.cpu(), loT)
        for n in dev:
            for t, h in zip(dev[n], host[n]):
                _same_bits("convert_weights_kernel", f"{tag} source {n}", t.cpu(), h)

    def poison():
        """NaN in every row-major element and every live transposed one (the padding is never written: it stays zero)."""
        wc.hi.view(U8).fill_(255)
        if wc.lo is not None:
            wc.lo.view(U8).fill_(255)
        for n, _ in WEIGHTS:
            Rr = sum(t.shape[0] for t in host[n])
            wT = wc.wT(n)[0]
            wT.hi[:, :Rr] = float("nan")
            if wT.lo is not None:
                wT.lo[:, :Rr] = float("nan")

    wc.refresh(named, exact, lo_names=lo_names)
    # the dispatch of convert_weights_kernel, mirrored: vector rows need src % 16 == 0, hi % 8 == 0 and lo % 8 == 0
    for n in ("sq", "big", "stack"):
        assert wc.w(n).hi.data_ptr() % 8 == 0 and (wc.w(n).lo is None or wc.w(n).lo.data_ptr() % 8 == 0), n
        assert all(t.data_ptr() % 16 == 0 for t in dev[n])
    after = wc.w("after")
    assert after.hi.data_ptr() % 8 == 2 and after.lo.data_ptr() % 8 == 2, "`after` must take the element-wise rows (C % 4 == 0)"
    assert wc.wT("after")[0].hi.data_ptr() % 8 == 0, "... next to vector transposed stores"
    assert wc.w("row").hi.data_ptr() % 8 != 0
    check("first")
    poison()
    wc.refresh(named, exact, lo_names=lo_names)               # no version counter moved: no launch
    torch.cuda.synchronize()
    assert torch.isnan(wc.hi).all() and torch.isnan(wc.wT("big")[0].hi[:, :330]).all(), "converted although nothing changed"
    dev["odd"][0].mul_(-3.0)                                  # one in-place update: one launch converts everything
    host["odd"][0] = host["odd"][0] * -3.0
    wc.refresh(named, exact, lo_names=lo_names)
    check("after an in-place update")
    poison()
    wc.refresh(named, exact, lo_names=lo_names)
    torch.cuda.synchronize()
    assert torch.isnan(wc.hi).all()
    wc.refresh(named, exact, force=True, lo_names=lo_names)
    check("forced")
    WORST.setdefault("convert_weights_kernel (bit-equal)", 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# AdamW

def _adamw_path(k):
    return "adamw_multi_kernel (" + ("vector" if k < 3 else "scalar") + ")"


def _adamw_check(tag, got, ref_in, step, grp):
    """got: per tensor (p, m, v) on the host after the step; ref_in: per tensor (p, g, m, v) before it."""
    for k, ((p, m, v), before) in enumerate(zip(got, ref_in)):
        ref = R.adamw(*before, step, **grp)
        for j, (name, t) in enumerate((("p", p), ("m", m), ("v", v))):
            _check(f"{_adamw_path(k)} {name}", f"{tag} n={t.numel()}", t, ref[j], R.K["adamw_" + name] * R.EPS * ref[3 + j])


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("gi", [0, 1])
def test_adamw_one_step(gi, step):
    grp = R.ADAMW_GROUPS[gi]
    host = [R.adamw_inputs(n, seed=gi) for n in R.ADAMW_SIZES]
    gd = []
    for k, (p, g, m, v) in enumerate(host):
        off = 1 if k == 4 else 0                              # the last tensor's grad: a view at a 4-byte offset
        gb = torch.zeros(g.numel() + 4, device="cuda")
        gb[off:off + g.numel()] = g.cuda()
        gd.append(gb[off:off + g.numel()])
        assert gd[-1].data_ptr() % 16 == 4 * off
    b1, b2 = R.ADAMW_BETAS

    def launch():
        bufs, rows = {}, []
        for k, (p, g, m, v) in enumerate(host):
            n = p.numel()
            row = []
            for name, t in (("p", p), ("m", m), ("v", v)):
                b = _buf(n, F32)
                b[:n] = t.cuda()
                bufs[f"{name}{k}"] = (b, n)
                row.append(b.data_ptr())
            rows.append([row[0], gd[k].data_ptr(), row[1], row[2], n, 0, 0, 0])
        table = torch.tensor(rows, dtype=I64).cuda()
        _L().lib().wc_adamw_multi(_p(table), len(rows), grp["lr"], b1, b2, R.ADAMW_EPS, grp["weight_decay"], 1.0 - b1 ** step,
                                  1.0 - b2 ** step, 64, _L().stream())
        torch.cuda.synchronize()
        return bufs
    r = _run("wc_adamw_multi", gd, launch)
    _adamw_check(f"group {gi} step {step}", [(r[f"p{k}"], r[f"m{k}"], r[f"v{k}"]) for k in range(len(host))], host, step, grp)


def test_poly_warmup_adamw_five_steps():
    """Five steps of PolyWarmupAdamW (warm-up, then polynomial decay) on the same sizes in two groups.  Every step is checked on
    its own: the fp64 reference takes the step from the state the device held before it (read back bit for bit), with the lr of
    the same schedule, so that the one-step bound applies to every step.  After the fifth step the device state is also compared
    with an fp64 trajectory stepped on its own from the initial state, within the bound R.adamw_drift carries along it."""
    from weclip_vit_comer_amd.utils.optimizer import PolyWarmupAdamW
    host = [R.adamw_inputs(n, seed=5) for n in R.ADAMW_SIZES]
    ps = [torch.nn.Parameter(p.cuda()) for p, _, _, _ in host]
    split = (0, 1, 0, 1, 1)
    groups = [dict(params=[p for p, s in zip(ps, split) if s == gi], **R.ADAMW_GROUPS[gi]) for gi in (0, 1)]
    sched = dict(warmup_iter=2, warmup_ratio=1e-3, max_iter=50, power=0.9)
    opt = PolyWarmupAdamW(groups, lr=1e-3, weight_decay=0.01, betas=list(R.ADAMW_BETAS), **sched)
    gbuf = torch.zeros(R.ADAMW_SIZES[4] + 4, device="cuda")
    traj = [(p.double(), torch.zeros(p.numel(), dtype=F64), torch.zeros(p.numel(), dtype=F64)) for p, _, _, _ in host]
    drift = [tuple(torch.zeros(p.numel(), dtype=F64) for _ in range(3)) for p, _, _, _ in host]
    for it in range(5):
        gen = torch.Generator().manual_seed(100 + it)
        grads = []
        for k, p in enumerate(ps):
            g = torch.randn(p.numel(), generator=gen) * (0.1 + it)
            g[it::7] = 0.0
            if k == 4:
                gbuf[1:1 + g.numel()] = g.cuda()
                p.grad = gbuf[1:1 + g.numel()]
                assert p.grad.data_ptr() % 16 == 4
            else:
                p.grad = g.cuda()
            grads.append(g)
        before = []
        for k, p in enumerate(ps):
            st = opt.state[p]
            m, v = (st[n].cpu() for n in ("exp_avg", "exp_avg_sq")) if len(st) else (torch.zeros(p.numel()), torch.zeros(p.numel()))
            before.append((p.detach().cpu(), grads[k], m, v))
        assert opt._hip_ok()
        opt.step()
        torch.cuda.synchronize()
        mult = R.poly_lr_mult(it, **sched)
        for gi in (0, 1):
            grp = dict(R.ADAMW_GROUPS[gi], lr=R.ADAMW_GROUPS[gi]["lr"] * mult)
            assert opt.param_groups[gi]["lr"] == grp["lr"]
            idx = [k for k, s in enumerate(split) if s == gi]
            got = [(ps[k].detach().cpu(), opt.state[ps[k]]["exp_avg"].cpu(), opt.state[ps[k]]["exp_avg_sq"].cpu()) for k in idx]
            for k, gt in zip(idx, got):
                assert float(opt.state[ps[k]]["step"]) == it + 1
                ref = R.adamw(*before[k], it + 1, **grp)
                for j, name in enumerate(("p", "m", "v")):
                    _check(f"{_adamw_path(k)} {name}", f"PolyWarmupAdamW step {it + 1} n={gt[j].numel()}", gt[j], ref[j],
                           R.K["adamw_" + name] * R.EPS * ref[3 + j])
            for k in idx:
                _same_bits("adamw_multi_kernel", f"step {it + 1}: grad of tensor {k}", ps[k].grad.cpu(), grads[k])
                traj[k], drift[k] = R.adamw_drift(drift[k], traj[k], grads[k], it + 1, **grp)
    for k, p in enumerate(ps):
        got = (p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu())
        for j, name in enumerate(("p", "m", "v")):
            _check(f"PolyWarmupAdamW five steps, {_adamw_path(k)} {name}", f"n={p.numel()}", got[j], traj[k][j], drift[k][j])
