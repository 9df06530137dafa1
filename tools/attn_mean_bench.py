"""Head-mean attention map kernel alone at the encoder shape (HIP events around back-to-back launches)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from weclip_vit_comer_amd import ops, _lib as L
B, L_, H, DH = int(os.environ.get("AB_B", 16)), int(os.environ.get("AB_L", 1025)), 12, 64
qkv = (torch.randn(B * L_, 3 * H * DH, device="cuda") * 0.5).half()
o16, lse, mean = ops.attention(qkv, B, L_, H, DH, want_mean=True)
lib = L.lib()
for _ in range(3):
    lib.wc_attn_mean(L.ptr(qkv), L.ptr(lse), L.ptr(mean), B, L_, H, DH, L.stream())
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
n = 30
e0.record()
for _ in range(n):
    lib.wc_attn_mean(L.ptr(qkv), L.ptr(lse), L.ptr(mean), B, L_, H, DH, L.stream())
e1.record(); torch.cuda.synchronize()
us = e0.elapsed_time(e1) / n * 1e3
print(f"attn_mean abl={os.environ.get('WECLIP_MEAN_ABL', '0')} B={B} L={L_}: {us:7.1f} us  {2.0 * B * H * L_ * L_ * DH / us / 1e6:7.1f} TFLOP/s", flush=True)

# `python tools/attn_mean_bench.py affw`: the affinity weight of the normal branch at this shape, eight layers -- today's eight wc_attn_mean launches +
# wc_aff_weight_c1 against ONE wc_attn_aff_weight launch (csrc/attention.hip attn_affw_kernel); both per call and per launch.
if "affw" in sys.argv[1:]:
    import ctypes
    from weclip_vit_comer_amd import cam_pipeline as CP
    NL, hw = 8, L_ - 1
    qs = [(torch.randn(B * L_, 3 * H * DH, device="cuda") * 0.5).half() for _ in range(NL)]
    ls = [ops.attention(q, B, L_, H, DH, want_mean=False)[1] for q in qs]
    maps = [torch.empty(B, L_, L_, device="cuda") for _ in range(NL)]
    wgt = torch.full((B, NL), 1.0 / NL, device="cuda")
    W, c1 = torch.empty(B, hw, hw, device="cuda"), torch.empty(B, hw, device="cuda")
    ws = torch.empty(B * ((hw + 7) // 8) * hw, device="cuda")
    marr = (ctypes.c_void_p * NL)(*[m.data_ptr() for m in maps])
    qarr = (ctypes.c_void_p * NL)(*[q.data_ptr() for q in qs])
    larr = (ctypes.c_void_p * NL)(*[x.data_ptr() for x in ls])

    def old():
        for q, x, m in zip(qs, ls, maps):
            lib.wc_attn_mean(L.ptr(q), L.ptr(x), L.ptr(m), B, L_, H, DH, L.stream())
        lib.wc_aff_weight_c1(marr, NL, L.ptr(wgt), None, L.ptr(W), L.ptr(c1), L.ptr(ws), B, L_, L.stream())

    def new():
        lib.wc_attn_aff_weight(qarr, larr, NL, L.ptr(wgt), L.ptr(W), L.ptr(c1), L.ptr(ws), B, L_, H, DH, L.stream())

    def timed(fn, n=10):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    for rnd in range(3):          # alternated
        t_old, t_new = timed(old), timed(new)
        print(f"affw B={B} L={L_} layers={NL} round {rnd}: 8 x attn_mean + aff_weight_c1 {t_old:7.1f} us ({t_old / (NL + 2):6.1f} per launch, "
              f"10 launches)   attn_aff_weight {t_new:7.1f} us (2 launches: attn_affw_kernel + aff_colreduce)   "
              f"{2.0 * B * H * NL * hw * hw * DH / t_new / 1e6:7.1f} TFLOP/s", flush=True)
