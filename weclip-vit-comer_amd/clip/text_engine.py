"""CLIP text tower on the HIP path (reference clip/model.py:392-405 `encode_text`, WeCLIP_model/model_attn_aff_voc.py:34-46
`zeroshot_classifier`).

    ids --wc_text_embed--> rows (N*Lu, W) f32 + eot (N)      [one host sync: eot and the out-of-range flag]
        --12 x vit_engine.run_block(causal=True)-->          [LN / GEMMs as the vision tower, wc_attn_fwd_causal]
        --wc_text_pool--> (N, Ed) f32                          [row eot[n], ln_final, @ text_projection]

Lu = max(eot) + 1.  Under the causal mask a position attends only to itself and earlier positions, so rows 0..eot[n] of
every block output (the only rows the EOT gather reads, through their own history) do not depend on positions after
them: dropping positions >= Lu changes nothing that reaches the result.
"""
from types import SimpleNamespace

import torch

from .. import _lib as L
from .. import ops
from . import vit_engine as VE


def _ids(text, dev):
    t = torch.as_tensor(text)
    if t.dim() != 2:
        raise RuntimeError(f"encode_text: expected (N, context_length) token ids, got shape {tuple(t.shape)}")
    if t.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f"encode_text: token ids must be int32 or int64, got {t.dtype}")
    return t.to(device=dev, dtype=torch.int32).contiguous()


def run(ids, tok_emb, pos, packs, ln_w, ln_b, proj, eps=1e-5, full_context=False):
    """ids (N, Lctx) int32 CUDA; tok_emb (V, W), pos (>= Lctx, W), ln_w / ln_b (W), proj (W, Ed): f32 CUDA;
    packs: one vit_engine.BlockPack per block -> (N, Ed) f32."""
    N, Lctx = ids.shape
    if pos.shape[0] < Lctx:
        raise RuntimeError(f"encode_text: {Lctx} positions, but the positional embedding has {pos.shape[0]}")
    _, eot, bad = ops.text_embed(ids, tok_emb, pos, 0)
    flags = torch.cat([eot, bad]).cpu().tolist()          # the one host sync
    if flags[-1]:
        raise RuntimeError(f"encode_text: token ids outside [0, {tok_emb.shape[0]})")
    Lu = Lctx if full_context else max(flags[:-1]) + 1
    x, eot, _ = ops.text_embed(ids, tok_emb, pos, Lu)
    for pk in packs:
        x, _ = VE.run_block(pk, x, N, Lu, want_mean=False, causal=True)
    return ops.text_pool(x, eot, N, Lu, ln_w, ln_b, proj, eps=eps)


def _f32(p):
    return p.detach().float().contiguous()


def encode_text(model, text, full_context=False):
    """CLIP.encode_text of a clip.model.CLIP."""
    L.require_gpu()
    dev = model.token_embedding.weight.device
    if dev.type != "cuda":
        raise RuntimeError("encode_text: the model must be on the GPU (there is no CPU path)")
    tr = model.transformer
    with torch.no_grad():
        return run(_ids(text, dev), _f32(model.token_embedding.weight), _f32(model.positional_embedding),
                   [b.pack() for b in tr.resblocks], _f32(model.ln_final.weight), _f32(model.ln_final.bias),
                   _f32(model.text_projection), eps=model.ln_final.eps, full_context=full_context)


BLOCK_KEYS = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln_1.weight",
              "ln_1.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight",
              "ln_2.bias")


def packs_from_tensors(blocks, heads):
    """BlockPacks from a flat list of len(BLOCK_KEYS) tensors per block (state-dict order above)."""
    n = len(BLOCK_KEYS)
    if len(blocks) % n:
        raise RuntimeError(f"encode_text: {len(blocks)} block tensors is not a multiple of {n}")
    packs = []
    for i in range(0, len(blocks), n):
        t = dict(zip(BLOCK_KEYS, blocks[i:i + n]))
        W = t["ln_1.weight"].shape[0]
        blk = SimpleNamespace(
            attn=SimpleNamespace(embed_dim=W, num_heads=heads, in_proj_weight=t["attn.in_proj_weight"],
                                 in_proj_bias=t["attn.in_proj_bias"],
                                 out_proj=SimpleNamespace(weight=t["attn.out_proj.weight"], bias=t["attn.out_proj.bias"])),
            ln_1=SimpleNamespace(weight=t["ln_1.weight"], bias=t["ln_1.bias"]),
            ln_2=SimpleNamespace(weight=t["ln_2.weight"], bias=t["ln_2.bias"]),
            mlp=SimpleNamespace(c_fc=SimpleNamespace(weight=t["mlp.c_fc.weight"], bias=t["mlp.c_fc.bias"]),
                                c_proj=SimpleNamespace(weight=t["mlp.c_proj.weight"], bias=t["mlp.c_proj.bias"])),
            fp32_mlp=False)
        packs.append(VE.BlockPack(blk))
    return packs


def zeroshot(model, classnames, templates):
    """zeroshot_classifier with one batched encode_text for all class names x templates -> (C, Ed) f32 unit rows."""
    from .tokenizer import tokenize
    texts = [t.format(c) for c in classnames for t in templates]
    feat = model.encode_text(tokenize(texts))
    return ops.text_zeroshot(feat, len(classnames), len(templates))
