"""`WeCLIP` fully supervised variant (reference WeCLIP_model/model_attn_aff_voc_seg.py:56-125): frozen CLIP ViT encoder
(the 11 blocks whose outputs feed the adapters) -> adapters -> decoder -> seg.  No head-mean attention maps, no 12th
block, no GradCAM, no affinity and no PAR; labels are ground-truth masks, so the model trains on a plain cross-entropy
(train_step.SupervisedTrainStep, utils.losses.get_ce_loss_fused).

The head runs on the HIP engine in its seg-only mode (head_engine.HeadEngine(attn_pred=False): no Gram product
sigmoid(F^T F), no fp16 copy of F); `WECLIP_HEAD=torch` runs the module head through stock autograd instead (A/B path).
State dict: `encoder.*`, `decoder_fts_fuse.*`, `decoder.*` -- the reference's keys, so its checkpoints load strict."""
import os

import torch
import torch.nn as nn

from ..clip import vit_engine as VE
from ..clip.clip import load as clip_load
from ..head_engine import HeadEngine, HeadFunction
from ..pytorch_grad_cam import GradCAM
from .Decoder.TransDecoder_seg import DecoderTransformer
from .model_attn_aff_voc import TEMPLATES, default_text_features, reshape_transform, zeroshot_classifier  # noqa: F401
from .segformer_head_seg import SegFormerHead


def _drop_derived_keys(state_dict, prefix, *args):
    """The reference's VisionTransformer.forward stores its resized positional embedding as a module attribute
    (clip/model.py:266), so a checkpoint it saves after any forward carries `encoder.visual.positional_embedding_new`:
    derived from positional_embedding and the last input size, recomputed by every forward here -- dropped on load."""
    state_dict.pop(prefix + "encoder.visual.positional_embedding_new", None)


class WeCLIP(nn.Module):
    fg_names, bg_names = "new_class_names", "BACKGROUND_CATEGORY"      # clip.clip_text lists of the text rows (:76-79)
    val_runs_cam = False        # no CAM leg at all, and
    val_logits_only = True      # forward takes no `labels` and returns the logits tensor alone (validate.Validator reads both)

    def __init__(self, num_classes=None, clip_model=None, embedding_dim=256, in_channels=512, dataset_root_path=None,
                 device="cuda", text_features=None):
        """`text_features=(bg, fg)`: the zero-shot text rows, computed like the VOC model does when omitted and the
        reference checkout is known, else None.  forward never reads them (API parity with the reference :76-79)."""
        super().__init__()
        self.num_classes, self.embedding_dim, self.in_channels = num_classes, embedding_dim, in_channels
        self.encoder, _ = clip_load(clip_model, device=device)
        for p in self.encoder.parameters():
            p.requires_grad = False                              # reference :64-65: the whole encoder is frozen
        self.decoder_fts_fuse = SegFormerHead(in_channels=in_channels, embedding_dim=embedding_dim,
                                              num_classes=num_classes, index=11)
        self.decoder = DecoderTransformer(width=embedding_dim, layers=3, heads=8, output_dim=num_classes)
        if text_features is None:
            text_features = default_text_features(self.encoder, self.fg_names, self.bg_names)
        self.bg_text_features, self.fg_text_features = (None, None) if text_features is None else text_features
        self.target_layers = [self.encoder.visual.transformer.resblocks[-1].ln_1]
        self.grad_cam = GradCAM(model=self.encoder, target_layers=self.target_layers,
                                reshape_transform=reshape_transform)
        self.root_path = os.path.join(dataset_root_path, "JPEGImages") if dataset_root_path else None
        self.cam_bg_thres = 1
        self.encoder.eval()
        self.iter_num = 0
        self.require_all_fts = True
        self.head_impl = os.environ.get("WECLIP_HEAD", "hip")   # "hip" (head_engine.py, seg-only) | "torch" (stock autograd)
        self.head_engine = HeadEngine(self.decoder_fts_fuse, self.decoder, attn_pred=False)
        self._register_load_state_dict_pre_hook(_drop_derived_keys)
        self.to(device)

    def get_param_groups(self):
        groups = [[], [], [], []]   # backbone; backbone_norm; cls_head; seg_head
        groups[3].extend(self.decoder.parameters())
        groups[3].extend(self.decoder_fts_fuse.parameters())
        return groups

    def encode(self, img, x16=None):
        """Frozen encoder: token rows of blocks 1..11 (the adapters' inputs), no head-mean maps.  `x16` (a list)
        additionally receives fp16 copies of the block outputs (the HIP head's operands)."""
        xs, _, B, Lq = VE.encode_blocks(self.encoder.visual, img, [False] * 11, x16)
        return xs, B, Lq

    def forward(self, img, img_names="2007_000032", mode="train"):
        """-> seg (B, nc, H/16, W/16) f32 (reference :101-125; `img_names` and `mode` are accepted for API parity)."""
        B, _, H, W = img.shape
        h, w = H // 16, W // 16
        self.encoder.eval()
        self.iter_num += 1
        img = img.cuda().float().contiguous()
        hip_head = self.head_impl == "hip"
        x16 = VE.X16Stack(self.encoder.visual.transformer.layers - 1) if hip_head else None
        with torch.no_grad():
            xs, _, Lq = self.encode(img, x16)
        if hip_head:
            drop = self.head_engine.draw_dropout(B, img.device) if self.training else None
            seg, _ = HeadFunction.apply(self.head_engine, x16, B, Lq, h, w, drop, *self.head_engine.params())
            return seg
        fts = self.decoder_fts_fuse.forward_rows(xs, B, Lq, h, w)
        seg, _ = self.decoder(fts, need_weights=False)
        return seg
