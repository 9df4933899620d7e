"""The DeepEncoder runtime of the vision path (deepencoder/deepencoder_infer.py:149-189, 195-278, 376-587): camera files -> [256, 2048]
vision tokens per view, through the SAM ViT-B tower (vision_tower), the CLIP-L tower (clip_tower) and the 2048 -> 2048 projector.

  resize_and_pad_to_square / _pil_to_tensor_og_norm      host image preparation (PIL is imported inside them)
  DEFAULT_VIEW_ORDER / FIXED_IMAGE_SIZE / FIXED_GRID_SIDE / resolve_cam_image_paths(nusc, sample_token)   duck-typed on nusc.get / nusc.dataroot
  load_openclip_state_dict(vit, sd)                       the reference's CLIP ViT-L/14 key mapping on a state dict the caller holds
  DeepEncoderRuntime(sam_ckpt=None, ...)                  eval(), encode_pixels(x), encode_image(path), encode_views(paths, strict=, view_order=)
  multiview_tokens_from_sample_token(sample_token, nusc, runtime=...)

The join moves no activation with torch.  lvq_clip_embed hands SAM's channel-major features back as the token-major bf16 operand, and
the projector runs as two K = 1024 products over the two column halves of its weight (ldw = 2048): the CLIP half on the tower's output
rows with the class row skipped by the batch stride, the SAM half on that operand with the first product as its fp32 residual --
cat(clip[:, 1:], sam^T) @ W^T + b without the [B, HW, 2048] concatenation.  encode_views runs the views that are present as ONE batch.

This package never reaches the network: there is no checkpoint download and no model fetched by name.  `auto_download_sam` and
`openclip_pretrained` are accepted for signature compatibility and ignored (one warning); with sam_ckpt=None the towers keep their default
initialisation, a path that does not exist raises FileNotFoundError, and CLIP weights come from load_openclip_state_dict on a state dict
loaded by the caller.  Inference only: train(), lora_config.enabled and trainable_parameters() raise LvqError.
"""
from __future__ import annotations

import warnings
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _ffi as F
from . import ops as O
from .clip_tower import VitModel, build_clip_l
from .fusion import MlpProjectorLinear
from .vision_tower import build_sam_vit_b

FIXED_IMAGE_SIZE = 1024
FIXED_GRID_SIDE = 16
DEFAULT_VIEW_ORDER: Tuple[str, ...] = ("CAM_FRONT", "CAM_FRONT_RIGHT", "CAM_FRONT_LEFT", "CAM_BACK", "CAM_BACK_RIGHT", "CAM_BACK_LEFT")


# ------------------------------------------------------------------------------------------------------------------------------------
# image preparation (host)
# ------------------------------------------------------------------------------------------------------------------------------------
def resize_and_pad_to_square(im, target: int = FIXED_IMAGE_SIZE):
    """Aspect-preserving LANCZOS resize into target x target, centred on a black canvas (no stretching)."""
    from PIL import Image
    if im.mode != "RGB":
        im = im.convert("RGB")
    w, h = im.size
    scale = min(target / w, target / h)
    new_w, new_h = min(int(round(w * scale)), target), min(int(round(h * scale)), target)
    resized = im.resize((new_w, new_h), Image.Resampling.LANCZOS)
    canvas = Image.new("RGB", (target, target), color=0)
    canvas.paste(resized, ((target - new_w) // 2, (target - new_h) // 2))
    return canvas


def _pil_to_tensor_og_norm(im) -> torch.Tensor:
    """PIL RGB -> fp32 [1, 3, H, W] in [-1, 1]: x / 255, then (x - 0.5) / 0.5."""
    if im.mode != "RGB":
        im = im.convert("RGB")
    arr = np.array(im).astype(np.float32) / 255.0
    t = torch.from_numpy(arr).permute(2, 0, 1).unsqueeze(0)
    return (t - 0.5) / 0.5


def resolve_cam_image_paths(nusc, sample_token: str, view_order: Sequence[str] = DEFAULT_VIEW_ORDER) -> List[Optional[Path]]:
    """Absolute image paths of the views of a nuScenes sample; None for a view the sample lacks or whose file is missing."""
    sample = nusc.get("sample", sample_token)
    out: List[Optional[Path]] = []
    for cam in view_order:
        sd_tok = sample["data"].get(cam, None)
        if not sd_tok:
            out.append(None)
            continue
        sd = nusc.get("sample_data", sd_tok)
        p = (Path(nusc.dataroot) / sd["filename"]).resolve()
        out.append(p if p.exists() else None)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# CLIP ViT-L/14 weights from an OpenCLIP `visual` state dict the caller already holds
# ------------------------------------------------------------------------------------------------------------------------------------
_BLOCK_KEYS = (("attn.in_proj_weight", "self_attn.qkv_proj.weight"), ("attn.in_proj_bias", "self_attn.qkv_proj.bias"),
               ("attn.out_proj.weight", "self_attn.out_proj.weight"), ("attn.out_proj.bias", "self_attn.out_proj.bias"),
               ("mlp.c_fc.weight", "mlp.fc1.weight"), ("mlp.c_fc.bias", "mlp.fc1.bias"), ("mlp.c_proj.weight", "mlp.fc2.weight"),
               ("mlp.c_proj.bias", "mlp.fc2.bias"), ("ln_1.weight", "layer_norm1.weight"), ("ln_1.bias", "layer_norm1.bias"),
               ("ln_2.weight", "layer_norm2.weight"), ("ln_2.bias", "layer_norm2.bias"))


@torch.no_grad()
def load_openclip_state_dict(vit: VitModel, sd, dtype: torch.dtype = torch.float32) -> List[str]:
    """The reference's best-effort mapping (deepencoder_infer.py:219-276): class_embedding, positional_embedding (the whole table when
    the lengths agree, else the first n positions) and, per block i, transformer.resblocks.i.{attn.in_proj_*, attn.out_proj.*, mlp.c_fc.*,
    mlp.c_proj.*, ln_1.*, ln_2.*}.  A key the state dict lacks is skipped; CLIP's patch conv is not copied.  Returns the keys it read."""
    used = []
    emb = vit.embeddings
    if "class_embedding" in sd:
        emb.class_embedding.copy_(sd["class_embedding"].to(dtype))
        used.append("class_embedding")
    if "positional_embedding" in sd:
        pe = sd["positional_embedding"].to(dtype)
        pe = pe.squeeze(0) if pe.dim() == 3 else pe
        if emb.num_positions == pe.shape[0]:
            emb.position_embedding.weight.copy_(pe)
        else:
            n = min(emb.num_positions, pe.shape[0])
            emb.position_embedding.weight[:n].copy_(pe[:n])
        used.append("positional_embedding")
    named = dict(vit.named_parameters())
    for i in range(len(vit.transformer.layers)):
        for src, dst in _BLOCK_KEYS:
            v = sd.get(f"transformer.resblocks.{i}.{src}", None)
            if v is not None:
                named[f"transformer.layers.{i}.{dst}"].copy_(v.to(dtype))
                used.append(f"transformer.resblocks.{i}.{src}")
    return used


# ------------------------------------------------------------------------------------------------------------------------------------
# runtime
# ------------------------------------------------------------------------------------------------------------------------------------
_warned_network = False


def _to_dtype(s) -> torch.dtype:
    if not isinstance(s, str):
        return s
    if s.lower() in ("bf16", "bfloat16"):
        return torch.bfloat16
    if s.lower() in ("fp32", "float32"):
        return torch.float32
    raise ValueError(f"Unsupported dtype string: {s}")


class DeepEncoderRuntime:
    """SAM ViT-B -> CLIP-L conditioned on SAM's features -> projector, on the HIP kernels.  `dtype` is recorded for callers that read
    it; the kernels' number formats are set by `precision` (None -> "bf16x3", or "bf16") and every result is fp32."""

    def __init__(self, *, sam_ckpt: Optional[str] = None, auto_download_sam: bool = True, device="cuda", dtype=torch.bfloat16,
                 openclip_pretrained: str = "openai", lora_config=None, freeze_clip_backbone_when_lora_enabled: bool = True):
        global _warned_network
        if not _warned_network:
            _warned_network = True
            warnings.warn("DeepEncoderRuntime: auto_download_sam and openclip_pretrained are accepted and ignored -- this package never "
                          "reaches the network; pass sam_ckpt= a local file and load CLIP weights with load_openclip_state_dict()", stacklevel=2)
        if lora_config is not None and getattr(lora_config, "enabled", False):
            raise F.LvqError("DeepEncoderRuntime: LoRA / training of the towers is outside this package (inference-only kernels)")
        self.lora_config = lora_config
        self.freeze_clip_backbone_when_lora_enabled = freeze_clip_backbone_when_lora_enabled
        self._set(build_sam_vit_b(checkpoint=sam_ckpt), build_clip_l(), MlpProjectorLinear(2048, 2048), device, dtype)

    def _set(self, sam, clip_vit, projector, device, dtype):
        self.image_size = FIXED_IMAGE_SIZE
        self.grid = (FIXED_GRID_SIDE, FIXED_GRID_SIDE)
        self.device = device
        self.dtype = _to_dtype(dtype)
        self.precision: Optional[str] = None
        self.sam = sam.to(device)
        self.clip_vit = clip_vit.to(device)
        self.projector = projector.to(device)
        for m in (self.sam, self.clip_vit, self.projector):
            for p in m.parameters():
                p.requires_grad = False
        return self.eval()

    @classmethod
    def from_modules(cls, sam, clip_vit, projector, *, device="cuda", dtype=torch.float32) -> "DeepEncoderRuntime":
        """A runtime over towers the caller built (other geometries, weights already loaded); nothing is constructed or read here."""
        self = object.__new__(cls)
        self.lora_config, self.freeze_clip_backbone_when_lora_enabled = None, True
        return self._set(sam, clip_vit, projector, device, dtype)

    def train(self):
        raise F.LvqError("DeepEncoderRuntime: inference-only kernels; training of the towers is outside this package")

    def trainable_parameters(self):
        raise F.LvqError("DeepEncoderRuntime: inference-only kernels; there are no trainable parameters")

    def eval(self):
        self.sam.eval()
        self.clip_vit.eval()
        self.projector.eval()
        return self

    @torch.no_grad()
    def encode_pixels(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, 3, S, S] fp32 in [-1, 1] on the device -> vision tokens [B, HW, n_embed] fp32."""
        for m in (self.sam, self.clip_vit, self.projector):
            m.precision = self.precision
        sam_feats = self.sam(x)                                               # [B, C_sam, g, g] fp32, channel-major
        split = self.clip_vit._enter(x, sam_feats)
        clip_rows, sam_tok, hw = self.clip_vit._run(x, sam_feats, split, want_tok=True)
        b, d_clip, d_sam = x.shape[0], clip_rows.shape[1], sam_feats.shape[1]
        lin = self.projector.layers
        if lin.in_features != d_clip + d_sam or d_clip % 8:
            raise F.LvqError(f"DeepEncoderRuntime: the projector reads {lin.in_features} columns, the towers give {d_clip} + {d_sam}")
        w = self.projector._w(lin.weight)
        if (w[1] is not None) != split:
            raise F.LvqError("DeepEncoderRuntime: the projector and the towers must run in one precision mode")
        bias = lin.bias.detach().float().contiguous() if lin.bias is not None else None
        y, _ = O.linear(O.cast(clip_rows, split), w, bias, w_cols=(0, d_clip), a_rows=(b, 1 + hw, 1, hw), out_f32=True, tag="clip_gemm")
        y, _ = O.linear(sam_tok, w, None, w_cols=(d_clip, d_clip + d_sam), residual=y, out_f32=True, tag="clip_gemm")
        return y.view(b, hw, -1)

    def _load(self, path) -> torch.Tensor:
        from PIL import Image
        return _pil_to_tensor_og_norm(resize_and_pad_to_square(Image.open(path), self.image_size))

    def encode_image(self, image_path) -> dict:
        tok = self.encode_pixels(self._load(str(image_path)).to(self.device))
        return {"tokens": tok[0], "grid": self.grid, "image_size": self.image_size}

    def encode_views(self, image_paths: Sequence[Optional[Path]], *, strict: bool = True, view_order: Sequence[str] = DEFAULT_VIEW_ORDER) -> dict:
        """Tokens [HW, n_embed] per view; the views that are present run as one batch.  A missing view gives zeros, or with
        strict=True raises FileNotFoundError."""
        present = [p is not None and Path(p).exists() for p in image_paths]
        for p, ok in zip(image_paths, present):
            if strict and not ok:
                raise FileNotFoundError(f"Missing view file: {p}")
        if not any(present):
            raise RuntimeError("No available camera views to infer token shape.")
        x = torch.cat([self._load(str(p)) for p, ok in zip(image_paths, present) if ok]).to(self.device)
        tok = self.encode_pixels(x)
        it = iter(tok.unbind(0))
        tokens = [next(it) if ok else torch.zeros(tok.shape[1:], device=tok.device, dtype=tok.dtype) for ok in present]
        return {"tokens": tokens, "present_mask": present, "view_names": list(view_order), "grid": self.grid, "image_size": self.image_size}


def multiview_tokens_from_sample_token(sample_token: str, nusc, *, runtime: Optional[DeepEncoderRuntime] = None,
                                       view_order: Sequence[str] = DEFAULT_VIEW_ORDER, strict: bool = False, sam_ckpt: Optional[str] = None,
                                       auto_download_sam: bool = True, device="cuda", dtype=torch.bfloat16,
                                       openclip_pretrained: str = "openai") -> dict:
    """encode_views on the sample's camera files, plus the runtime (built here when none is given)."""
    if runtime is None:
        runtime = DeepEncoderRuntime(sam_ckpt=sam_ckpt, auto_download_sam=auto_download_sam, device=device, dtype=dtype,
                                     openclip_pretrained=openclip_pretrained)
    out = runtime.encode_views(resolve_cam_image_paths(nusc, sample_token, view_order=view_order), strict=strict, view_order=view_order)
    out["runtime"] = runtime
    return out
