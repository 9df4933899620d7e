"""The CLIP-L tower of the vision path (deepencoder/clip_sdpa.py) on the HIP kernels of liblvq_hip.so.

  VitModel(cfg)                       forward(x [B, 3, H, W], patch_embeds [B, C, Hs, Ws] | None) -> [B, 1 + Hs Ws, C] fp32
                                      (also forward(pixel_values=, patch_embeds=), the reference's keyword form)
  CLIPVisionEmbeddings / NoTPFeedForward / NoTPAttention / NoTPTransformerBlock / NoTPTransformer / LayerNormfp32
                                      the reference's sub-modules (same constructors, registration order and state_dict keys)
  get_abs_pos / quick_gelu / clip_l_lora_default_targets / vit_model_cfg / build_clip_l()

The modules hold nn.Linear / nn.LayerNorm / nn.Embedding / nn.Conv2d in the reference's registration order (`pre_layrnorm`, the
reference's spelling, after `transformer`; `position_ids` a non-persistent buffer), so checkpoints load strictly and default
initialisation consumes the RNG in the reference's order.  forward never calls these containers.  The chain, every arithmetic step
a launch of the library:

  embedding   the position table through get_abs_pos (input-independent: once per weights version and grid, by torch) ->
              lvq_clip_embed: class row + transposed patch features + positions + pre_layrnorm in one launch; on request it also
              hands back the patch features as the token-major bf16 operand the DeepEncoder's projector reads
  block       lvq_layernorm -> qkv_proj lvq_gemm_bf16 (packed bf16 [B S, 3 d]) -> lvq_attention_bf16 through strides ->
              out_proj + residual -> lvq_layernorm -> fc1 + QuickGELU (LVQ_GEMM_QUICK_GELU) -> fc2 + residual

With patch_embeds=None the module's own bias-free stride-14 conv runs as one GEMM over the patches gathered by a permute (K = 588
zero-padded to 592 for the 16-byte operand loads); its token-major result is turned channel-major by a copy.

Inference only: train() mode, or a call with gradients in reach, raises LvqError, and so do CPU tensors (no fallback).  Head dims
other than 64 have no attention kernel here and raise LvqError.  Precision: `precision` of the module, None -> "bf16x3" (hi + lo
operands) or "bf16"; operand copies of the weights and the position tables are cached per parameter version and mode.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as TF

from . import _ffi as F
from . import ops as O
from .vision_tower import _cached, _f32, _guard, _operand

__all__ = ["VitModel", "build_clip_l", "clip_l_lora_default_targets", "vit_model_cfg"]


def clip_l_lora_default_targets():
    """The Linear sub-module names the reference lists as LoRA targets (LoRA itself is outside this package)."""
    return ("qkv_proj", "out_proj", "mlp.fc1", "mlp.fc2")


class _Cfg(dict):
    """A plain attribute dict: cfg.hidden_size and cfg.get("fp32norm", False) both work, as with the reference's config object."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name, value):
        self[name] = value


def quick_gelu(x: torch.Tensor) -> torch.Tensor:
    """x sigmoid(1.702 x): the definition (host / fp64 checks); the towers apply it in the fc1 GEMM's epilogue."""
    return x * torch.sigmoid(1.702 * x)


def get_abs_pos(abs_pos: torch.Tensor, tgt_tokens: int) -> torch.Tensor:
    """[1, Npos, C] position table -> [1, tgt_tokens, C], as the reference computes it (clip_sdpa.py:77-117): unchanged when the length
    fits; bicubic antialiased resample of the grid part in fp32 when both grids are square; otherwise truncated, or padded with zeros."""
    if abs_pos.dim() != 3 or abs_pos.size(0) != 1:
        return abs_pos
    cls, grid = abs_pos[:, :1, :], abs_pos[:, 1:, :]
    src_hw = grid.size(1)
    if src_hw == tgt_tokens - 1:
        return abs_pos
    src_side = int(math.sqrt(src_hw))
    tgt_side = int(math.sqrt(max(tgt_tokens - 1, 1)))
    if src_side * src_side != src_hw or tgt_side * tgt_side != (tgt_tokens - 1):
        if tgt_tokens <= abs_pos.size(1):
            return abs_pos[:, :tgt_tokens, :]
        pad = torch.zeros(1, tgt_tokens - abs_pos.size(1), abs_pos.size(2), dtype=abs_pos.dtype, device=abs_pos.device)
        return torch.cat([abs_pos, pad], dim=1)
    g = grid.transpose(1, 2).reshape(1, grid.size(2), src_side, src_side).to(torch.float32)
    g = TF.interpolate(g, size=(tgt_side, tgt_side), mode="bicubic", align_corners=False, antialias=True).to(abs_pos.dtype)
    return torch.cat([cls, g.reshape(1, grid.size(2), tgt_side * tgt_side).transpose(1, 2)], dim=1)


def _ln_params(ln: nn.Module, who: str):
    if not isinstance(ln, nn.LayerNorm) or len(ln.normalized_shape) != 1 or ln.weight is None:
        raise F.LvqError(f"{who}: {type(ln).__name__} has no kernel here (nn.LayerNorm over the last dim, affine)")
    return _f32(ln.weight), _f32(ln.bias), ln.eps


class CLIPVisionEmbeddings(nn.Module):
    def __init__(self, hidden_size=1024, image_size=224, patch_size=14, num_channels=3):
        super().__init__()
        self.embed_dim = hidden_size
        self.image_size = image_size
        self.patch_size = patch_size
        self.class_embedding = nn.Parameter(torch.randn(self.embed_dim))
        self.patch_embedding = nn.Conv2d(in_channels=num_channels, out_channels=self.embed_dim, kernel_size=self.patch_size,
                                         stride=self.patch_size, bias=False)
        self.num_patches = (self.image_size // self.patch_size) ** 2
        self.num_positions = self.num_patches + 1
        self.position_embedding = nn.Embedding(self.num_positions, self.embed_dim)
        self.register_buffer("position_ids", torch.arange(self.num_positions).expand((1, -1)), persistent=False)

    def _pos_table(self, tokens: int) -> torch.Tensor:
        """position_embedding at `tokens` rows, fp32 [tokens, C]: get_abs_pos once per weights version and length."""
        p = self.position_embedding.weight
        return _cached(self, ("pos", tokens), (p,), lambda: get_abs_pos(p.detach().float().unsqueeze(0), tokens)[0].contiguous())

    def _own_patches(self, x: torch.Tensor, split: bool) -> torch.Tensor:
        """The module's own patch conv as a GEMM over gathered patches -> channel-major features [B, C, gh gw] fp32."""
        conv = self.patch_embedding
        k = conv.kernel_size
        if tuple(conv.stride) != tuple(k) or tuple(conv.padding) != (0, 0) or tuple(conv.dilation) != (1, 1) or conv.groups != 1 \
                or conv.bias is not None:
            raise F.LvqError("CLIPVisionEmbeddings: the patch GEMM needs kernel = stride, padding 0, dilation 1, groups 1, no bias")
        b, c, h, w = x.shape
        gh, gw = h // k[0], w // k[1]
        if gh < 1 or gw < 1 or c != conv.in_channels:
            raise F.LvqError(f"CLIPVisionEmbeddings: a [{c}, {h}, {w}] image leaves no {k[0]} x {k[1]} patch")
        kk = c * k[0] * k[1]
        pad = -kk % 8                                        # 16-byte operand loads: K in multiples of 8
        rows = x[:, :, :gh * k[0], :gw * k[1]].reshape(b, c, gh, k[0], gw, k[1]).permute(0, 2, 4, 1, 3, 5).reshape(b * gh * gw, kk)
        wt = _cached(conv, ("w", "patch", split, pad), (conv.weight,),
                     lambda: O.cast(TF.pad(conv.weight.detach().float().reshape(conv.out_channels, kk), (0, pad)).contiguous(), split))
        tok, _ = O.linear(O.cast(TF.pad(rows, (0, pad)).contiguous(), split), wt, None, out_f32=True)
        return tok.view(b, gh * gw, -1).transpose(1, 2).contiguous()

    def _run(self, x: torch.Tensor, patch_embeds: Optional[torch.Tensor], ln: nn.Module, split: bool, want_tok: bool = False):
        """-> (hidden [B (1 + hw), C] fp32 = ln(embeddings), tok BF [B hw, C] | None, hw): one lvq_clip_embed launch."""
        if patch_embeds is None:
            feat = self._own_patches(x.float(), split)
        else:
            if patch_embeds.dim() != 4 or patch_embeds.shape[1] != self.embed_dim:
                raise F.LvqError(f"CLIPVisionEmbeddings: patch_embeds must be [B, {self.embed_dim}, Hs, Ws], got {tuple(patch_embeds.shape)}")
            feat = patch_embeds.float().flatten(2).contiguous()
        b, c, hw = feat.shape
        if not O.clip_embed_ok(b, c, hw):
            raise F.LvqError(f"CLIPVisionEmbeddings: width {c} on {hw} patches is outside lvq_clip_embed's family (c % 64 == 0, c <= 2048)")
        gamma, beta, eps = _ln_params(ln, "VitModel.pre_layrnorm")
        hidden, tok = O.clip_embed(feat, _f32(self.class_embedding), self._pos_table(1 + hw), gamma, beta, eps, want_tok=want_tok,
                                   split=split, tag="clip_embed")
        return hidden, tok, hw

    def forward(self, pixel_values: torch.Tensor, patch_embeds: Optional[torch.Tensor] = None, **kwargs):
        raise F.LvqError("CLIPVisionEmbeddings: the embedding step runs fused with pre_layrnorm (lvq_clip_embed); call VitModel, or "
                         "VitModel.embed(x, patch_embeds) for the normalised embeddings")


class NoTPFeedForward(nn.Module):
    def __init__(self, cfg, dim: int, hidden_dim: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden_dim, bias=True)
        self.fc2 = nn.Linear(hidden_dim, dim, bias=True)

    def _run(self, h: O.BF, residual: Optional[torch.Tensor], split: bool) -> torch.Tensor:
        """fc2(quick_gelu(fc1(h))) (+ residual) on rows: two GEMMs, the activation and the residual in their epilogues."""
        _, m = O.linear(h, _operand(self.fc1, "weight", split), _f32(self.fc1.bias), quick_gelu=True, out_bf=True, tag="clip_gemm")
        return O.linear(m, _operand(self.fc2, "weight", split), _f32(self.fc2.bias), residual=residual, out_f32=True, tag="clip_gemm")[0]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        split = _guard(self, x, x.dim())
        rows = x.float().reshape(-1, x.shape[-1]).contiguous()
        return self._run(O.cast(rows, split), None, split).view(*x.shape[:-1], -1)


class NoTPAttention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.num_heads = cfg.num_attention_heads
        self.head_dim = cfg.hidden_size // cfg.num_attention_heads
        self.max_seq_len = cfg.seq_length
        self.use_flash_attention = False                  # one attention kernel here, whatever cfg.use_flash_attn says
        self.qkv_proj = nn.Linear(cfg.hidden_size, cfg.hidden_size * 3, bias=True)
        self.out_proj = nn.Linear(cfg.hidden_size, cfg.hidden_size, bias=True)
        self.attn_drop = cfg.attention_dropout

    def _run(self, h: O.BF, batch: int, s: int, residual: Optional[torch.Tensor], split: bool) -> torch.Tensor:
        """h BF [batch s, d] -> out_proj(attention(qkv_proj(h))) (+ residual) fp32 [batch s, d]."""
        d, dh, nh = self.qkv_proj.in_features, self.head_dim, self.num_heads
        if dh != 64 or dh * nh != d:
            raise F.LvqError(f"NoTPAttention: head dim {dh} ({nh} heads of width {d}) is outside the kernel family (head dim 64)")
        _, qkv = O.linear(h, _operand(self.qkv_proj, "weight", split), _f32(self.qkv_proj.bias), out_bf=True, tag="clip_gemm")
        sl = lambda c: (qkv[0][:, c * d:], None if qkv[1] is None else qkv[1][:, c * d:])      # row = [3, heads, dh]
        st = (s * 3 * d, 3 * d, dh)
        o = O.attention(sl(0), sl(1), sl(2), batch=batch, n_heads=nh, n_kv_heads=nh, nq=s, nkv=s, dh=dh, q_strides=st, k_strides=st,
                        v_strides=st, scale=1.0 / math.sqrt(dh), tag="clip_attn")
        return O.linear(o, _operand(self.out_proj, "weight", split), _f32(self.out_proj.bias), residual=residual, out_f32=True,
                        tag="clip_gemm")[0]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        split = _guard(self, x, 3)
        b, s, c = x.shape
        return self._run(O.cast(x.float().reshape(-1, c).contiguous(), split), b, s, None, split).view(b, s, c)


class NoTPTransformerBlock(nn.Module):
    def __init__(self, cfg, layer_id: int, multiple_of=256):
        super().__init__()
        self.n_heads = cfg.num_attention_heads
        self.dim = cfg.hidden_size
        self.head_dim = cfg.hidden_size // cfg.num_attention_heads
        self.self_attn = NoTPAttention(cfg)
        self.mlp = NoTPFeedForward(cfg, dim=cfg.hidden_size, hidden_dim=cfg.ffn_hidden_size)
        self.layer_id = layer_id
        self.layer_norm1 = nn.LayerNorm(cfg.hidden_size, eps=cfg.layernorm_epsilon)
        self.layer_norm2 = nn.LayerNorm(cfg.hidden_size, eps=cfg.layernorm_epsilon)

    @staticmethod
    def _norm(ln: nn.Module, rows: torch.Tensor, split: bool) -> O.BF:
        gamma, beta, eps = _ln_params(ln, "NoTPTransformerBlock")
        with O.region("clip_ln", rows.device):
            return O.layernorm(rows, gamma, beta, eps, split)[1]

    def _run(self, x: torch.Tensor, batch: int, s: int, split: bool) -> torch.Tensor:
        """x [batch s, d] fp32 rows -> the same."""
        x = self.self_attn._run(self._norm(self.layer_norm1, x, split), batch, s, x, split)
        return self.mlp._run(self._norm(self.layer_norm2, x, split), x, split)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        split = _guard(self, x, 3)
        b, s, c = x.shape
        return self._run(x.float().reshape(-1, c).contiguous(), b, s, split).view(b, s, c)


class NoTPTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.num_layers = cfg.num_layers
        self.layers = nn.ModuleList([NoTPTransformerBlock(cfg, layer_id=i + 1) for i in range(self.num_layers)])

    def _run(self, x: torch.Tensor, batch: int, s: int, split: bool) -> torch.Tensor:
        for layer in self.layers:
            x = layer._run(x, batch, s, split)
        return x

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        split = _guard(self, hidden_states, 3)
        b, s, c = hidden_states.shape
        return self._run(hidden_states.float().reshape(-1, c).contiguous(), b, s, split).view(b, s, c)


class LayerNormfp32(nn.LayerNorm):
    """nn.LayerNorm whose statistics are fp32 whatever the input type: every LayerNorm launch here already is."""


class VitModel(nn.Module):
    def __init__(self, cfg, freeze_embed=False, freeze_pre_norm=False) -> None:
        super().__init__()
        self.embeddings = CLIPVisionEmbeddings(hidden_size=cfg.hidden_size, image_size=cfg.image_size, patch_size=cfg.patch_size)
        if freeze_embed:
            for _, p in self.embeddings.named_parameters():
                p.requires_grad = False
        self.transformer = NoTPTransformer(cfg=cfg)
        norm = LayerNormfp32 if cfg.get("fp32norm", False) else nn.LayerNorm
        self.pre_layrnorm = norm(cfg.hidden_size, eps=cfg.get("pre_layernorm_epsilon", 1e-5))
        if freeze_pre_norm:
            for _, p in self.pre_layrnorm.named_parameters():
                p.requires_grad = False
        self.precision: Optional[str] = None          # None -> "bf16x3"

    def __str__(self) -> str:
        return "open_clip"

    @staticmethod
    def _args(args, x, patch_embeds, pixel_values, kwargs):
        if len(args) >= 1 and x is None and pixel_values is None:
            x = args[0]
        if len(args) >= 2 and patch_embeds is None:
            patch_embeds = args[1]
        if x is None and pixel_values is not None:
            x = pixel_values
        if x is None and "inputs_embeds" in kwargs and kwargs.get("pixel_values") is not None:
            x = kwargs["pixel_values"]
        if x is None:
            raise ValueError(f"Either 'x' or 'pixel_values' must be provided. Received: args_len={len(args)}, "
                             f"patch_embeds={patch_embeds is not None}, kwargs_keys={list(kwargs.keys())}")
        return x, patch_embeds

    def _run(self, x: torch.Tensor, patch_embeds: Optional[torch.Tensor], split: bool, want_tok: bool = False):
        """-> (output rows [B (1 + hw), C] fp32, tok BF | None, hw)."""
        hidden, tok, hw = self.embeddings._run(x, patch_embeds, self.pre_layrnorm, split, want_tok)
        return self.transformer._run(hidden, x.shape[0], 1 + hw, split), tok, hw

    def _enter(self, x: torch.Tensor, patch_embeds: Optional[torch.Tensor]) -> bool:
        split = _guard(self, x, 4)
        if patch_embeds is not None:
            F.require_cuda(patch_embeds.contiguous())
            if patch_embeds.requires_grad and torch.is_grad_enabled():
                raise F.LvqError("VitModel: inference-only kernels; call it in eval() mode under torch.no_grad()")
        return split

    def embed(self, x: torch.Tensor, patch_embeds: Optional[torch.Tensor] = None) -> torch.Tensor:
        """pre_layrnorm(embeddings(x, patch_embeds)) [B, 1 + hw, C]: the residual stream of block 0."""
        split = self._enter(x, patch_embeds)
        hidden, _, hw = self.embeddings._run(x, patch_embeds, self.pre_layrnorm, split)
        return hidden.view(x.shape[0], 1 + hw, -1)

    def forward(self, *args, x: Optional[torch.Tensor] = None, patch_embeds: Optional[torch.Tensor] = None,
                pixel_values: Optional[torch.Tensor] = None, **kwargs):
        x, patch_embeds = self._args(args, x, patch_embeds, pixel_values, kwargs)
        split = self._enter(x, patch_embeds)
        out, _, hw = self._run(x, patch_embeds, split)
        return out.view(x.shape[0], 1 + hw, -1)


vit_model_cfg = _Cfg(
    num_layers=24,
    hidden_size=1024,
    num_heads=16,
    num_attention_heads=16,
    ffn_hidden_size=4096,
    seq_length=256,
    max_position_embeddings=256,
    use_flash_attn=False,
    understand_projector_stride=2,
    hidden_dropout=0.0,
    attention_dropout=0.0,
    no_persist_layer_norm=False,
    layernorm_epsilon=1e-5,
    pre_layernorm_epsilon=1e-5,
    image_size=224,
    patch_size=14,
    recompute_list=[],
)


def build_clip_l():
    return VitModel(cfg=vit_model_cfg, freeze_embed=False, freeze_pre_norm=False)
