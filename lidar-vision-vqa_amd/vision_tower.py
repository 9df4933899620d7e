"""The SAM ViT image encoder of the vision path (deepencoder/sam_vary_sdpa.py:100-511) on the HIP kernels of liblvq_hip.so.

  ImageEncoderViT(img_size, patch_size, ..., window_size, global_attn_indexes)     forward(x [B, 3, S, S] fp32) -> [B, 1024, S/64, S/64] fp32
  Block / Attention / MLPBlock / LayerNorm2d / PatchEmbed                          the reference's sub-modules (same constructors)
  window_partition / window_unpartition                                            the padded window split and its inverse (copies)
  build_sam_vit_b(checkpoint=None)                                                 the ViT-B geometry + the three checkpoint prefix cases

The modules hold nn.Conv2d / nn.Linear / nn.LayerNorm / nn.Parameter in the reference's registration order, so state_dict() keys, order
and shapes are the reference's (checkpoints load with strict=True) and default initialisation consumes the RNG in the reference's
order.  forward never calls these containers.  The chain, every arithmetic step a launch of the library:

  patch embed    the 16 x 16 x 3 patches gathered by a permute, ONE lvq_gemm_bf16 with the conv bias and `pos_embed` (rowtab) in its epilogue
  block          lvq_layernorm (eps from the module) -> qkv lvq_gemm_bf16 -> lvq_attention_relpos_bf16 (the decomposed relative-position
                 bias is formed inside the kernel) -> proj lvq_gemm_bf16 + residual -> lvq_layernorm -> lin1 + GELU -> lin2 + residual
  neck           1 x 1 conv as a GEMM -> LayerNorm2d as a row LayerNorm over channels-last rows (its bf16 outputs ARE the conv planes)
                 -> 3 x 3 lvq_conv2d -> LayerNorm2d
  net_2, net_3   lvq_conv2d (stride 2); net_3 as c_out = 512 halves written at channel offsets 0 and 512 of the result

Windowed blocks: the LayerNorm output is zero-padded to a multiple of the window AFTER the norm and split into windows by a copy
(window_partition on the 16-bit operand planes); the pad rows go through the qkv projection like every other row (k = b_k, v = b_v) and
are live keys of their window's softmax, exactly as in the reference.  The attention output is un-partitioned and cropped by a second
copy BEFORE the output projection, which therefore runs on the image's own rows with the residual in its epilogue.

torch moves data (permute, pad, view, contiguous) and prepares input-independent tables once per weights version (the bicubic resize
of `pos_embed`, the linear resize of a relative-position table whose length is not 2 size - 1, both as the reference computes them);
it does no per-input arithmetic.

Inference only: train() mode, or a call with gradients in reach, raises LvqError, and so do CPU tensors (no fallback).
`use_rel_pos=False` and head dims other than 64 have no kernel here and raise LvqError.
Precision: `precision` of the encoder, "bf16x3" (hi + lo operands: the default) or "bf16".  Operand copies of the weights and the resized
tables are cached per parameter version and mode.
"""
from __future__ import annotations

import os
from functools import partial
from typing import Optional, Tuple, Type

import torch
import torch.nn as nn
import torch.nn.functional as TF

from . import _ffi as F
from . import autograd_route as AG
from . import ops as O

MODES = ("bf16x3", "bf16")
DEFAULT_MODE = "bf16x3"
FAMILY = "use_rel_pos=True, head dim 64, attention grids (window, or image / patch) of 1 .. 64 per side"


# ------------------------------------------------------------------------------------------------------------------------------------
# caches and guards
# ------------------------------------------------------------------------------------------------------------------------------------
def _cached(mod: nn.Module, key, params, build):
    """build() once per (key, version of params): packed weights and resized tables."""
    return F.derived(mod.__dict__.setdefault("_lvq_cache", {}), key, params, build)


def _operand(mod: nn.Module, name: str, split: bool, shape=None) -> O.BF:
    """A parameter as a bf16 (hi, lo) operand, viewed as `shape`."""
    p = getattr(mod, name)
    return _cached(mod, ("w", name, split, shape), (p,), lambda: O.cast(p.detach().float().reshape(shape or p.shape).contiguous(), split))


def _f32(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if p is None else p.detach().float().contiguous()


def _mode(mod: nn.Module) -> bool:
    mode = getattr(mod, "precision", None) or DEFAULT_MODE
    if mode not in MODES:
        raise F.LvqError(f"{type(mod).__name__} runs in {MODES}, not {mode!r}")
    return mode == "bf16x3"


def _guard(mod: nn.Module, x: torch.Tensor, dims: int) -> bool:
    name = type(mod).__name__
    if AG.wanted(mod, x):
        raise F.LvqError(f"{name}: inference-only kernels; call it in eval() mode under torch.no_grad()")
    if x.dim() != dims:
        raise F.LvqError(f"{name}: expected a {dims}-d input, got {tuple(x.shape)}")
    F.require_cuda(x.contiguous(), *mod.parameters())
    return _mode(mod)


# ------------------------------------------------------------------------------------------------------------------------------------
# data movement
# ------------------------------------------------------------------------------------------------------------------------------------
def window_partition(x: torch.Tensor, window_size: int) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """[B, H, W, C] -> ([B * windows, window, window, C], (Hp, Wp)): zero padding at the bottom / right up to a multiple of the window."""
    b, h, w, c = x.shape
    hp, wp = -(-h // window_size) * window_size, -(-w // window_size) * window_size
    if (hp, wp) != (h, w):
        x = TF.pad(x, (0, 0, 0, wp - w, 0, hp - h))
    x = x.view(b, hp // window_size, window_size, wp // window_size, window_size, c).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(-1, window_size, window_size, c), (hp, wp)


def window_unpartition(windows: torch.Tensor, window_size: int, pad_hw: Tuple[int, int], hw: Tuple[int, int]) -> torch.Tensor:
    """The inverse: [B * windows, window, window, C] -> [B, H, W, C] with the padding cropped."""
    hp, wp = pad_hw
    h, w = hw
    nh, nw = hp // window_size, wp // window_size
    b = windows.shape[0] // (nh * nw)
    x = windows.view(b, nh, nw, window_size, window_size, -1).permute(0, 1, 3, 2, 4, 5).reshape(b, hp, wp, -1)
    return x[:, :h, :w, :].contiguous()


def _bf_map(x: O.BF, fn) -> O.BF:
    return fn(x[0]), (None if x[1] is None else fn(x[1]))


# ------------------------------------------------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------------------------------------------------
class MLPBlock(nn.Module):
    def __init__(self, embedding_dim: int, mlp_dim: int, act: Type[nn.Module] = nn.GELU) -> None:
        super().__init__()
        self.lin1 = nn.Linear(embedding_dim, mlp_dim)
        self.lin2 = nn.Linear(mlp_dim, embedding_dim)
        self.act = act()

    def _run(self, h: O.BF, residual: Optional[torch.Tensor], split: bool) -> torch.Tensor:
        """lin2(GELU(lin1(h))) (+ residual) on rows: two GEMMs, the activation and the residual in their epilogues."""
        if not isinstance(self.act, nn.GELU) or getattr(self.act, "approximate", "none") != "none":
            raise F.LvqError(f"MLPBlock: {type(self.act).__name__} has no kernel here (exact GELU only)")
        _, m = O.linear(h, _operand(self.lin1, "weight", split), _f32(self.lin1.bias), gelu=True, out_bf=True)
        return O.linear(m, _operand(self.lin2, "weight", split), _f32(self.lin2.bias), residual=residual, out_f32=True)[0]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        split = _guard(self, x, x.dim())
        rows = x.float().reshape(-1, x.shape[-1]).contiguous()
        return self._run(O.cast(rows, split), None, split).view(*x.shape[:-1], -1)


class LayerNorm2d(nn.Module):
    def __init__(self, num_channels: int, eps: float = 1e-6) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))
        self.eps = eps

    def _rows(self, rows: torch.Tensor, split: bool, want_f32: bool = False):
        """Row LayerNorm over channels-last rows [pixels, C] (biased variance, eps inside the root: LayerNorm2d's arithmetic)."""
        return O.layernorm(rows, _f32(self.weight), _f32(self.bias), self.eps, split, want_f32=want_f32, want_bf=not want_f32)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        split = _guard(self, x, 4)
        b, c, h, w = x.shape
        y, _ = self._rows(x.float().permute(0, 2, 3, 1).reshape(-1, c).contiguous(), split, want_f32=True)
        return y.view(b, h, w, c).permute(0, 3, 1, 2).contiguous()


class PatchEmbed(nn.Module):
    def __init__(self, kernel_size: Tuple[int, int] = (16, 16), stride: Tuple[int, int] = (16, 16), padding: Tuple[int, int] = (0, 0),
                 in_chans: int = 3, embed_dim: int = 768) -> None:
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=kernel_size, stride=stride, padding=padding)

    def _run(self, x: torch.Tensor, split: bool, rowtab: Optional[torch.Tensor] = None):
        """[B, C, H, W] fp32 -> (tokens [B * gh * gw, d] fp32, gh, gw): the patches gathered by a permute, one GEMM, bias (+ rowtab)."""
        conv = self.proj
        k = conv.kernel_size
        if tuple(conv.stride) != tuple(k) or tuple(conv.padding) != (0, 0) or tuple(conv.dilation) != (1, 1) or conv.groups != 1:
            raise F.LvqError("PatchEmbed: the patch GEMM needs kernel = stride, padding 0, dilation 1, groups 1")
        b, c, h, w = x.shape
        gh, gw = h // k[0], w // k[1]
        if gh < 1 or gw < 1 or (c * k[0] * k[1]) % 8:
            raise F.LvqError(f"PatchEmbed: a [{c}, {h}, {w}] image leaves no {k[0]} x {k[1]} patch row the GEMM takes")
        rows = x[:, :, :gh * k[0], :gw * k[1]].reshape(b, c, gh, k[0], gw, k[1]).permute(0, 2, 4, 1, 3, 5).reshape(b * gh * gw, c * k[0] * k[1])
        wt = _operand(conv, "weight", split, (conv.out_channels, c * k[0] * k[1]))
        tok, _ = O.linear(O.cast(rows.contiguous(), split), wt, _f32(conv.bias), rowtab=rowtab, out_f32=True)
        return tok, gh, gw

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        split = _guard(self, x, 4)
        tok, gh, gw = self._run(x.float().contiguous(), split)
        return tok.view(x.shape[0], gh, gw, -1)


class Attention(nn.Module):
    """Multi-head self-attention over a token grid with decomposed relative-position embeddings."""

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = True, use_rel_pos: bool = False, rel_pos_zero_init: bool = True,
                 input_size: Optional[Tuple[int, int]] = None) -> None:
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.use_rel_pos = use_rel_pos
        if use_rel_pos:
            assert input_size is not None, "Input size must be provided if using relative positional encoding."
            self.rel_pos_h = nn.Parameter(torch.zeros(2 * input_size[0] - 1, head_dim))
            self.rel_pos_w = nn.Parameter(torch.zeros(2 * input_size[1] - 1, head_dim))

    def _table(self, name: str, size: int, split: bool) -> O.BF:
        """rel_pos_h / rel_pos_w as a [2 size - 1, dh] operand; another length is resized linearly, once per weights version."""
        p = getattr(self, name)

        def build():
            t = p.detach().float()
            n = 2 * size - 1
            if t.shape[0] != n:
                t = TF.interpolate(t.t().unsqueeze(0), size=n, mode="linear")[0].t()
            return O.cast(t.contiguous(), split)
        return _cached(self, ("rel", name, size, split), (p,), build)

    def _core(self, h: O.BF, batch: int, gh: int, gw: int, split: bool) -> O.BF:
        """qkv projection + fused attention on `batch` grids of gh x gw rows -> the un-projected heads [batch * gh * gw, d]."""
        d = self.qkv.in_features
        dh = d // self.num_heads
        if not self.use_rel_pos or dh * self.num_heads != d or not O.attention_relpos_ok(gh, gw, dh):
            raise F.LvqError(f"Attention(use_rel_pos={self.use_rel_pos}, head dim {dh}) on a {gh} x {gw} grid is outside the kernel family ({FAMILY})")
        _, qkv = O.linear(h, _operand(self.qkv, "weight", split), _f32(self.qkv.bias), out_bf=True)
        return O.attention_relpos(qkv, self._table("rel_pos_h", gh, split), self._table("rel_pos_w", gw, split), batch=batch,
                                  n_heads=self.num_heads, gh=gh, gw=gw, dh=dh, scale=float(self.scale))

    def _project(self, o: O.BF, residual: Optional[torch.Tensor], split: bool) -> torch.Tensor:
        return O.linear(o, _operand(self.proj, "weight", split), _f32(self.proj.bias), residual=residual, out_f32=True)[0]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        split = _guard(self, x, 4)
        b, gh, gw, d = x.shape
        h = O.cast(x.float().reshape(-1, d).contiguous(), split)
        return self._project(self._core(h, b, gh, gw, split), None, split).view(b, gh, gw, d)


class Block(nn.Module):
    """norm1 -> (windowed) attention -> + shortcut -> norm2 -> MLP -> + shortcut."""

    def __init__(self, dim: int, num_heads: int, mlp_ratio: float = 4.0, qkv_bias: bool = True, norm_layer: Type[nn.Module] = nn.LayerNorm,
                 act_layer: Type[nn.Module] = nn.GELU, use_rel_pos: bool = False, rel_pos_zero_init: bool = True, window_size: int = 0,
                 input_size: Optional[Tuple[int, int]] = None) -> None:
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, use_rel_pos=use_rel_pos, rel_pos_zero_init=rel_pos_zero_init,
                              input_size=input_size if window_size == 0 else (window_size, window_size))
        self.norm2 = norm_layer(dim)
        self.mlp = MLPBlock(embedding_dim=dim, mlp_dim=int(dim * mlp_ratio), act=act_layer)
        self.window_size = window_size

    @staticmethod
    def _norm(ln: nn.Module, rows: torch.Tensor, split: bool) -> O.BF:
        if not isinstance(ln, nn.LayerNorm) or len(ln.normalized_shape) != 1 or ln.weight is None:
            raise F.LvqError(f"Block: {type(ln).__name__} has no kernel here (nn.LayerNorm over the last dim, affine)")
        return O.layernorm(rows, _f32(ln.weight), _f32(ln.bias), ln.eps, split)[1]

    def _run(self, x: torch.Tensor, b: int, gh: int, gw: int, split: bool) -> torch.Tensor:
        """x [b * gh * gw, d] fp32 rows -> the same."""
        d, ws = x.shape[1], self.window_size
        h = self._norm(self.norm1, x, split)
        if ws > 0:
            hp = wp = 0

            def part(t):
                nonlocal hp, wp
                win, (hp, wp) = window_partition(t.view(b, gh, gw, d), ws)
                return win.reshape(-1, d).contiguous()
            h = _bf_map(h, part)
            o = self.attn._core(h, b * (hp // ws) * (wp // ws), ws, ws, split)
            o = _bf_map(o, lambda t: window_unpartition(t.view(-1, ws, ws, d), ws, (hp, wp), (gh, gw)).view(-1, d))
        else:
            o = self.attn._core(h, b, gh, gw, split)
        x = self.attn._project(o, x, split)
        return self.mlp._run(self._norm(self.norm2, x, split), x, split)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        split = _guard(self, x, 4)
        b, gh, gw, d = x.shape
        return self._run(x.float().reshape(-1, d).contiguous(), b, gh, gw, split).view(b, gh, gw, d)


def _conv(conv: nn.Conv2d, x: O.BF, b: int, h: int, w: int, split: bool, planes: bool):
    """One bias-free 3 x 3 nn.Conv2d (padding 1, stride 1 or 2) on channels-last operand planes x [b * h * w, c_in]: lvq_conv2d per
    chunk of at most 512 output channels, written at its channel offset.  Returns (planes BF [b * oh * ow, c_out] | fp32 [b, c_out, oh, ow], oh, ow)."""
    L = F.lib()
    k, s, c_in, c_out = conv.kernel_size[0], conv.stride[0], conv.in_channels, conv.out_channels
    if (tuple(conv.kernel_size), tuple(conv.padding), tuple(conv.dilation), conv.groups) != ((3, 3), (1, 1), (1, 1), 1) or conv.bias is not None \
            or tuple(conv.stride) not in ((1, 1), (2, 2)) or c_in % 32 or c_out % 64:
        raise F.LvqError(f"lvq_conv2d: Conv2d({c_in} -> {c_out}, kernel {tuple(conv.kernel_size)}, stride {tuple(conv.stride)}) is outside the "
                         "kernel family (3 x 3, padding 1, stride 1 / 2, no bias, c_in a multiple of 32, c_out of 64)")
    oh, ow = L.lvq_conv2d_out_size(h, k, s), L.lvq_conv2d_out_size(w, k, s)
    dev = x[0].device
    out_bf = O._bf_empty((b * oh * ow, c_out), dev, split) if planes else (None, None)
    out32 = None if planes else torch.empty((b, c_out, oh, ow), dtype=torch.float32, device=dev)
    for c0 in range(0, c_out, 512):
        c1 = min(c_out, c0 + 512)
        wh, wl = _cached(conv, ("conv", c0, c1, split), (conv.weight,),
                         lambda: O.conv2d_pack_weights(conv.weight.detach().float()[c0:c1].contiguous(), c1 - c0, c_in, k, False, split))
        F.check(L.lvq_conv2d(F.ptr(x[0]), F.ptr(x[1]), b, h, w, c_in, F.ptr(wh), F.ptr(wl), c1 - c0,
                             k, s, F.ptr(None), F.ptr(None), 0, F.ptr(out_bf[0]), F.ptr(out_bf[1]), F.ptr(out32),
                             c_out, c0, F.stream_ptr(dev)), "lvq_conv2d")
    return (out_bf if planes else out32), oh, ow


class ImageEncoderViT(nn.Module):
    def __init__(self, img_size: int = 1024, patch_size: int = 16, in_chans: int = 3, embed_dim: int = 768, depth: int = 12, num_heads: int = 12,
                 mlp_ratio: float = 4.0, out_chans: int = 256, qkv_bias: bool = True, norm_layer: Type[nn.Module] = nn.LayerNorm,
                 act_layer: Type[nn.Module] = nn.GELU, use_abs_pos: bool = True, use_rel_pos: bool = False, rel_pos_zero_init: bool = True,
                 window_size: int = 0, global_attn_indexes: Tuple[int, ...] = ()) -> None:
        super().__init__()
        self.img_size = img_size
        self.patch_embed = PatchEmbed(kernel_size=(patch_size, patch_size), stride=(patch_size, patch_size), in_chans=in_chans, embed_dim=embed_dim)
        grid = img_size // patch_size
        self.pos_embed: Optional[nn.Parameter] = None
        if use_abs_pos:
            self.pos_embed = nn.Parameter(torch.zeros(1, grid, grid, embed_dim))
        self.blocks = nn.ModuleList()
        for i in range(depth):
            self.blocks.append(Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, norm_layer=norm_layer,
                                     act_layer=act_layer, use_rel_pos=use_rel_pos, rel_pos_zero_init=rel_pos_zero_init,
                                     window_size=0 if i in global_attn_indexes else window_size, input_size=(grid, grid)))
        self.neck = nn.Sequential(nn.Conv2d(embed_dim, out_chans, kernel_size=1, bias=False), LayerNorm2d(out_chans),
                                  nn.Conv2d(out_chans, out_chans, kernel_size=3, padding=1, bias=False), LayerNorm2d(out_chans))
        self.net_2 = nn.Conv2d(256, 512, kernel_size=3, stride=2, padding=1, bias=False)
        self.net_3 = nn.Conv2d(512, 1024, kernel_size=3, stride=2, padding=1, bias=False)
        self.precision: Optional[str] = None          # None -> "bf16x3"

    def _pos_table(self, g: int) -> Optional[torch.Tensor]:
        """pos_embed as the GEMM's row table [g * g, d]; another grid is resized (bicubic, antialiased), once per weights version."""
        p = self.pos_embed
        if p is None:
            return None

        def build():
            t = p.detach().float()
            if t.shape[1] != g:
                t = TF.interpolate(t.permute(0, 3, 1, 2), size=(g, g), mode="bicubic", antialias=True, align_corners=False).permute(0, 2, 3, 1)
            return t.reshape(g * g, -1).contiguous()
        return _cached(self, ("pos", g), (p,), build)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        split = _guard(self, x, 4)
        b = x.shape[0]
        p = self.patch_embed.proj.kernel_size
        gh, gw = x.shape[2] // p[0], x.shape[3] // p[1]
        if self.pos_embed is not None and gh != gw:
            raise F.LvqError(f"ImageEncoderViT: pos_embed is resized to a square grid; a {gh} x {gw} patch grid does not fit it")
        tok, gh, gw = self.patch_embed._run(x.float().contiguous(), split, self._pos_table(gh))
        for blk in self.blocks:
            tok = blk._run(tok, b, gh, gw, split)
        # neck: 1 x 1 conv (GEMM) -> LayerNorm2d -> 3 x 3 conv -> LayerNorm2d, on channels-last rows
        c0, n0, c1, n1 = self.neck
        if tuple(c0.kernel_size) != (1, 1) or c0.bias is not None or c0.out_channels % 32:
            raise F.LvqError("ImageEncoderViT: neck[0] runs as a GEMM (1 x 1, no bias, out_chans a multiple of 32)")
        y, _ = O.linear(O.cast(tok, split), _operand(c0, "weight", split, (c0.out_channels, c0.in_channels)), None, out_f32=True)
        _, planes = n0._rows(y, split)
        y, _, _ = _conv(c1, planes, b, gh, gw, split, planes=False)
        _, planes = n1._rows(y.permute(0, 2, 3, 1).reshape(-1, c1.out_channels).contiguous(), split)
        planes, oh, ow = _conv(self.net_2, planes, b, gh, gw, split, planes=True)
        return _conv(self.net_3, planes, b, oh, ow, split, planes=False)[0]


# ------------------------------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------------------------------
CHECKPOINT_PREFIXES = ("image_encoder.", "vision_tower_high.")


def _build_sam(encoder_embed_dim, encoder_depth, encoder_num_heads, encoder_global_attn_indexes, checkpoint=None):
    enc = ImageEncoderViT(depth=encoder_depth, embed_dim=encoder_embed_dim, img_size=1024, mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                          num_heads=encoder_num_heads, patch_size=16, qkv_bias=True, use_rel_pos=True,
                          global_attn_indexes=encoder_global_attn_indexes, window_size=14, out_chans=256)
    if checkpoint is not None:
        if not os.path.exists(checkpoint):
            raise FileNotFoundError(f"SAM checkpoint not found: {checkpoint}")
        sd = torch.load(checkpoint, map_location="cpu")
        # official SAM checkpoints carry "image_encoder.", the multimodal ones "vision_tower_high." (loaded strictly); anything else as it is
        prefix = next((p for p in CHECKPOINT_PREFIXES if any(k.startswith(p) for k in sd)), None)
        if prefix is not None:
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        missing, unexpected = enc.load_state_dict(sd, strict=prefix == "vision_tower_high.")
        if missing or unexpected:
            print(f"[SAM] {checkpoint}: missing {list(missing)}, unexpected {list(unexpected)}")
    return enc


def build_sam_vit_b(checkpoint=None):
    return _build_sam(encoder_embed_dim=768, encoder_depth=12, encoder_num_heads=12, encoder_global_attn_indexes=[2, 5, 8, 11], checkpoint=checkpoint)
