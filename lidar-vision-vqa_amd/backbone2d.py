"""The dense 2-D BEV backbone between the scattered canvas and `spatial_features_2d`: the reference's module API
(pcdet/models/backbones_2d/base_bev_backbone.py:6-204) on the HIP kernels of csrc/conv2d.hip.

  BaseBEVBackbone(model_cfg, input_channels)   reads data_dict['spatial_features'] [B, C, H, W], writes data_dict['spatial_features_2d']
  BaseBEVBackboneV1(model_cfg, **kwargs)       reads data_dict['multi_scale_2d_features']['x_conv4' / 'x_conv5'], writes the same key
  backbones_2d_all                             registry with the reference's NAME strings

`blocks` / `deblocks` hold nn.ZeroPad2d / Conv2d / BatchNorm2d / ReLU / ConvTranspose2d in the reference's nn.Sequential order, so
state_dict() keys and shapes are the reference's (checkpoints load with strict=True) and default initialisation consumes the RNG in the
reference's order.  forward never calls these containers: the input goes once through lvq_conv2d_to_planes, every conv + BatchNorm +
ReLU is ONE lvq_conv2d / lvq_deconv2d launch with the folded eval-mode statistics (eps read from the module) in its epilogue, activations
stay channels-last bf16 operand planes between layers, and the deblocks write their channel range of the concatenated result directly
(fp32 [B, C, H, W] when that result is the module's output).

Inference only: train() mode, or a call with gradients in reach, raises LvqError, and so do CPU tensors (no fallback).
Precision: `precision` of the backbone, "bf16x3" (hi + lo operands, three MFMA passes: the default) or "bf16" (plain operands).
Packed weights and the folded scale / shift are cached per parameter version and mode.
UPSAMPLE_STRIDES below 1 become a strided conv of kernel = stride = int(round(1 / stride)).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import _ffi as F
from . import ops
from .head_common import DEFAULT_MODE, MODES, _get, cached_plan, guard  # noqa: F401  (the precision names are re-exported)

FAMILY = "c_in 1 .. 512, c_out a multiple of 64 in 64 .. 512; kernel 3 at stride 1 / 2, or kernel = stride in 1, 2, 4"
_lib = F.lib


def pad32(c: int) -> int:
    return (int(c) + 31) // 32 * 32


class Planes:
    """Channels-last operand planes [B, H, W, Cp] (int16 storage of bf16): hi and, in the bf16x3 form, lo."""

    def __init__(self, batch: int, h: int, w: int, c: int, split: bool, device):
        self.batch, self.h, self.w, self.c = int(batch), int(h), int(w), int(c)
        shape = (self.batch, self.h, self.w, pad32(c))
        self.hi = torch.empty(shape, dtype=torch.int16, device=device)
        self.lo = torch.empty(shape, dtype=torch.int16, device=device) if split else None


def to_planes(x: torch.Tensor, split: bool) -> Planes:
    """lvq_conv2d_to_planes: [B, C, H, W] fp32 -> Planes."""
    F.require_cuda(x)
    b, c, h, w = x.shape
    if _lib().lvq_conv2d_plane_elems(b, c, h, w) == 0:
        raise F.LvqError(f"lvq_conv2d_to_planes: a [{b}, {c}, {h}, {w}] canvas is outside the kernel family ({FAMILY})")
    p = Planes(b, h, w, c, split, x.device)
    F.check(_lib().lvq_conv2d_to_planes(F.ptr(x), b, c, h, w, F.ptr(p.hi), F.ptr(p.lo), F.stream_ptr(x.device)),
            "lvq_conv2d_to_planes")
    return p


class _Layer:
    """One conv / transposed conv + BatchNorm2d + ReLU of a block or deblock: reads the containers' tensors, never calls them.
    A conv bias (the dense BasicBlock of the pillar backbones has one) is folded into the shift: shift' = bias * scale + shift."""

    def __init__(self, conv: nn.Module, bn: Optional[nn.BatchNorm2d], relu: bool):
        self.conv, self.bn, self.relu = conv, bn, relu
        self.transposed = isinstance(conv, nn.ConvTranspose2d)
        k, s, p = conv.kernel_size, conv.stride, conv.padding
        if k[0] != k[1] or s[0] != s[1] or p[0] != p[1] or conv.groups != 1 or tuple(conv.dilation) != (1, 1):
            raise NotImplementedError("dense 2-D convolutions: square kernels, dilation 1, groups 1")
        if conv.bias is not None and (bn is None or self.transposed):
            raise NotImplementedError("dense 2-D convolutions: a bias only in front of a BatchNorm2d (it is folded into the shift)")
        self.kernel, self.stride, self.padding = int(k[0]), int(s[0]), int(p[0])
        self.c_in, self.c_out = conv.in_channels, conv.out_channels
        self._cache = {}

    def out_size(self, h: int, w: int, pad: int = 0) -> Tuple[int, int]:
        """torch's output size; `pad` is the ZeroPad2d in front of the conv (the reference pads 1 and convolves with padding 0)."""
        if self.transposed:
            return h * self.stride, w * self.stride
        p = self.padding + pad
        return (h + 2 * p - self.kernel) // self.stride + 1, (w + 2 * p - self.kernel) // self.stride + 1

    def packed(self, split: bool):
        p = self.conv.weight

        def build():
            hi, lo = ops.conv2d_pack_weights(p.detach().float().contiguous(), self.c_out, self.c_in, self.stride if self.transposed else self.kernel,
                                             self.transposed, split)
            return hi.view(torch.int16), None if lo is None else lo.view(torch.int16)
        return F.derived(self._cache, ("w", split), (p,), build)

    def folded(self):
        bn = self.bn
        if bn is None:
            return None, None
        bias = self.conv.bias

        def build():
            scale, shift = F.fold_batchnorm(bn)
            if bias is not None:
                shift = (bias.detach().float() * scale + shift).contiguous()
            return scale, shift
        return F.derived(self._cache, "bn", (bn.weight, bn.bias, bn.running_mean, bn.running_var, bias), build, (bn.eps,))

    def run(self, x: Planes, split: bool, pad: int = 0, planes: Optional[Planes] = None, f32: Optional[torch.Tensor] = None,
            c_off: int = 0, residual: Optional[Planes] = None) -> Optional[Planes]:
        """One launch.  The result goes to channels c_off .. c_off + c_out - 1 of `planes` (made here when neither target is given)
        and / or of `f32` [B, C_total, OH, OW].  `residual` (planes of the output's own size and channels) is added before the ReLU:
        lvq_conv2d_res."""
        if x.c != self.c_in:
            raise F.LvqError(f"{type(self.conv).__name__}: expected {self.c_in} input channels, got {x.c}")
        if not self.transposed and (self.kernel, self.padding + pad) not in ((3, 1), (self.stride, 0)):
            raise F.LvqError(f"lvq_conv2d: kernel {self.kernel} with padding {self.padding + pad} is outside the kernel family ({FAMILY})")
        hi, lo = self.packed(split)
        scale, shift = self.folded()
        oh, ow = self.out_size(x.h, x.w, pad)
        if oh <= 0 or ow <= 0:
            raise F.LvqError(f"{type(self.conv).__name__}: a {x.h} x {x.w} canvas leaves no output pixel")
        dev = x.hi.device
        if planes is None and f32 is None:
            planes = Planes(x.batch, oh, ow, self.c_out, split, dev)
        targets = ([] if planes is None else [(planes.h, planes.w, planes.hi.shape[3])]) + ([] if f32 is None else [(*f32.shape[2:], f32.shape[1])])
        c_total = targets[0][2]                      # the pixel pitch of the planes = the channel count of the fp32 buffer
        if any(t != (oh, ow, c_total) for t in targets):
            raise F.LvqError(f"{type(self.conv).__name__}: output {oh} x {ow} does not fit its target(s) {targets} (h, w, channels)")
        out = (F.ptr(planes.hi if planes is not None else None), F.ptr(planes.lo if planes is not None else None), F.ptr(f32), c_total,
               c_off, F.stream_ptr(dev))
        head = (F.ptr(x.hi), F.ptr(x.lo), x.batch, x.h, x.w, self.c_in, F.ptr(hi), F.ptr(lo), self.c_out)
        tail = (F.ptr(scale), F.ptr(shift), int(self.relu))
        if residual is not None:
            if self.transposed or (residual.batch, residual.h, residual.w, residual.c) != (x.batch, oh, ow, self.c_out):
                raise F.LvqError(f"{type(self.conv).__name__}: the residual must be [{x.batch}, {oh}, {ow}, {self.c_out}] planes of a conv")
            F.check(_lib().lvq_conv2d_res(*head, self.kernel, self.stride, F.ptr(scale), F.ptr(shift), F.ptr(residual.hi),
                                          F.ptr(residual.lo if split else None), int(self.relu), *out), "lvq_conv2d_res")
        elif self.transposed:
            F.check(_lib().lvq_deconv2d(*head, self.stride, *tail, *out), "lvq_deconv2d")
        else:
            F.check(_lib().lvq_conv2d(*head, self.kernel, self.stride, *tail, *out), "lvq_conv2d")
        return planes


def _layers(seq: nn.Sequential) -> List[Tuple[_Layer, int]]:
    """(layer, zero padding in front of it) for every conv of a Sequential; BatchNorm2d and ReLU fold into the conv before them."""
    mods, out, i, pad = list(seq), [], 0, 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.ZeroPad2d):
            if len(set(m.padding)) != 1:
                raise NotImplementedError("ZeroPad2d: one padding for all four sides")
            pad = int(m.padding[0])
            i += 1
        elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            bn, relu, j = None, False, i + 1
            if j < len(mods) and isinstance(mods[j], nn.BatchNorm2d):
                bn, j = mods[j], j + 1
            if j < len(mods) and isinstance(mods[j], nn.ReLU):
                relu, j = True, j + 1
            out.append((_Layer(m, bn, relu), pad))
            pad, i = 0, j
        else:
            raise F.LvqError(f"{type(m).__name__} follows no convolution: it has no kernel here")
    return out


def _conv_block(c_in, c_out, stride, n_layers) -> nn.Sequential:
    mods = [nn.ZeroPad2d(1), nn.Conv2d(c_in, c_out, kernel_size=3, stride=stride, padding=0, bias=False),
            nn.BatchNorm2d(c_out, eps=1e-3, momentum=0.01), nn.ReLU()]
    for _ in range(n_layers):
        mods.extend([nn.Conv2d(c_out, c_out, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(c_out, eps=1e-3, momentum=0.01), nn.ReLU()])
    return nn.Sequential(*mods)


def _deblock(c_in, c_out, stride, transposed: bool) -> nn.Sequential:
    if transposed:
        conv = nn.ConvTranspose2d(c_in, c_out, stride, stride=stride, bias=False)
    else:
        s = int(round(1 / stride))
        conv = nn.Conv2d(c_in, c_out, s, stride=s, bias=False)
    return nn.Sequential(conv, nn.BatchNorm2d(c_out, eps=1e-3, momentum=0.01), nn.ReLU())


class _Backbone2d(nn.Module):
    def _plan(self):
        return cached_plan(self, lambda: dict(blocks=[_layers(b) for b in self.blocks], deblocks=[_layers(d) for d in self.deblocks]))

    def _guard(self, *tensors) -> bool:
        return guard(self, "BatchNorm folded", *tensors)

    @staticmethod
    def _chain(layers, x: Planes, split: bool, **last) -> Planes:
        for i, (layer, pad) in enumerate(layers):
            x = layer.run(x, split, pad, **(last if i == len(layers) - 1 else {}))
        return x

    @staticmethod
    def _aligned(sizes, what):
        if len(set(sizes)) > 1:
            raise F.LvqError(f"{what}: the maps to concatenate have sizes " + ", ".join(f"{h} x {w}" for h, w in sizes) +
                             " (the canvas must be divisible by the total stride)")

    @staticmethod
    def _sizes(layers, h, w):
        for layer, pad in layers:
            h, w = layer.out_size(h, w, pad)
        return h, w


class BaseBEVBackbone(_Backbone2d):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        if _get(model_cfg, "LAYER_NUMS") is not None:
            layer_nums, layer_strides, num_filters = model_cfg.LAYER_NUMS, model_cfg.LAYER_STRIDES, model_cfg.NUM_FILTERS
            assert len(layer_nums) == len(layer_strides) == len(num_filters)
        else:
            layer_nums = layer_strides = num_filters = []
        if _get(model_cfg, "UPSAMPLE_STRIDES") is not None:
            upsample_strides, num_upsample_filters = model_cfg.UPSAMPLE_STRIDES, model_cfg.NUM_UPSAMPLE_FILTERS
            assert len(upsample_strides) == len(num_upsample_filters)
        else:
            upsample_strides = num_upsample_filters = []
        num_levels = len(layer_nums)
        c_in_list = [input_channels, *num_filters[:-1]]
        self.blocks = nn.ModuleList()
        self.deblocks = nn.ModuleList()
        for idx in range(num_levels):
            self.blocks.append(_conv_block(c_in_list[idx], num_filters[idx], layer_strides[idx], layer_nums[idx]))
            if len(upsample_strides) > 0:
                stride = upsample_strides[idx]
                transposed = stride > 1 or (stride == 1 and not _get(model_cfg, "USE_CONV_FOR_NO_STRIDE", False))
                self.deblocks.append(_deblock(num_filters[idx], num_upsample_filters[idx], stride, transposed))
        c_in = sum(num_upsample_filters)
        if len(upsample_strides) > num_levels:
            self.deblocks.append(_deblock(c_in, c_in, upsample_strides[-1], True))
        self.num_bev_features = c_in
        self.precision: Optional[str] = None          # None -> "bf16x3"

    def forward(self, data_dict):
        x = data_dict["spatial_features"]
        split = self._guard(x)
        x = x.float().contiguous()
        plan = self._plan()
        blocks, deblocks = plan["blocks"], plan["deblocks"]
        n, dev = len(blocks), x.device
        if n == 0:
            data_dict["spatial_features_2d"] = x
            return data_dict
        extra = deblocks[n][0][0] if len(deblocks) > n else None
        # sizes first: the concat must line up before anything is launched
        sizes, chans, (h, w) = [], [], x.shape[2:]
        for i in range(n):
            h, w = self._sizes(blocks[i], h, w)
            sizes.append(self._sizes(deblocks[i], h, w) if deblocks else (h, w))
            chans.append((deblocks[i] if deblocks else blocks[i])[-1][0].c_out)
        self._aligned(sizes, "BaseBEVBackbone")
        c_cat, (ch, cw) = sum(chans), sizes[0]
        cat_f32 = cat_planes = None
        if extra is None:
            cat_f32 = torch.empty((x.shape[0], c_cat, ch, cw), dtype=torch.float32, device=dev)
        else:
            cat_planes = Planes(x.shape[0], ch, cw, c_cat, split, dev)
        cur, off = to_planes(x, split), 0
        for i in range(n):
            if deblocks:
                cur = self._chain(blocks[i], cur, split)
                self._chain(deblocks[i], cur, split, planes=cat_planes, f32=cat_f32, c_off=off)
            elif i + 1 < n:                            # no deblocks: a block's output is the next block's input AND a part of the result
                mid = self._chain(blocks[i][:-1], cur, split)
                layer, pad = blocks[i][-1]
                layer.run(mid, split, pad, f32=cat_f32, c_off=off)
                cur = layer.run(mid, split, pad)
            else:
                self._chain(blocks[i], cur, split, planes=cat_planes, f32=cat_f32, c_off=off)
            off += chans[i]
        if extra is not None:
            oh, ow = extra.out_size(ch, cw)
            cat_f32 = torch.empty((x.shape[0], extra.c_out, oh, ow), dtype=torch.float32, device=dev)
            extra.run(cat_planes, split, f32=cat_f32)
        data_dict["spatial_features_2d"] = cat_f32
        return data_dict


class BaseBEVBackboneV1(_Backbone2d):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums, num_filters = model_cfg.LAYER_NUMS, model_cfg.NUM_FILTERS
        assert len(layer_nums) == len(num_filters) == 2
        num_upsample_filters, upsample_strides = model_cfg.NUM_UPSAMPLE_FILTERS, model_cfg.UPSAMPLE_STRIDES
        assert len(num_upsample_filters) == len(upsample_strides)
        num_levels = len(layer_nums)
        self.blocks = nn.ModuleList()
        self.deblocks = nn.ModuleList()
        for idx in range(num_levels):
            self.blocks.append(_conv_block(num_filters[idx], num_filters[idx], 1, layer_nums[idx]))
            if len(upsample_strides) > 0:
                stride = upsample_strides[idx]
                self.deblocks.append(_deblock(num_filters[idx], num_upsample_filters[idx], stride, stride >= 1))
        c_in = sum(num_upsample_filters)
        if len(upsample_strides) > num_levels:
            self.deblocks.append(_deblock(c_in, c_in, upsample_strides[-1], True))
        self.num_bev_features = c_in
        self.precision: Optional[str] = None

    def forward(self, data_dict):
        feats = data_dict["multi_scale_2d_features"]
        x4, x5 = feats["x_conv4"], feats["x_conv5"]
        split = self._guard(x4, x5)
        x4, x5 = x4.float().contiguous(), x5.float().contiguous()
        plan = self._plan()
        blocks, deblocks = plan["blocks"], plan["deblocks"]
        if x4.shape[0] != x5.shape[0]:
            raise F.LvqError(f"BaseBEVBackboneV1: x_conv4 holds {x4.shape[0]} scenes, x_conv5 {x5.shape[0]}")
        s0 = self._sizes(deblocks[0], *x4.shape[2:])
        s1 = self._sizes(deblocks[1], *self._sizes(blocks[1], *x5.shape[2:]))
        self._aligned([s0, s1], "BaseBEVBackboneV1")
        c0, c1 = deblocks[0][-1][0].c_out, deblocks[1][-1][0].c_out
        cat = Planes(x4.shape[0], *s0, c0 + c1, split, x4.device)
        self._chain(deblocks[0], to_planes(x4, split), split, planes=cat, c_off=0)
        self._chain(deblocks[1], self._chain(blocks[1], to_planes(x5, split), split), split, planes=cat, c_off=c0)
        oh, ow = self._sizes(blocks[0], *s0)
        out = torch.empty((x4.shape[0], blocks[0][-1][0].c_out, oh, ow), dtype=torch.float32, device=x4.device)
        self._chain(blocks[0], cat, split, f32=out)
        data_dict["spatial_features_2d"] = out
        return data_dict


backbones_2d_all = {"BaseBEVBackbone": BaseBEVBackbone, "BaseBEVBackboneV1": BaseBEVBackboneV1}
