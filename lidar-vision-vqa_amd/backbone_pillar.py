"""The sparse 2-D pillar backbones between DynamicPillarVFESimple2D and BaseBEVBackboneV1 (PillarNet): the reference's module API
(pcdet/models/backbones_3d/spconv_backbone_2d.py:8-300) on the HIP kernels of csrc/sparse_conv.hip and csrc/conv2d.hip.

  post_act_block, SparseBasicBlock   the 2-D twins of backbone3d's (SubMConv2d / SparseConv2d + BatchNorm1d + ReLU; conv + bn + residual)
  post_act_block_dense, BasicBlock   nn.Conv2d / nn.BatchNorm2d parameter containers, as in backbone2d.py: forward never calls them
  PillarBackBone8x, PillarRes18BackBone8x   conv1 .. conv4 sparse (conv4 is the 256-channel layer of lvq_sparse_conv), x_conv4 densified
                          by lvq_sparse_to_dense, conv5 dense: lvq_conv2d_to_planes once, then lvq_conv2d (stride 2) and either two more
                          lvq_conv2d or, per BasicBlock, lvq_conv2d + lvq_conv2d_res (the block's input planes are the residual; the
                          conv bias is folded into the shift).  Activations stay operand planes; fp32 is written for x_conv5 only.

Both register in backbone3d.backbones_3d_all under the reference's NAME strings.  Inference only, "bf16x3" (default) or "bf16", as backbone3d.
"""
from __future__ import annotations

from functools import partial
from typing import Optional

import torch
import torch.nn as nn

from . import _ffi as F
from . import autograd_route as AG
from . import backbone2d as B2
from . import backbone3d as B3
from .backbone3d import SparseConv2d, SparseConvTensor, SparseSequential, SubMConv2d


def post_act_block(in_channels, out_channels, kernel_size, indice_key=None, stride=1, padding=0, conv_type="subm", norm_fn=None):
    if conv_type == "subm":
        conv = SubMConv2d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key)
    elif conv_type == "spconv":
        conv = SparseConv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False, indice_key=indice_key)
    else:
        raise NotImplementedError(f"conv_type {conv_type!r} (SparseInverseConv2d has no kernel here)")
    return SparseSequential(conv, norm_fn(out_channels), nn.ReLU())


def post_act_block_dense(in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, norm_fn=None):
    return nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding=padding, dilation=dilation, bias=False),
                         norm_fn(out_channels), nn.ReLU())


class SparseBasicBlock(B3.SparseBasicBlock):
    conv_cls = SubMConv2d

    def __init__(self, inplanes, planes, stride=1, norm_fn=None, downsample=None, indice_key=None):
        super().__init__(inplanes, planes, stride=stride, norm_fn=norm_fn, downsample=downsample, indice_key=indice_key)


class BasicBlock(nn.Module):
    """Parameter container of the dense residual block: y = relu(bn2(conv2(relu(bn1(conv1(x))))) + x), run by the backbone as
    lvq_conv2d + lvq_conv2d_res."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, norm_fn=None, downsample=None):
        super().__init__()
        assert norm_fn is not None
        if downsample is not None or stride != 1:
            raise NotImplementedError("BasicBlock: stride 1 and no downsample (the residual is the block's own input)")
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=True)
        self.bn1 = norm_fn(planes)
        self.relu = nn.ReLU()
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=True)
        self.bn2 = norm_fn(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        raise F.LvqError("BasicBlock is a parameter container: PillarRes18BackBone8x runs it on lvq_conv2d / lvq_conv2d_res")


class _PillarBackBone8x(nn.Module):
    """What the two pillar backbones share: the bookkeeping and the forward."""

    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        g = [int(v) for v in grid_size]
        self.sparse_shape = [g[1], g[0]]               # grid_size[[1, 0]]
        self.precision: Optional[str] = None          # None -> "bf16x3"
        self.num_point_features = 256
        self.backbone_channels = {"x_conv1": 32, "x_conv2": 64, "x_conv3": 128, "x_conv4": 256, "x_conv5": 256}

    def _dense_plan(self):
        """conv5 as [(first layer, second layer or None)]: a post_act_block_dense is one layer, a BasicBlock two with a residual."""
        plan = self.__dict__.get("_plan_cache")
        if plan is None:
            plan = []
            for m in self.conv5:
                if isinstance(m, BasicBlock):
                    plan.append((B2._Layer(m.conv1, m.bn1, True), B2._Layer(m.conv2, m.bn2, True)))
                else:
                    (layer, pad), = B2._layers(m)
                    assert pad == 0
                    plan.append((layer, None))
            self.__dict__["_plan_cache"] = plan
        return plan

    def _conv5(self, x4: torch.Tensor, split: bool) -> torch.Tensor:
        plan = self._dense_plan()
        h, w = x4.shape[2:]
        for first, _ in plan:
            h, w = first.out_size(h, w)
        out = torch.empty((x4.shape[0], plan[-1][0].c_out, h, w), dtype=torch.float32, device=x4.device)
        cur = B2.to_planes(x4, split)
        for i, (first, second) in enumerate(plan):
            last = dict(f32=out) if i == len(plan) - 1 else {}
            if second is None:
                cur = first.run(cur, split, **last)
            else:
                cur = second.run(first.run(cur, split), split, residual=cur, **last)
        return out

    def forward(self, batch_dict):
        name = type(self).__name__
        feats, coords = batch_dict["pillar_features"], batch_dict["pillar_coords"]
        if AG.wanted(self, feats):
            raise F.LvqError(f"{name}: inference-only kernels (BatchNorm folded); call it in eval() mode under torch.no_grad()")
        F.require_cuda(feats, coords)
        mode = self.precision or B3.DEFAULT_MODE
        if mode not in B3.MODES:
            raise F.LvqError(f"{name} runs in {B3.MODES}, not {mode!r}")
        x = SparseConvTensor(feats.float().contiguous(), coords.to(torch.int32).contiguous(), self.sparse_shape, batch_dict["batch_size"],
                             None, mode)
        x_conv1 = self.conv1(x)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4 = self.conv4(x_conv3).dense()
        x_conv5 = self._conv5(x_conv4, mode == "bf16x3")
        batch_dict.update({"multi_scale_2d_features": {"x_conv1": x_conv1, "x_conv2": x_conv2, "x_conv3": x_conv3, "x_conv4": x_conv4,
                                                       "x_conv5": x_conv5}})
        batch_dict.update({"multi_scale_2d_strides": {"x_conv1": 1, "x_conv2": 2, "x_conv3": 4, "x_conv4": 8, "x_conv5": 16}})
        return batch_dict


class PillarBackBone8x(_PillarBackBone8x):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__(model_cfg, input_channels, grid_size, **kwargs)
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        block = partial(post_act_block, norm_fn=norm_fn)
        self.conv1 = SparseSequential(block(32, 32, 3, padding=1, indice_key="subm1"), block(32, 32, 3, padding=1, indice_key="subm1"))
        self.conv2 = SparseSequential(block(32, 64, 3, stride=2, padding=1, indice_key="spconv2", conv_type="spconv"),
                                      block(64, 64, 3, padding=1, indice_key="subm2"), block(64, 64, 3, padding=1, indice_key="subm2"))
        self.conv3 = SparseSequential(block(64, 128, 3, stride=2, padding=1, indice_key="spconv3", conv_type="spconv"),
                                      block(128, 128, 3, padding=1, indice_key="subm3"), block(128, 128, 3, padding=1, indice_key="subm3"))
        self.conv4 = SparseSequential(block(128, 256, 3, stride=2, padding=1, indice_key="spconv4", conv_type="spconv"),
                                      block(256, 256, 3, padding=1, indice_key="subm4"), block(256, 256, 3, padding=1, indice_key="subm4"))
        dense_block = partial(post_act_block_dense, norm_fn=partial(nn.BatchNorm2d, eps=1e-3, momentum=0.01))
        self.conv5 = nn.Sequential(dense_block(256, 256, 3, stride=2, padding=1), dense_block(256, 256, 3, padding=1),
                                   dense_block(256, 256, 3, padding=1))


class PillarRes18BackBone8x(_PillarBackBone8x):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__(model_cfg, input_channels, grid_size, **kwargs)
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        block = partial(post_act_block, norm_fn=norm_fn)
        res = partial(SparseBasicBlock, norm_fn=norm_fn)
        self.conv1 = SparseSequential(res(32, 32, indice_key="res1"), res(32, 32, indice_key="res1"))
        self.conv2 = SparseSequential(block(32, 64, 3, stride=2, padding=1, indice_key="spconv2", conv_type="spconv"),
                                      res(64, 64, indice_key="res2"), res(64, 64, indice_key="res2"))
        self.conv3 = SparseSequential(block(64, 128, 3, stride=2, padding=1, indice_key="spconv3", conv_type="spconv"),
                                      res(128, 128, indice_key="res3"), res(128, 128, indice_key="res3"))
        self.conv4 = SparseSequential(block(128, 256, 3, stride=2, padding=1, indice_key="spconv4", conv_type="spconv"),
                                      res(256, 256, indice_key="res4"), res(256, 256, indice_key="res4"))
        norm_fn = partial(nn.BatchNorm2d, eps=1e-3, momentum=0.01)
        self.conv5 = nn.Sequential(post_act_block_dense(256, 256, 3, norm_fn=norm_fn, stride=2, padding=1), BasicBlock(256, 256, norm_fn=norm_fn),
                                   BasicBlock(256, 256, norm_fn=norm_fn))


B3.backbones_3d_all["PillarBackBone8x"] = PillarBackBone8x
B3.backbones_3d_all["PillarRes18BackBone8x"] = PillarRes18BackBone8x
