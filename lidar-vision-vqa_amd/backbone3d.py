"""The sparse 3-D convolution backbones between MeanVFE and the BEV canvas: the reference's module API
(pcdet/models/backbones_3d/spconv_backbone_voxelnext.py:8-225 and spconv_backbone.py:8-295, spconv 2.x layers through
pcdet/utils/spconv_utils.py) on the HIP kernels of csrc/sparse_conv.hip.  spconv itself is not a dependency.

  SubMConv3d / SubMConv2d / SparseConv3d / SparseConv2d   parameter containers (weight [C_out, *kernel, C_in], optional bias) whose
                          forward is two C-ABI calls: lvq_sparse_conv_rules (once per indice_key: layers that share a key share the
                          neighbour table, as in spconv) and lvq_sparse_conv (gather-form implicit GEMM + fused epilogue)
  SparseSequential        runs its children; a conv followed by BatchNorm1d (and ReLU) becomes ONE kernel launch with the folded
                          eval-mode statistics in its epilogue
  post_act_block, SparseBasicBlock, VoxelResBackBone8xVoxelNeXt, VoxelBackBone8x, VoxelResBackBone8x   the reference's containers
                          under the reference's names, so a checkpoint's `backbone_3d.*` entries load with strict=True.  The last two
                          (SECOND / CenterPoint / TransFusion / BEVFusion) end in a (3, 1, 1) stride (2, 1, 1) conv whose 3-D result
                          goes through bev.HeightCompression into backbone2d.BaseBEVBackbone.
  backbones_3d_all        registry with the reference's NAME strings (backbone_pillar.py adds the two pillar backbones)

Inference only: train() mode, or a call with gradients in reach, raises LvqError, and so do CPU tensors (no fallback).
Precision: `precision` of the backbone, "bf16x3" (hi + lo operands, three MFMA passes: the default here, it meets the 1e-3 parity bar)
or "bf16" (plain operands).  Packed weights and the folded scale / shift are cached per parameter version and mode.
Row order: a regular sparse conv returns its rows in ascending (b, z, y, x) order (spconv leaves it unspecified); everything
downstream addresses rows through coordinates.
"""
from __future__ import annotations

from functools import partial
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _ffi as F
from . import autograd_route as AG
from .bev import SparseTensor, bev_out

MODES = ("bf16x3", "bf16")
DEFAULT_MODE = "bf16x3"
_lib = F.lib


class SparseConvTensor(SparseTensor):
    """bev.SparseTensor + what a chain of layers shares: the neighbour tables by indice_key and the precision mode."""

    def __init__(self, features, indices, spatial_shape, batch_size, indice_dict: Optional[dict] = None, precision: Optional[str] = None):
        super().__init__(features, indices, spatial_shape, batch_size)
        self.indice_dict = indice_dict if indice_dict is not None else {}
        self.precision = precision

    def replace_feature(self, features: torch.Tensor) -> "SparseConvTensor":
        return SparseConvTensor(features, self.indices, self.spatial_shape, self.batch_size, self.indice_dict, self.precision)


def _tuple(v, nd) -> Tuple[int, ...]:
    return tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v),) * nd


def sparse_conv_rules(indices: torch.Tensor, spatial_shape, batch_size: int, kernel, stride, padding, subm: bool):
    """lvq_sparse_conv_rules: (out_indices, nbr [n_out, K], n_out_dev, out_shape).  For subm the output indices are the input's.
    Reads the row count once for a layer that changes the active set (the reference's torch.unique synchronises the same way)."""
    idx = indices if indices.dtype == torch.int32 else indices.to(torch.int32)
    idx = idx.contiguous()
    F.require_cuda(idx)
    n, cols = idx.shape
    nd = cols - 1
    L = _lib()
    dev = idx.device
    shape, k, s, p = [int(v) for v in spatial_shape], _tuple(kernel, nd), _tuple(stride, nd), _tuple(padding, nd)
    kvol = 1
    for v in k:
        kvol *= v
    out_shape = shape if subm else [(d + 2 * pp - kk) // ss + 1 for d, pp, kk, ss in zip(shape, p, k, s)]
    args = (nd, F.i32x(shape), batch_size, F.i32x(k), F.i32x(s), F.i32x(p), int(subm))
    n_out = torch.zeros((1,), dtype=torch.int32, device=dev)
    cells = batch_size
    kc = 1
    for d, kk, ss in zip(out_shape, k, s):
        cells *= d
        kc *= -(-kk // ss)
    full = max(1, min(n * (1 if subm else kc), cells))
    cap = full if subm else max(1, min(full, 4 * n + 64))      # LiDAR voxels reach ~2.8 sites each through a stride-2 layer
    while True:
        nbytes = L.lvq_sparse_conv_rules_workspace_bytes(n, *args)
        ws = F.workspace(nbytes, dev, "sprules", floor=1 << 20)
        out_idx = idx if subm else torch.empty((cap, cols), dtype=torch.int32, device=dev)
        nbr = torch.empty((cap, kvol), dtype=torch.int32, device=dev)
        rc = L.lvq_sparse_conv_rules(F.ptr(idx), n, *args, cap, F.ptr(None if subm else out_idx), F.ptr(nbr), F.ptr(n_out),
                                     F.ptr(ws), ws.numel(), F.stream_ptr(dev))
        F.check(rc, "lvq_sparse_conv_rules")
        if subm:
            return idx, nbr[:n], n_out, out_shape
        m = int(n_out.item())
        if m <= cap:
            return out_idx[:m], nbr[:m], n_out, out_shape
        cap = full                                   # more output sites than the first guess had room for: once more with the bound


class _SparseConv(nn.Module):
    """Parameter container with spconv 2.x's keys and shapes + the forward on the HIP kernels."""
    ndim = 3
    subm = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None,
                 **kwargs):
        super().__init__()
        nd = self.ndim
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.stride, self.padding = _tuple(kernel_size, nd), _tuple(stride, nd), _tuple(padding, nd)
        if _tuple(dilation, nd) != (1,) * nd or groups != 1:
            raise NotImplementedError("sparse convolutions: dilation 1 and groups 1 only")
        if self.subm and self.stride != (1,) * nd:
            raise NotImplementedError("submanifold convolutions have stride 1")
        self.indice_key = indice_key
        self.weight = nn.Parameter(torch.empty(self.out_channels, *self.kernel_size, self.in_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()
        object.__setattr__(self, "_cache", {})

    def reset_parameters(self):
        fan_in = self.in_channels
        for k in self.kernel_size:
            fan_in *= k
        bound = (1.0 / fan_in) ** 0.5
        nn.init.uniform_(self.weight, -bound * 3 ** 0.5, bound * 3 ** 0.5)
        if self.bias is not None:
            nn.init.uniform_(self.bias, -bound, bound)

    # ---- caches (per parameter version and precision mode) ----
    def _packed(self, split: bool):
        return F.derived(self._cache, ("w", split), (self.weight,), lambda: self._pack(split))

    def _pack(self, split: bool):
        L = _lib()
        kvol = 1
        for k in self.kernel_size:
            kvol *= k
        n = L.lvq_sparse_conv_packed_elems(self.out_channels, kvol, self.in_channels)
        if n == 0:
            raise F.LvqError(f"lvq_sparse_conv: channels ({self.in_channels} -> {self.out_channels}) outside the kernel family "
                             "(C_in in 4, 5, 16, 32, 64, 128 with C_out in 16, 32, 64, 128; or 128 -> 256, 256 -> 256)")
        w = self.weight.detach().float().contiguous()
        hi = torch.empty((n,), dtype=torch.int16, device=w.device)
        lo = torch.empty((n,), dtype=torch.int16, device=w.device) if split else None
        F.check(L.lvq_sparse_conv_pack_weights(F.ptr(w), self.out_channels, kvol, self.in_channels, F.ptr(hi), F.ptr(lo),
                                               F.stream_ptr(w.device)), "lvq_sparse_conv_pack_weights")
        return hi, lo

    def _folded(self, bn: nn.BatchNorm1d):
        return F.derived(self._cache, ("bn", id(bn)), (bn.weight, bn.bias, bn.running_mean, bn.running_var), lambda: F.fold_batchnorm(bn), (bn.eps,))

    def _rules(self, x: SparseConvTensor):
        key = self.indice_key
        hit = x.indice_dict.get(key) if key is not None else None
        if hit is not None and (self.subm or hit["in_indices"] is x.indices):
            if hit["kernel"] != self.kernel_size or hit["subm"] != self.subm or hit["in_indices"].shape != x.indices.shape:
                raise F.LvqError(f"indice_key {key!r} is shared by layers of different geometry")
            return hit
        out_idx, nbr, n_out, out_shape = sparse_conv_rules(x.indices, x.spatial_shape, x.batch_size, self.kernel_size, self.stride,
                                                           self.padding, self.subm)
        rec = dict(in_indices=x.indices, out_indices=out_idx, nbr=nbr, n_out=n_out, out_shape=out_shape, kernel=self.kernel_size,
                   subm=self.subm)
        x.indice_dict[key if key is not None else self] = rec      # (a layer without a key keeps its table under itself: never shared)
        return rec

    def run(self, x: SparseTensor, bn: Optional[nn.BatchNorm1d] = None, relu: bool = False,
            residual: Optional[torch.Tensor] = None) -> SparseConvTensor:
        """y = [relu]((conv(x) + bias) * scale + shift [+ residual]) in one launch."""
        if AG.wanted(self, x.features, residual) or (bn is not None and bn.training):
            raise F.LvqError(f"{type(self).__name__}: the sparse convolutions are inference-only kernels (BatchNorm folded); call them "
                             "in eval() mode under torch.no_grad()")
        if not isinstance(x, SparseConvTensor):
            x = SparseConvTensor(x.features, x.indices, x.spatial_shape, x.batch_size)
        feats = x.features
        F.require_cuda(feats, x.indices, self.weight)
        if feats.dtype != torch.float32:
            feats = feats.float()
        if x.indices.dtype != torch.int32:
            x = SparseConvTensor(feats, x.indices.to(torch.int32), x.spatial_shape, x.batch_size, x.indice_dict, x.precision)
        if len(x.spatial_shape) != self.ndim or feats.shape[1] != self.in_channels:
            raise F.LvqError(f"{type(self).__name__}: expected a {self.ndim}-D tensor with {self.in_channels} channels")
        mode = x.precision or DEFAULT_MODE
        if mode not in MODES:
            raise F.LvqError(f"sparse convolutions run in {MODES}, not {mode!r}")
        hi, lo = self._packed(mode == "bf16x3")
        rec = self._rules(x)
        nbr = rec["nbr"]
        m, kvol = nbr.shape
        out = torch.empty((m, self.out_channels), dtype=torch.float32, device=feats.device)
        scale, shift = self._folded(bn) if bn is not None else (None, None)
        bias = self.bias.detach().float().contiguous() if self.bias is not None else None
        if residual is not None:
            residual = residual.contiguous()
            assert residual.shape == out.shape and residual.dtype == torch.float32
        if m:
            rc = _lib().lvq_sparse_conv(F.ptr(feats), feats.shape[0], self.in_channels, F.ptr(nbr), kvol, m,
                                        F.ptr(None), F.ptr(hi), F.ptr(lo), self.out_channels, F.ptr(bias), F.ptr(scale), F.ptr(shift),
                                        F.ptr(residual), int(relu), F.ptr(out), F.stream_ptr(feats.device))
            F.check(rc, "lvq_sparse_conv")
        return SparseConvTensor(out, rec["out_indices"], rec["out_shape"], x.batch_size, x.indice_dict, x.precision)

    def forward(self, x: SparseTensor) -> SparseConvTensor:
        return self.run(x)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, "
                f"bias={self.bias is not None}, indice_key={self.indice_key!r}")


class SubMConv3d(_SparseConv):
    ndim, subm = 3, True


class SubMConv2d(_SparseConv):
    ndim, subm = 2, True


class SparseConv3d(_SparseConv):
    ndim, subm = 3, False


class SparseConv2d(_SparseConv):
    ndim, subm = 2, False


class SparseSequential(nn.Sequential):
    """spconv.SparseSequential: sparse layers take the tensor, dense layers (BatchNorm1d, ReLU) its features.  conv -> BatchNorm1d
    [-> ReLU] runs as one launch; a BatchNorm1d or ReLU that follows no conv has no kernel here and raises."""

    def forward(self, x):
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, _SparseConv):
                bn = relu = None
                j = i + 1
                if j < len(mods) and isinstance(mods[j], nn.BatchNorm1d):
                    bn = mods[j]
                    j += 1
                if j < len(mods) and isinstance(mods[j], nn.ReLU):
                    relu = mods[j]
                    j += 1
                x = m.run(x, bn=bn, relu=relu is not None)
                i = j
            elif isinstance(m, (nn.BatchNorm1d, nn.ReLU)):
                raise F.LvqError("SparseSequential: BatchNorm1d / ReLU are fused into the convolution before them; none precedes this one")
            else:
                x = m(x)
                i += 1
        return x


def post_act_block(in_channels, out_channels, kernel_size, indice_key=None, stride=1, padding=0, conv_type="subm", norm_fn=None):
    if conv_type == "subm":
        conv = SubMConv3d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key)
    elif conv_type == "spconv":
        conv = SparseConv3d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False, indice_key=indice_key)
    else:
        raise NotImplementedError(f"conv_type {conv_type!r} (SparseInverseConv3d has no kernel here)")
    return SparseSequential(conv, norm_fn(out_channels), nn.ReLU())


class SparseBasicBlock(nn.Module):
    expansion = 1

    conv_cls = SubMConv3d

    def __init__(self, inplanes, planes, stride=1, bias=None, norm_fn=None, downsample=None, indice_key=None):
        super().__init__()
        assert norm_fn is not None
        if bias is None:
            bias = norm_fn is not None
        self.conv1 = self.conv_cls(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn1 = norm_fn(planes)
        self.relu = nn.ReLU()
        self.conv2 = self.conv_cls(planes, planes, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn2 = norm_fn(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.conv1.run(x, bn=self.bn1, relu=True)
        return self.conv2.run(out, bn=self.bn2, relu=True, residual=identity.features)


class VoxelResBackBone8xVoxelNeXt(nn.Module):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        get = model_cfg.get if model_cfg is not None and hasattr(model_cfg, "get") else (lambda k, d: d)
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        ks = get("SPCONV_KERNEL_SIZES", [3, 3, 3, 3])
        ch = get("CHANNELS", [16, 32, 64, 128, 128])
        out_channel = get("OUT_CHANNEL", 128)
        g = [int(v) for v in grid_size]
        self.sparse_shape = [g[2] + 1, g[1], g[0]]
        self.precision: Optional[str] = None          # None -> "bf16x3"

        def res(c, key):
            return SparseBasicBlock(c, c, norm_fn=norm_fn, indice_key=key)

        def down(cin, cout, k, key):
            return post_act_block(cin, cout, k, norm_fn=norm_fn, stride=2, padding=int(k // 2), indice_key=key, conv_type="spconv")

        self.conv_input = SparseSequential(SubMConv3d(input_channels, ch[0], 3, padding=1, bias=False, indice_key="subm1"), norm_fn(ch[0]),
                                           nn.ReLU())
        self.conv1 = SparseSequential(res(ch[0], "res1"), res(ch[0], "res1"))
        self.conv2 = SparseSequential(down(ch[0], ch[1], ks[0], "spconv2"), res(ch[1], "res2"), res(ch[1], "res2"))
        self.conv3 = SparseSequential(down(ch[1], ch[2], ks[1], "spconv3"), res(ch[2], "res3"), res(ch[2], "res3"))
        self.conv4 = SparseSequential(down(ch[2], ch[3], ks[2], "spconv4"), res(ch[3], "res4"), res(ch[3], "res4"))
        self.conv5 = SparseSequential(down(ch[3], ch[4], ks[3], "spconv5"), res(ch[4], "res5"), res(ch[4], "res5"))
        self.conv6 = SparseSequential(down(ch[4], ch[4], ks[3], "spconv6"), res(ch[4], "res6"), res(ch[4], "res6"))
        self.conv_out = SparseSequential(SparseConv2d(ch[3], out_channel, 3, stride=1, padding=1, bias=False, indice_key="spconv_down2"),
                                         norm_fn(out_channel), nn.ReLU())
        self.shared_conv = SparseSequential(SubMConv2d(out_channel, out_channel, 3, stride=1, padding=1, bias=True), nn.BatchNorm1d(out_channel),
                                            nn.ReLU(True))
        self.forward_ret_dict = {}
        self.num_point_features = out_channel
        self.backbone_channels = {"x_conv1": ch[0], "x_conv2": ch[1], "x_conv3": ch[2], "x_conv4": ch[3]}

    def bev_out(self, x_conv: SparseTensor) -> SparseConvTensor:
        out = bev_out(x_conv)
        return SparseConvTensor(out.features, out.indices, out.spatial_shape, out.batch_size, None, getattr(x_conv, "precision", None))

    def forward(self, batch_dict):
        if AG.wanted(self, batch_dict["voxel_features"]):
            raise F.LvqError("VoxelResBackBone8xVoxelNeXt: inference-only kernels (BatchNorm folded); call it in eval() mode under torch.no_grad()")
        feats, coords = batch_dict["voxel_features"], batch_dict["voxel_coords"]
        F.require_cuda(feats, coords)
        mode = self.precision or DEFAULT_MODE
        x = SparseConvTensor(feats.float().contiguous(), coords.to(torch.int32).contiguous(), self.sparse_shape, batch_dict["batch_size"],
                             None, mode)
        x = self.conv_input(x)
        x_conv1 = self.conv1(x)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4 = self.conv4(x_conv3)
        x_conv5 = self.conv5(x_conv4)
        x_conv6 = self.conv6(x_conv5)
        # the coarser stages on conv4's grid: indices x 2 and x 4 (b untouched), then one z-merged 2-D tensor
        i5 = x_conv5.indices * torch.tensor([1, 2, 2, 2], dtype=torch.int32, device=feats.device)
        i6 = x_conv6.indices * torch.tensor([1, 4, 4, 4], dtype=torch.int32, device=feats.device)
        x_conv5 = SparseConvTensor(x_conv5.features, i5, x_conv5.spatial_shape, x_conv5.batch_size, x_conv5.indice_dict, mode)
        x_conv6 = SparseConvTensor(x_conv6.features, i6, x_conv6.spatial_shape, x_conv6.batch_size, x_conv6.indice_dict, mode)
        x_conv4 = SparseConvTensor(torch.cat([x_conv4.features, x_conv5.features, x_conv6.features]),
                                   torch.cat([x_conv4.indices, x_conv5.indices, x_conv6.indices]), x_conv4.spatial_shape, x_conv4.batch_size,
                                   None, mode)
        out = self.bev_out(x_conv4)
        out = self.conv_out(out)
        out = self.shared_conv(out)
        batch_dict.update({"encoded_spconv_tensor": out, "encoded_spconv_tensor_stride": 8})
        batch_dict.update({"multi_scale_3d_features": {"x_conv1": x_conv1, "x_conv2": x_conv2, "x_conv3": x_conv3, "x_conv4": x_conv4}})
        batch_dict.update({"multi_scale_3d_strides": {"x_conv1": 1, "x_conv2": 2, "x_conv3": 4, "x_conv4": 8}})
        return batch_dict


def _cfg_get(model_cfg, key, default=None):
    """model_cfg.get(key, default) for the reference's EasyDict, a dict, or no config at all."""
    return model_cfg.get(key, default) if model_cfg is not None and hasattr(model_cfg, "get") else default


class _VoxelBackBone8x(nn.Module):
    """What spconv_backbone.py's two backbones share: the constructor's bookkeeping and the forward."""

    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        g = [int(v) for v in grid_size]
        self.sparse_shape = [g[2] + 1, g[1], g[0]]    # grid_size[::-1] + [1, 0, 0]
        self.precision: Optional[str] = None          # None -> "bf16x3"
        self.num_point_features = 128

    def _conv_out(self, c_in, norm_fn):
        last_pad = _cfg_get(self.model_cfg, "last_pad", 0)
        return SparseSequential(SparseConv3d(c_in, 128, (3, 1, 1), stride=(2, 1, 1), padding=last_pad, bias=False, indice_key="spconv_down2"),
                                norm_fn(128), nn.ReLU())

    def forward(self, batch_dict):
        name = type(self).__name__
        if AG.wanted(self, batch_dict["voxel_features"]):
            raise F.LvqError(f"{name}: inference-only kernels (BatchNorm folded); call it in eval() mode under torch.no_grad()")
        feats, coords = batch_dict["voxel_features"], batch_dict["voxel_coords"]
        F.require_cuda(feats, coords)
        x = SparseConvTensor(feats.float().contiguous(), coords.to(torch.int32).contiguous(), self.sparse_shape, batch_dict["batch_size"],
                             None, self.precision or DEFAULT_MODE)
        x = self.conv_input(x)
        x_conv1 = self.conv1(x)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4 = self.conv4(x_conv3)
        out = self.conv_out(x_conv4)                   # [D4, H, W] -> [(D4 - 3) // 2 + 1, H, W]: HeightCompression folds z into the channels
        batch_dict.update({"encoded_spconv_tensor": out, "encoded_spconv_tensor_stride": 8})
        batch_dict.update({"multi_scale_3d_features": {"x_conv1": x_conv1, "x_conv2": x_conv2, "x_conv3": x_conv3, "x_conv4": x_conv4}})
        batch_dict.update({"multi_scale_3d_strides": {"x_conv1": 1, "x_conv2": 2, "x_conv3": 4, "x_conv4": 8}})
        return batch_dict


class VoxelBackBone8x(_VoxelBackBone8x):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__(model_cfg, input_channels, grid_size, **kwargs)
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        block = partial(post_act_block, norm_fn=norm_fn)
        self.conv_input = SparseSequential(SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key="subm1"), norm_fn(16), nn.ReLU())
        self.conv1 = SparseSequential(block(16, 16, 3, padding=1, indice_key="subm1"))
        self.conv2 = SparseSequential(block(16, 32, 3, stride=2, padding=1, indice_key="spconv2", conv_type="spconv"),
                                      block(32, 32, 3, padding=1, indice_key="subm2"), block(32, 32, 3, padding=1, indice_key="subm2"))
        self.conv3 = SparseSequential(block(32, 64, 3, stride=2, padding=1, indice_key="spconv3", conv_type="spconv"),
                                      block(64, 64, 3, padding=1, indice_key="subm3"), block(64, 64, 3, padding=1, indice_key="subm3"))
        self.conv4 = SparseSequential(block(64, 64, 3, stride=2, padding=(0, 1, 1), indice_key="spconv4", conv_type="spconv"),
                                      block(64, 64, 3, padding=1, indice_key="subm4"), block(64, 64, 3, padding=1, indice_key="subm4"))
        self.conv_out = self._conv_out(64, norm_fn)
        self.backbone_channels = {"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 64}


class VoxelResBackBone8x(_VoxelBackBone8x):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__(model_cfg, input_channels, grid_size, **kwargs)
        use_bias = _cfg_get(model_cfg, "USE_BIAS", None)
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        block = partial(post_act_block, norm_fn=norm_fn)
        res = partial(SparseBasicBlock, bias=use_bias, norm_fn=norm_fn)
        self.conv_input = SparseSequential(SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key="subm1"), norm_fn(16), nn.ReLU())
        self.conv1 = SparseSequential(res(16, 16, indice_key="res1"), res(16, 16, indice_key="res1"))
        self.conv2 = SparseSequential(block(16, 32, 3, stride=2, padding=1, indice_key="spconv2", conv_type="spconv"),
                                      res(32, 32, indice_key="res2"), res(32, 32, indice_key="res2"))
        self.conv3 = SparseSequential(block(32, 64, 3, stride=2, padding=1, indice_key="spconv3", conv_type="spconv"),
                                      res(64, 64, indice_key="res3"), res(64, 64, indice_key="res3"))
        self.conv4 = SparseSequential(block(64, 128, 3, stride=2, padding=(0, 1, 1), indice_key="spconv4", conv_type="spconv"),
                                      res(128, 128, indice_key="res4"), res(128, 128, indice_key="res4"))
        self.conv_out = self._conv_out(128, norm_fn)
        self.backbone_channels = {"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 128}


backbones_3d_all = {"VoxelResBackBone8xVoxelNeXt": VoxelResBackBone8xVoxelNeXt, "VoxelBackBone8x": VoxelBackBone8x,
                    "VoxelResBackBone8x": VoxelResBackBone8x}

# the pillar backbones (spconv_backbone_2d.py) live in backbone_pillar.py, which builds on this module: their entries are added from that side
from . import backbone_pillar as _backbone_pillar  # noqa: E402,F401
