"""tools/ref_standins.py -- stand-ins for the two libraries the reference's sparse backbones and dynamic VFEs import and this project
does not have: the small surface of `spconv.pytorch` that pcdet/models/backbones_3d/spconv_backbone*.py touch, and `torch_scatter`'s
`scatter_mean` / `scatter_max`.  Written from spconv's and torch_scatter's documented behaviour; used ONLY by
tools/make_lidar_encoder_goldens.py and tools/make_voxelnext_head_golden.py (the sparse SeparateHead of VoxelNeXtHead: SubMConv2d,
SparseSequential), which run the reference's unmodified classes on them and store what they return.  A layer's initialisation draws
from the RNG as spconv 2.x's reset_parameters does (weight, then bias), so the generator state behind a constructor is spconv's.  Never
imported by the package, by tests/ or by a conftest.

What the stand-in pins, and what it does not.  The fixtures made through it pin the reference's WIRING: which layers a class builds, in
which order, with which kernel, stride, padding, BatchNorm eps and bias; where the residual is added; the state_dict keys; the
batch_dict keys; VoxelNeXt's in-place `indices[:, 1:] *= 2` merge; HeightCompression's view.  spconv's OWN semantics -- what a
submanifold and a regular sparse convolution compute -- are taken from spconv's documentation and written here in dense form:

  SubMConv      the output's active set is the input's; out[site] = the dense cross-correlation (padding k // 2, stride 1) at the site
  SparseConv    a site is active where a ones-kernel convolution of the occupancy mask is above zero, listed ascending in
                (b, z, y, x); out[site] = the dense cross-correlation with the layer's stride and padding
  weight        [C_out, *kernel, C_in] (spconv 2.x), bias added at the active sites only

That residual assumption stays an assumption: tests/test_sparse_conv_restatements.py and tests/test_second_pillarnet_restatements.py
restate the same two definitions layer kind by layer kind (dictionary form against dense form), and nothing on this side can check them
against spconv's binaries.

`indice_key` is accepted and ignored (it only shares rule tables).  SparseInverseConv2d / 3d exist so that every `conv_type` branch of
the reference's `post_act_block` resolves, and raise when called: the five backbones construct none.  Integer `indices` keep the dtype
they are given.
"""
from __future__ import annotations

import contextlib
import math
import sys
import types

import torch
import torch.nn as nn
import torch.nn.functional as TF


# --------------------------------------------------------------------------------------------------------------------------------
# spconv.pytorch
# --------------------------------------------------------------------------------------------------------------------------------
class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size, **kwargs):
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(v) for v in spatial_shape]
        self.batch_size = int(batch_size)

    def replace_feature(self, feature):
        """spconv 2.x: a new tensor object over the SAME indices tensor."""
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size)

    def _sites(self, idx=None):
        ix = (self.indices if idx is None else idx).long()
        return tuple(ix[:, a] for a in range(ix.shape[1]))

    def dense(self, channels_first=True):
        nd = len(self.spatial_shape)
        out = self.features.new_zeros((self.batch_size, *self.spatial_shape, self.features.shape[1]))
        out[self._sites()] = self.features
        return out.permute(0, nd + 1, *range(1, nd + 1)).contiguous() if channels_first else out


class SparseModule(nn.Module):
    pass


class SparseSequential(SparseModule):
    """Sparse modules take the tensor; every other module (BatchNorm1d, ReLU) takes its features."""

    def __init__(self, *modules):
        super().__init__()
        for i, m in enumerate(modules):
            self.add_module(str(i), m)

    def __getitem__(self, i):
        return list(self._modules.values())[i]

    def __len__(self):
        return len(self._modules)

    def forward(self, x):
        for m in self._modules.values():
            if isinstance(m, SparseModule):
                x = m(x)
            elif isinstance(x, SparseConvTensor):
                x = x.replace_feature(m(x.features)) if x.indices.shape[0] else x
            else:
                x = m(x)
        return x


def _tuple(v, nd):
    return tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v),) * nd


class SparseConvolution(SparseModule):
    def __init__(self, ndim, in_channels, out_channels, kernel_size=3, stride=1, padding=0, dilation=1, groups=1, bias=True, subm=False,
                 indice_key=None, **kwargs):
        super().__init__()
        assert _tuple(dilation, ndim) == (1,) * ndim and groups == 1, "the backbones use neither dilation nor groups"
        self.ndim, self.in_channels, self.out_channels, self.subm, self.indice_key = ndim, in_channels, out_channels, subm, indice_key
        self.kernel_size, self.stride, self.padding = _tuple(kernel_size, ndim), _tuple(stride, ndim), _tuple(padding, ndim)
        self.weight = nn.Parameter(torch.empty(out_channels, *self.kernel_size, in_channels))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:                                  # spconv 2.x's reset_parameters: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), drawn after the weight
            bound = 1.0 / math.sqrt(in_channels * math.prod(self.kernel_size))
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        nd = self.ndim
        assert len(x.spatial_shape) == nd and x.features.shape[1] == self.in_channels
        conv = TF.conv3d if nd == 3 else TF.conv2d
        w = self.weight.permute(0, nd + 1, *range(1, nd + 1))
        if self.subm:
            y = conv(x.dense(), w, None, 1, tuple(k // 2 for k in self.kernel_size))
            out_idx, shape = x.indices, x.spatial_shape
        else:
            y = conv(x.dense(), w, None, self.stride, self.padding)
            occ = x.features.new_zeros((x.batch_size, *x.spatial_shape, 1))
            occ[x._sites()] = 1
            occ = occ.permute(0, nd + 1, *range(1, nd + 1))
            hit = conv(occ, occ.new_ones((1, 1, *self.kernel_size)), None, self.stride, self.padding)[:, 0] > 0.5
            out_idx, shape = torch.nonzero(hit).to(x.indices.dtype), list(y.shape[2:])
        f = y.permute(0, *range(2, nd + 2), 1)[x._sites(out_idx)]
        if self.bias is not None:
            f = f + self.bias
        return SparseConvTensor(f, out_idx, shape, x.batch_size)


def _conv_class(name, ndim, subm):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None, **kwargs):
        SparseConvolution.__init__(self, ndim, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, subm, indice_key)

    return type(name, (SparseConvolution,), {"__init__": __init__})


def _inverse_class(name):
    def __init__(self, *args, **kwargs):
        SparseModule.__init__(self)

    def forward(self, x):
        raise NotImplementedError(f"{name}: the stand-in has no inverse convolution (none of the five backbones builds one)")

    return type(name, (SparseModule,), {"__init__": __init__, "forward": forward})


def install_spconv():
    """Register `spconv`, `spconv.pytorch` and `spconv.pytorch.conv` in sys.modules; returns spconv.pytorch."""
    sp = types.ModuleType("spconv")
    sp.__path__ = []
    sp.__version__ = "2.3.6"
    sp.constants = types.SimpleNamespace(SPCONV_USE_DIRECT_TABLE=True)
    pt = types.ModuleType("spconv.pytorch")
    pt.__path__ = []
    cv = types.ModuleType("spconv.pytorch.conv")
    cv.SparseConvolution = SparseConvolution
    pt.SparseConvTensor, pt.SparseModule, pt.SparseSequential, pt.conv = SparseConvTensor, SparseModule, SparseSequential, cv
    for nd in (2, 3):
        for prefix, subm in (("SubMConv", True), ("SparseConv", False)):
            setattr(pt, f"{prefix}{nd}d", _conv_class(f"{prefix}{nd}d", nd, subm))
        setattr(pt, f"SparseInverseConv{nd}d", _inverse_class(f"SparseInverseConv{nd}d"))
    sp.pytorch = pt
    sys.modules["spconv"], sys.modules["spconv.pytorch"], sys.modules["spconv.pytorch.conv"] = sp, pt, cv
    return pt


# --------------------------------------------------------------------------------------------------------------------------------
# torch_scatter
# --------------------------------------------------------------------------------------------------------------------------------
def scatter_mean(src, index, dim=0, out=None, dim_size=None):
    """Segment sums over dim 0 divided by the segment's count (an empty segment divides by 1)."""
    assert dim == 0 and out is None
    m = int(index.max()) + 1 if dim_size is None else dim_size
    index = index.long()
    total = src.new_zeros((m, *src.shape[1:])).index_add_(0, index, src)
    count = torch.bincount(index, minlength=m).clamp(min=1).to(src.dtype)
    return total / count.view(-1, *[1] * (src.dim() - 1))


def scatter_max(src, index, dim=0, out=None, dim_size=None):
    """(segment maxima over dim 0, None): the callers take [0]; argmax is not provided."""
    assert dim == 0 and out is None and src.dim() == 2
    m = int(index.max()) + 1 if dim_size is None else dim_size
    top = src.new_full((m, src.shape[1]), float("-inf"))
    return top.scatter_reduce(0, index.long().view(-1, 1).expand(-1, src.shape[1]), src, reduce="amax", include_self=True), None


def install_torch_scatter():
    ts = types.ModuleType("torch_scatter")
    ts.scatter_mean, ts.scatter_max = scatter_mean, scatter_max
    sys.modules["torch_scatter"] = ts
    return ts


# --------------------------------------------------------------------------------------------------------------------------------
# .cuda() on a machine without a GPU
# --------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def cuda_is_identity():
    """The dynamic VFEs' constructors call `.cuda()` on three small tensors.  Inside this context torch.Tensor.cuda returns the tensor
    itself; the attribute is put back on the way out.  For the generator process only."""
    real = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *args, **kwargs: self
    try:
        yield
    finally:
        torch.Tensor.cuda = real
