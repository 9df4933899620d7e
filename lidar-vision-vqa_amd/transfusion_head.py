"""TransFusionHead: `spatial_features_2d` -> heat-map proposals -> one transformer decoder layer over the BEV key stream -> 3-D boxes, with the
reference's module API (pcdet/models/dense_heads/transfusion_head.py, model_utils/transfusion_utils.py, basic_block_2d.py), on lvq_conv2d,
lvq_gemm_bf16, lvq_attention_bf16, lvq_layernorm and the kernels of csrc/transfusion_head.hip.  Inference only.

  BasicBlock2D, SeparateHead_Transfusion, PositionEmbeddingLearned, TransformerDecoderLayer      the reference's containers, in its order
  TransFusionHead(model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size, predict_boxes_when_training)
  dense_heads_all                                                                                 anchor_head's registry plus TransFusionHead

state_dict() has the reference's keys and shapes (96 with USE_BIAS_BEFORE_NORM False; a checkpoint's `dense_head.*` keys load with
strict=True) and the constructor consumes the RNG as the reference does (xavier_uniform_ on the decoder's matrices, BN momentum).  `bev_pos`
is a plain attribute.  The loss objects and the Hungarian assigner are parameter-free placeholders; loss / get_targets / get_targets_single /
encode_bbox raise LvqError.

forward(batch_dict), eval() under torch.no_grad():
  convs      lvq_conv2d_to_planes, then shared_conv (3 x 3, bias as the shift) -> planes [B, H, W, 128] (hi + lo), which are ALSO the row-major
             A operand [B HW, 128] of the K | V GEMM; heatmap_head = lvq_conv2d (BN folded, ReLU) + the last conv padded to 64 channels with
             exact zeros, fp32 NCHW.  forward_ret_dict['dense_heatmap'] is a view of its first n_cls channels.
  proposals  ONE lvq_heatmap_proposals: sigmoid, 3 x 3 local maxima (point classes keep every cell), the P largest, EQUAL HEATS TOWARDS THE
             LOWER FLAT INDEX (the reference's argsort leaves ties open), query_heatmap_score.
  queries    ONE lvq_transfusion_queries: feature rows + class column, labels, positions (the reference's own formula, see below), query_pe.
  keys       key_pe = cross_posembed(bev_pos) depends on the weights and (H, W) only, and it enters the layer through the K | V projection
             alone, so per weights version and (H, W) ONE lvq_pos_embed_learned writes rowtab [HW, 256] = key_pe [Wk; Wv]^T + [bk; bv] (the
             projection folded into the embedding's last conv).  K | V = lidar_feat [Wk; Wv]^T + rowtab[row % HW] is ONE lvq_gemm_bf16 over
             B HW rows; (feat + pos) is never formed.
  decoder    self-attention (q = k = v = query + query_pe: the value carries the embedding too), cross-attention (nq = P, nkv = HW), scale
             1 / sqrt(dh); in_proj / out_proj on lvq_gemm_bf16 with the residual operand, norm1 / norm2 on lvq_layernorm,
             lvq_transfusion_add_pe for "x + query_pe as the next A operand".
  tail       ONE lvq_transfusion_tail (two launches): FFN + norm3, the prediction branches, get_bboxes + decode_bbox(filter=True), in fp32.
  writes     batch_dict['final_box_dicts']: per scene pred_boxes [n, 9 | 7] (center(2), height, dim(3), rot, vel(2)), pred_scores [n],
             pred_labels [n] int32 1-based (the reference's `.int() + 1`), IN PROPOSAL ORDER, compacted by the mask; exactly one device-to-host
             copy, of the [B] counts.  self.query_labels [B, P] int64; forward_ret_dict: center, height, dim, rot, (vel), heatmap [B, c, P]
             (views of the tail's buffer; center carries + query_pos), query_heatmap_score [B, n_cls, P], dense_heatmap [B, n_cls, H, W],
             and ours: top_proposals [B, P] int32, the flat indices class * HW + cell.

Positions.  create_2D_grid is an `ij` meshgrid over (x_size, y_size) flattened, and predict() indexes it with the row-major cell n of the
[H, W] map and flips: position(n) = (n % y_size + 0.5, n // y_size + 0.5).  On a square grid that is (column + 0.5, row + 0.5); on any other it
is not (the two axes are mixed), and it is reproduced as it is.  y_size is the map's own H (= grid_size[1] // FEATURE_MAP_STRIDE wherever the
reference runs at all), so a second (H, W) through the same module is served with its own tables.

Labels.  The reference takes the label as the argmax over classes of sigmoid(heatmap) * query_heatmap_score * one_hot(query class); for a score
of exactly 0 that argmax is arbitrary.  Here the label is always the query's class; such rows cannot pass `score > SCORE_THRESH >= 0`.

LVQ_HEAD_TORCH_POST=1 runs predict()'s selection and get_bboxes / decode_bbox as the reference's own sequence of torch ops on the device,
around the same convs and decoder kernels: the cross-check and the timing yardstick, not a fallback (it needs the same library).

Supported: HIDDEN_CHANNEL 128; NUM_HEADS in 1, 2, 4, 8; FFN_CHANNEL a multiple of 64 up to 512; ACTIVATION relu; num_conv = 2 in every branch
(NUM_HM_CONV = 2); branches center, height, dim, rot and an optional vel; NUM_PROPOSALS <= 1024; NMS_KERNEL_SIZE 3; input channels <= 512;
<= 64 classes (nuScenes mode >= 10, Waymo mode >= 3: the reference indexes them); use_sigmoid True.  Anything else raises LvqError naming the
limit, before any launch.  `precision`: "bf16x3" (default) or "bf16", as on the other heads; the tail's bits do not depend on it.

Shared with the other heads: the forward preamble and the plan cache (head_common.guard, cached_plan), the fused convs (dense_head._Fused),
and in the kernels the geometry, the range-and-threshold mask and the compaction of csrc/head_common.h.
"""
from __future__ import annotations

import copy
import math
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as TF

from . import _ffi as F
from . import anchor_head as AH
from . import autograd_route as AG
from . import ops
from .backbone2d import _Layer, to_planes
from .dense_head import _Fused
from .head_common import _get, cached_plan, guard

HIDDEN = 128
HEAD_C = 64
MAX_P = 1024
BOX_BRANCHES = {"center": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2}
POINT_CLASSES = {"nuScenes": (8, 9), "Waymo": (1, 2)}


class BasicBlock2D(nn.Module):
    """basic_block_2d.py:4-34: Conv2d, BatchNorm2d, ReLU as a parameter container."""

    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.conv = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, features):
        raise F.LvqError("BasicBlock2D: runs as one lvq_conv2d inside TransFusionHead.forward (there is no torch route)")


class SeparateHead_Transfusion(nn.Module):
    """transfusion_head.py:15-49: per branch (num_conv - 1) x [Conv1d, BatchNorm1d, ReLU] + Conv1d with bias.  (The reference's kaiming
    loop looks for nn.Conv2d among Conv1d layers and so draws nothing from the RNG; only the heatmap bias is set.)"""

    def __init__(self, input_channels, head_channels, kernel_size, sep_head_dict, init_bias=-2.19, use_bias=False):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        for cur_name in self.sep_head_dict:
            output_channels = self.sep_head_dict[cur_name]["out_channels"]
            num_conv = self.sep_head_dict[cur_name]["num_conv"]
            fc_list = []
            for _ in range(num_conv - 1):
                fc_list.append(nn.Sequential(
                    nn.Conv1d(input_channels, head_channels, kernel_size, stride=1, padding=kernel_size // 2, bias=use_bias),
                    nn.BatchNorm1d(head_channels),
                    nn.ReLU()))
            fc_list.append(nn.Conv1d(head_channels, output_channels, kernel_size, stride=1, padding=kernel_size // 2, bias=True))
            fc = nn.Sequential(*fc_list)
            if "hm" in cur_name:
                fc[-1].bias.data.fill_(init_bias)
            self.__setattr__(cur_name, fc)

    def forward(self, x):
        raise F.LvqError("SeparateHead_Transfusion: the branches run inside lvq_transfusion_tail (there is no torch route)")


class PositionEmbeddingLearned(nn.Module):
    """transfusion_utils.py:10-26.  forward(xyz [n, 2] or [B, n, 2]) -> [.., n, d] through lvq_pos_embed_learned (channels last: the kernels'
    layout, not the reference's [B, d, n])."""

    def __init__(self, input_channel, num_pos_feats=288):
        super().__init__()
        self.position_embedding_head = nn.Sequential(
            nn.Conv1d(input_channel, num_pos_feats, kernel_size=1),
            nn.BatchNorm1d(num_pos_feats),
            nn.ReLU(inplace=True),
            nn.Conv1d(num_pos_feats, num_pos_feats, kernel_size=1))

    def operands(self):
        """(w1 [d, 2], scale, shift, w2 [d, d], b2) of lvq_pos_embed_learned, per weights version."""
        c1, bn, _, c2 = self.position_embedding_head

        def build():
            scale, shift = F.fold_batchnorm(bn)
            shift = (c1.bias.detach().float() * scale + shift).contiguous()
            return (c1.weight.detach().float()[:, :, 0].contiguous(), scale, shift, c2.weight.detach().float()[:, :, 0].contiguous(),
                    c2.bias.detach().float().contiguous())
        return F.derived(self.__dict__.setdefault("_cache", {}), "pe", (c1.weight, c1.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                                                       c2.weight, c2.bias), build, (bn.eps,))

    def forward(self, xyz):
        if AG.wanted(self, xyz):
            raise F.LvqError("PositionEmbeddingLearned: inference-only kernel (BatchNorm folded); eval() under torch.no_grad()")
        if xyz.shape[-1] != 2:
            raise F.LvqError(f"PositionEmbeddingLearned: lvq_pos_embed_learned takes 2-D positions, got {tuple(xyz.shape)}")
        out = ops.pos_embed_learned(xyz.reshape(-1, 2).float().contiguous(), *self.operands())
        return out.view(*xyz.shape[:-1], out.shape[-1])


class TransformerDecoderLayer(nn.Module):
    """transfusion_utils.py:29-101 as a parameter container (the reference's registration order)."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", self_posembed=None, cross_posembed=None,
                 cross_only=False):
        super().__init__()
        self.cross_only = cross_only
        if not self.cross_only:
            self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.dropout3 = nn.Dropout(dropout)
        if activation not in ("relu", "gelu", "glu"):
            raise RuntimeError(f"activation should be relu/gelu, not {activation}.")
        self.activation = activation
        self.self_posembed = self_posembed
        self.cross_posembed = cross_posembed

    def forward(self, *args, **kwargs):
        raise F.LvqError("TransformerDecoderLayer: runs fused inside TransFusionHead.forward (there is no torch route)")


def grid_positions(h: int, w: int, device=None) -> torch.Tensor:
    """Position of every row-major cell n of an [h, w] map as predict() sees it after the flip: (n % h + 0.5, n // h + 0.5)."""
    n = torch.arange(h * w, device=device)
    return torch.stack(((n % h).float() + 0.5, torch.div(n, h, rounding_mode="floor").float() + 0.5), dim=-1).contiguous()


class TransFusionHead(nn.Module):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True):
        super().__init__()
        self.grid_size = grid_size
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size
        self.num_classes = num_class
        self.class_names = class_names
        self.model_cfg = model_cfg
        target_cfg = model_cfg.TARGET_ASSIGNER_CONFIG
        self.feature_map_stride = _get(target_cfg, "FEATURE_MAP_STRIDE", None)
        self.dataset_name = _get(target_cfg, "DATASET", "nuScenes")
        hidden_channel = model_cfg.HIDDEN_CHANNEL
        self.num_proposals = model_cfg.NUM_PROPOSALS
        self.bn_momentum = model_cfg.BN_MOMENTUM
        self.nms_kernel_size = model_cfg.NMS_KERNEL_SIZE
        num_heads = model_cfg.NUM_HEADS
        dropout = model_cfg.DROPOUT
        activation = model_cfg.ACTIVATION
        ffn_channel = model_cfg.FFN_CHANNEL
        bias = _get(model_cfg, "USE_BIAS_BEFORE_NORM", False)
        loss_cls = model_cfg.LOSS_CONFIG.LOSS_CLS
        self.use_sigmoid_cls = _get(loss_cls, "use_sigmoid", False)
        if not self.use_sigmoid_cls:
            raise F.LvqError("TransFusionHead: LOSS_CLS.use_sigmoid False (a background class in the heat map) is out of scope")
        self.build_losses()
        self.code_size = 10

        self.shared_conv = nn.Conv2d(in_channels=input_channels, out_channels=hidden_channel, kernel_size=3, padding=1)
        layers = [BasicBlock2D(hidden_channel, hidden_channel, kernel_size=3, padding=1, bias=bias),
                  nn.Conv2d(in_channels=hidden_channel, out_channels=num_class, kernel_size=3, padding=1)]
        self.heatmap_head = nn.Sequential(*layers)
        self.class_encoding = nn.Conv1d(num_class, hidden_channel, 1)
        self.decoder = TransformerDecoderLayer(hidden_channel, num_heads, ffn_channel, dropout, activation,
                                               self_posembed=PositionEmbeddingLearned(2, hidden_channel),
                                               cross_posembed=PositionEmbeddingLearned(2, hidden_channel))
        heads = copy.deepcopy(dict(model_cfg.SEPARATE_HEAD_CFG.HEAD_DICT))
        heads["heatmap"] = dict(out_channels=self.num_classes, num_conv=model_cfg.NUM_HM_CONV)
        self.prediction_head = SeparateHead_Transfusion(hidden_channel, HEAD_C, 1, heads, use_bias=bias)
        self.init_weights()
        self.bbox_assigner = None                      # HungarianAssigner3D: training only, no parameters
        x_size = self.grid_size[0] // self.feature_map_stride
        y_size = self.grid_size[1] // self.feature_map_stride
        self.bev_pos = self.create_2D_grid(int(x_size), int(y_size))
        self.forward_ret_dict = {}
        self.predict_boxes_when_training = predict_boxes_when_training
        self.precision: Optional[str] = None           # None -> "bf16x3"

    def build_losses(self):
        """The reference holds a sigmoid focal, an L1 and a Gaussian focal loss here; they have no parameters, and there is no training route."""
        self.add_module("loss_cls", nn.Module())
        self.add_module("loss_bbox", nn.Module())
        self.add_module("loss_heatmap", nn.Module())

    def create_2D_grid(self, x_size, y_size):
        meshgrid = [[0, x_size - 1, x_size], [0, y_size - 1, y_size]]
        batch_x, batch_y = torch.meshgrid(*[torch.linspace(it[0], it[1], it[2]) for it in meshgrid], indexing="ij")
        batch_x = batch_x + 0.5
        batch_y = batch_y + 0.5
        coord_base = torch.cat([batch_x[None], batch_y[None]], dim=0)[None]
        return coord_base.view(1, 2, -1).permute(0, 2, 1)

    def init_weights(self):
        for m in self.decoder.parameters():
            if m.dim() > 1:
                nn.init.xavier_uniform_(m)
        for m in self.modules():
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                m.momentum = self.bn_momentum

    def loss(self, *args, **kwargs):
        raise F.LvqError("TransFusionHead.loss: the losses are out of scope (inference-only kernels)")

    def get_targets(self, *args, **kwargs):
        raise F.LvqError("TransFusionHead.get_targets: training targets are out of scope (inference-only kernels)")

    def get_targets_single(self, *args, **kwargs):
        raise F.LvqError("TransFusionHead.get_targets_single: the Hungarian assigner is out of scope (inference-only kernels)")

    def encode_bbox(self, *args, **kwargs):
        raise F.LvqError("TransFusionHead.encode_bbox: training targets are out of scope (inference-only kernels)")

    # ------------------------------------------------------------------------------------------------------------------------------
    def _plan(self):
        return cached_plan(self, self._build_plan)

    def _build_plan(self):
        cfg, dec = self.model_cfg, self.decoder
        n_cls = int(self.num_classes)
        if int(cfg.HIDDEN_CHANNEL) != HIDDEN:
            raise F.LvqError(f"TransFusionHead: HIDDEN_CHANNEL = {cfg.HIDDEN_CHANNEL}; the query kernels are laid out for {HIDDEN}")
        if int(cfg.NUM_HEADS) not in (1, 2, 4, 8):
            raise F.LvqError(f"TransFusionHead: NUM_HEADS = {cfg.NUM_HEADS}; lvq_attention_bf16's fused kernel takes head_dim % 16 == 0: 1, 2, 4 or 8 heads")
        ffn = int(cfg.FFN_CHANNEL)
        if ffn % 64 or not 0 < ffn <= 512:
            raise F.LvqError(f"TransFusionHead: FFN_CHANNEL = {ffn}; lvq_transfusion_tail takes a multiple of 64 up to 512")
        if cfg.ACTIVATION != "relu":
            raise F.LvqError(f"TransFusionHead: ACTIVATION {cfg.ACTIVATION!r} has no kernel (relu only; gelu and glu are out of scope)")
        if dec.cross_only:
            raise F.LvqError("TransFusionHead: cross_only decoder layers are out of scope")
        p = int(self.num_proposals)
        if not 0 < p <= MAX_P:
            raise F.LvqError(f"TransFusionHead: NUM_PROPOSALS = {p}; lvq_heatmap_proposals sorts at most {MAX_P}")
        if int(self.nms_kernel_size) != 3:
            raise F.LvqError(f"TransFusionHead: NMS_KERNEL_SIZE = {self.nms_kernel_size}; lvq_heatmap_proposals tests 3 x 3 neighbourhoods only")
        if self.shared_conv.in_channels > 512:
            raise F.LvqError(f"TransFusionHead: {self.shared_conv.in_channels} input channels; lvq_conv2d takes at most 512")
        if n_cls > 64:
            raise F.LvqError(f"TransFusionHead: {n_cls} classes; the heat map's last conv and the point-class mask take at most 64")
        point = POINT_CLASSES.get(self.dataset_name, ())
        if point and n_cls <= max(point):
            raise F.LvqError(f"TransFusionHead: DATASET {self.dataset_name!r} indexes heat-map classes {point}, there are {n_cls}")
        names = list(self.prediction_head.sep_head_dict)
        box = [n for n in names if n != "heatmap"]
        vel = "vel" in box
        if box != ["center", "height", "dim", "rot"] + (["vel"] if vel else []):
            raise F.LvqError(f"TransFusionHead: branches {box}; lvq_transfusion_tail reads center, height, dim, rot and an optional vel, in this order")
        for n in names:
            d = self.prediction_head.sep_head_dict[n]
            if int(d["num_conv"]) != 2:
                raise F.LvqError(f"TransFusionHead: branch {n!r} has num_conv = {d['num_conv']}; lvq_transfusion_tail runs two convs per branch "
                                 "(NUM_HM_CONV included)")
            if n != "heatmap" and int(d["out_channels"]) != BOX_BRANCHES[n]:
                raise F.LvqError(f"TransFusionHead: branch {n!r} has {d['out_channels']} channels, the decode reads {BOX_BRANCHES[n]}")
        post = cfg.POST_PROCESSING
        thresh = float(post.SCORE_THRESH)
        limit = [float(v) for v in post.POST_CENTER_RANGE]

        shared = self.shared_conv
        block, last = self.heatmap_head[0], self.heatmap_head[1]

        def last_w():
            w = last.weight.new_zeros((64, HIDDEN, 3, 3), dtype=torch.float32)
            w[:n_cls] = last.weight.detach().float()
            return w

        def last_affine():
            shift = last.weight.new_zeros((64,), dtype=torch.float32)
            shift[:n_cls] = last.bias.detach().float()
            return torch.ones_like(shift), shift

        return dict(
            shared=_Fused([shared], shared.in_channels, HIDDEN, False, lambda: shared.weight.detach().float(),
                          lambda: (torch.ones_like(shared.bias, dtype=torch.float32), shared.bias.detach().float().contiguous()),
                          [shared.weight, shared.bias]),
            hm0=_Layer(block.conv, block.bn, True),
            hm1=_Fused([last], HIDDEN, 64, False, last_w, last_affine, [last.weight, last.bias]),
            n_cls=n_cls, p=p, vel=vel, ffn=ffn, heads=int(cfg.NUM_HEADS), thresh=thresh, limit=limit,
            mask=sum(1 << c for c in point), branches=names, cache={})

    def _bf_weight(self, plan, key, tensor, split):
        """A Linear weight as the bf16 (hi, lo) W operand of lvq_gemm_bf16, per weights version."""
        return F.derived(plan["cache"], (key, split), (tensor,), lambda: ops.cast(tensor.detach().float().contiguous(), split))

    def _rowtab(self, plan, h, w):
        """[HW, 256] fp32 = cross_posembed(positions) [Wk; Wv]^T + [bk; bv]: the projection folded into the embedding's last conv, then ONE
        lvq_pos_embed_learned over the grid.  Per weights version and (H, W)."""
        pe, ca = self.decoder.cross_posembed, self.decoder.multihead_attn
        c1, bn, _, c2 = pe.position_embedding_head
        deps = (c1.weight, c1.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, c2.weight, c2.bias, ca.in_proj_weight, ca.in_proj_bias)

        def build():
            w1, scale, shift, w2, b2 = pe.operands()
            wkv, bkv = ca.in_proj_weight.detach()[HIDDEN:].double(), ca.in_proj_bias.detach()[HIDDEN:].double()
            w2f = (wkv @ w2.double()).float().contiguous()                    # [256, 128]
            b2f = (wkv @ b2.double() + bkv).float().contiguous()
            return ops.pos_embed_learned(grid_positions(h, w, w1.device), w1, scale, shift, w2f, b2f, tag="tf_rowtab")
        return F.derived(plan["cache"], ("rowtab", h, w), deps, build, (bn.eps,))

    def key_pe(self, h, w):
        """cross_posembed over the grid, [HW, 128] fp32 (tests and tools; forward uses the folded table)."""
        plan = self._plan()
        pe = self.decoder.cross_posembed
        c1, bn, _, c2 = pe.position_embedding_head
        return F.derived(plan["cache"], ("key_pe", h, w), (c1.weight, c1.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, c2.weight, c2.bias),
                         lambda: pe(grid_positions(h, w, c1.weight.device)), (bn.eps,))

    def _tail_operands(self, plan):
        dec, ph = self.decoder, self.prediction_head
        seqs = [getattr(ph, n) for n in plan["branches"]]
        convs, bns, lasts = [s[0][0] for s in seqs], [s[0][1] for s in seqs], [s[1] for s in seqs]
        deps = [dec.linear1.weight, dec.linear1.bias, dec.linear2.weight, dec.linear2.bias, dec.norm3.weight, dec.norm3.bias] + \
               [t for m in convs for t in (m.weight, m.bias)] + [t for bn in bns for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)] + \
               [t for m in lasts for t in (m.weight, m.bias)]

        def f32(t):
            return t.detach().float().contiguous()

        def build():
            parts = [F.fold_batchnorm(bn) for bn in bns]
            scale = torch.cat([p[0] for p in parts]).contiguous()
            shift = torch.cat([p[1] if m.bias is None else m.bias.detach().float() * p[0] + p[1] for p, m in zip(parts, convs)]).contiguous()
            return dict(ffn=(f32(dec.linear1.weight), f32(dec.linear1.bias), f32(dec.linear2.weight), f32(dec.linear2.bias)),
                        norm=(f32(dec.norm3.weight), f32(dec.norm3.bias)),
                        heads=(torch.cat([f32(m.weight)[:, :, 0] for m in convs]).contiguous(), scale, shift,
                               torch.cat([f32(m.weight)[:, :, 0] for m in lasts]).contiguous(), torch.cat([f32(m.bias) for m in lasts]).contiguous()))
        return F.derived(plan["cache"], "tail", deps, build, tuple(bn.eps for bn in bns))

    def _class_operands(self, plan):
        ce = self.class_encoding
        return F.derived(plan["cache"], "class", (ce.weight, ce.bias),
                         lambda: (ce.weight.detach().float()[:, :, 0].contiguous(), ce.bias.detach().float().contiguous()))

    def tail_args(self, plan=None):
        """What lvq_transfusion_tail takes besides the rows (also used by tests and tools)."""
        plan = plan or self._plan()
        return dict(n_cls=plan["n_cls"], has_vel=plan["vel"], eps=float(self.decoder.norm3.eps), stride=int(self.feature_map_stride),
                    voxel_xy=[float(self.voxel_size[0]), float(self.voxel_size[1])],
                    range_xy=[float(self.point_cloud_range[0]), float(self.point_cloud_range[1])], limit_range=plan["limit"],
                    score_thresh=plan["thresh"], **self._tail_operands(plan))

    # ------------------------------------------------------------------------------------------------------------------------------
    def _dense(self, x, plan, split):
        """The conv stack: -> (shared planes [B, H, W, 128], maps [B, 64, H, W] fp32 with the heat-map logits in channels 0 .. n_cls - 1)."""
        b, _, h, w = x.shape
        with ops.region("tf_convs", x.device):
            lidar = plan["shared"].run(to_planes(x, split), split)
            mid = plan["hm0"].run(lidar, split)
            maps = torch.empty((b, 64, h, w), dtype=torch.float32, device=x.device)
            plan["hm1"].run(mid, split, f32=maps)
        return lidar, maps

    def _decoder(self, plan, lidar, qfeat, qpe, split):
        """self-attention, cross-attention over the B HW keys, the two post-norms -> [B P, 128] fp32 (the input of the tail)."""
        dec = self.decoder
        sa, ca = dec.self_attn, dec.multihead_attn
        b, hw = lidar.batch, lidar.h * lidar.w
        p, nh = plan["p"], plan["heads"]
        dh = HIDDEN // nh
        scale = 1.0 / math.sqrt(dh)
        rows = b * p
        qf, pe = qfeat.view(rows, HIDDEN), qpe.view(rows, HIDDEN)

        def col(t, c0):
            return t[0][:, c0:c0 + HIDDEN], None if t[1] is None else t[1][:, c0:c0 + HIDDEN]

        a = ops.transfusion_add_pe(qf, pe, split)
        _, qkv = ops.linear(a, self._bf_weight(plan, "sa_in", sa.in_proj_weight, split), sa.in_proj_bias, out_bf=True, tag="tf_sa_in")
        st = (p * 3 * HIDDEN, 3 * HIDDEN, dh)
        o = ops.attention(col(qkv, 0), col(qkv, HIDDEN), col(qkv, 2 * HIDDEN), batch=b, n_heads=nh, n_kv_heads=nh, nq=p, nkv=p, dh=dh,
                          q_strides=st, k_strides=st, v_strides=st, scale=scale, tag="tf_self_attn")
        x1, _ = ops.linear(o, self._bf_weight(plan, "sa_out", sa.out_proj.weight, split), sa.out_proj.bias, residual=qf, out_f32=True,
                           tag="tf_sa_out")
        q1, _ = ops.layernorm(x1, dec.norm1.weight, dec.norm1.bias, dec.norm1.eps, split, want_f32=True, want_bf=False)
        a2 = ops.transfusion_add_pe(q1, pe, split)
        w_ca = self._bf_weight(plan, "ca_in", ca.in_proj_weight, split)
        _, q = ops.linear(a2, w_ca, ca.in_proj_bias, w_rows=(0, HIDDEN), out_bf=True, tag="tf_ca_q")
        feat = (lidar.hi.view(torch.bfloat16).view(b * hw, HIDDEN), None if lidar.lo is None else lidar.lo.view(torch.bfloat16).view(b * hw, HIDDEN))
        _, kv = ops.linear(feat, w_ca, None, w_rows=(HIDDEN, 3 * HIDDEN), rowtab=self._rowtab(plan, lidar.h, lidar.w), out_bf=True, tag="tf_kv")
        kst = (hw * 2 * HIDDEN, 2 * HIDDEN, dh)
        o2 = ops.attention(q, col(kv, 0), col(kv, HIDDEN), batch=b, n_heads=nh, n_kv_heads=nh, nq=p, nkv=hw, dh=dh,
                           q_strides=(p * HIDDEN, HIDDEN, dh), k_strides=kst, v_strides=kst, scale=scale, tag="tf_cross_attn")
        x2, _ = ops.linear(o2, self._bf_weight(plan, "ca_out", ca.out_proj.weight, split), ca.out_proj.bias, residual=q1, out_f32=True,
                           tag="tf_ca_out")
        q2, _ = ops.layernorm(x2, dec.norm2.weight, dec.norm2.bias, dec.norm2.eps, split, want_f32=True, want_bf=False)
        return q2

    def forward(self, batch_dict):
        x = batch_dict["spatial_features_2d"]
        split = guard(self, "BatchNorm folded, no assigner, no losses", x)
        plan = self._plan()                            # refusals come before any launch
        b, _, h, w = x.shape
        if h < 3 or w < 3 or plan["p"] > plan["n_cls"] * h * w:
            raise F.LvqError(f"TransFusionHead: a {h} x {w} map with {plan['n_cls']} classes cannot give {plan['p']} proposals of 3 x 3 maxima")
        n_cls, p = plan["n_cls"], plan["p"]
        lidar, maps = self._dense(x.float().contiguous(), plan, split)
        ret = self.forward_ret_dict
        ret["dense_heatmap"] = maps[:, :n_cls]
        torch_post = bool(os.environ.get("LVQ_HEAD_TORCH_POST"))
        if torch_post:
            flat, pscore, qhs = self._torch_proposals(maps[:, :n_cls], plan)
        else:
            flat, pscore, qhs = ops.heatmap_proposals(maps, first_channel=0, n_cls=n_cls, point_class_mask=plan["mask"], n_proposals=p,
                                                      nms_kernel_size=int(self.nms_kernel_size), tag="tf_proposals")
        qfeat, qpos, qlab, qpe = ops.transfusion_queries(lidar.hi, lidar.lo, flat, n_cls=n_cls, y_size=h, class_w=self._class_operands(plan)[0],
                                                         class_b=self._class_operands(plan)[1], pe=self.decoder.self_posembed.operands(),
                                                         tag="tf_queries")
        self.query_labels = qlab.long()
        q2 = self._decoder(plan, lidar, qfeat, qpe, split)
        raw, boxes, scores, labels, counts = ops.transfusion_tail(q2.view(b, p, HIDDEN), qpos, qlab, pscore, tag="tf_tail", **self.tail_args(plan))
        o = 0
        for name in plan["branches"]:
            wd = n_cls if name == "heatmap" else BOX_BRANCHES[name]
            ret[name] = raw[:, o:o + wd]
            o += wd
        ret["query_heatmap_score"] = qhs
        ret["top_proposals"] = flat                    # [B, P] int32: class * HW + cell (the reference keeps only their two halves)
        if torch_post:
            batch_dict["final_box_dicts"] = self._torch_bboxes(ret, plan)
        else:
            totals = counts.cpu().tolist()             # THE device-to-host copy of a forward
            batch_dict["final_box_dicts"] = [dict(pred_boxes=boxes[s, :n], pred_scores=scores[s, :n], pred_labels=labels[s, :n])
                                             for s, n in enumerate(totals)]
        return batch_dict

    # ------------------------------------------------------------------------------------------------------------------------------
    # LVQ_HEAD_TORCH_POST=1: transfusion_head.py:161-185 and 397-479 as the reference's own torch ops
    # ------------------------------------------------------------------------------------------------------------------------------
    def _torch_proposals(self, dense_heatmap, plan):
        batch_size = dense_heatmap.shape[0]
        heatmap = dense_heatmap.detach().sigmoid()
        padding = self.nms_kernel_size // 2
        local_max = torch.zeros_like(heatmap)
        local_max_inner = TF.max_pool2d(heatmap, kernel_size=self.nms_kernel_size, stride=1, padding=0)
        local_max[:, :, padding:(-padding), padding:(-padding)] = local_max_inner
        for c in POINT_CLASSES.get(self.dataset_name, ()):
            local_max[:, c] = TF.max_pool2d(heatmap[:, c], kernel_size=1, stride=1, padding=0)
        heatmap = heatmap * (heatmap == local_max)
        heatmap = heatmap.view(batch_size, heatmap.shape[1], -1)
        flat_all = heatmap.view(batch_size, -1)
        top = flat_all.argsort(dim=-1, descending=True, stable=True)[..., :plan["p"]]       # stable: ties towards the lower flat index
        index = top % heatmap.shape[-1]
        qhs = heatmap.gather(index=index[:, None, :].expand(-1, heatmap.shape[1], -1), dim=-1)
        return top.to(torch.int32).contiguous(), flat_all.gather(1, top).contiguous(), qhs.contiguous()

    def _torch_bboxes(self, ret, plan):
        heat = ret["heatmap"].sigmoid()
        one_hot = TF.one_hot(self.query_labels, num_classes=self.num_classes).permute(0, 2, 1)
        batch_score = heat * ret["query_heatmap_score"] * one_hot
        center, height, dim, rot = ret["center"].clone(), ret["height"], ret["dim"], ret["rot"]
        vel = ret["vel"] if plan["vel"] else None
        post_center_range = torch.tensor(plan["limit"], dtype=torch.float32, device=heat.device)
        final_scores = batch_score.max(1, keepdims=False).values
        final_preds = self.query_labels                                  # the argmax wherever the score is not 0 (see the module docstring)
        center[:, 0, :] = center[:, 0, :] * self.feature_map_stride * self.voxel_size[0] + self.point_cloud_range[0]
        center[:, 1, :] = center[:, 1, :] * self.feature_map_stride * self.voxel_size[1] + self.point_cloud_range[1]
        dim = dim.exp()
        rot = torch.atan2(rot[:, 0:1, :], rot[:, 1:2, :])
        parts = [center, height, dim, rot] + ([vel] if vel is not None else [])
        final_box_preds = torch.cat(parts, dim=1).permute(0, 2, 1)
        thresh_mask = final_scores > plan["thresh"]
        mask = (final_box_preds[..., :3] >= post_center_range[:3]).all(2)
        mask &= (final_box_preds[..., :3] <= post_center_range[3:]).all(2)
        out = []
        for i in range(heat.shape[0]):
            cmask = mask[i, :] & thresh_mask[i]
            out.append(dict(pred_boxes=final_box_preds[i, cmask], pred_scores=final_scores[i, cmask],
                            pred_labels=final_preds[i, cmask].int() + 1))
        return out


dense_heads_all = dict(AH.dense_heads_all, TransFusionHead=TransFusionHead)
