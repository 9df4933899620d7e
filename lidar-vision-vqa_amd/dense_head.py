"""CenterHead: `spatial_features_2d` -> 3-D boxes, with the reference's module API (pcdet/models/dense_heads/center_head.py:12-416), on the
conv kernels of csrc/conv2d.hip and the post-processing kernels of csrc/center_head.hip.  Inference only.

  SeparateHead(input_channels, sep_head_dict, init_bias, use_bias, norm_func)   the parameter containers of one task (center_head.py:12-46)
  CenterHead(model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size, predict_boxes_when_training)
  dense_heads_all                                                               registry with the reference's NAME string

`shared_conv` and `heads_list.{i}.{name}` are the reference's nn.Sequential containers in the reference's construction order, so
state_dict() keys and shapes are the reference's (a checkpoint's `dense_head.*` keys load with strict=True) and the initialisation (hm bias
-2.19, kaiming_normal_ on the other branches) consumes the RNG as the reference does.  The constructor moves nothing to a device: the
class-id mappings are non-persistent buffers (`class_id_mapping_{i}`, also listed in `class_id_mapping_each_head`) that follow .to().

forward(data_dict), eval() under torch.no_grad():
  convs   spatial_features_2d goes once through lvq_conv2d_to_planes; the shared conv + BatchNorm + ReLU is one lvq_conv2d launch; per task
          the FIRST convs of all branches are one conv C -> n_branch * C (weights concatenated along C_out, BatchNorm folded, ReLU) and the
          LAST convs are one block-diagonal conv n_branch * C -> 64 with fp32 output and the biases as the shift: output channels of branch
          j read input channels j C .. j C + C - 1, every other weight is an exact zero.  Exact zeros add nothing under the kernel's fp32
          accumulation in ascending chunk order, so a channel carries the bits a conv of its branch alone would give.  Every task writes
          its 64 channels of ONE [B, 64 n_tasks, H, W] fp32 tensor; forward_ret_dict['pred_dicts'] are views of it.
  post    ONE lvq_center_decode (top-K, gathers, exp / atan2, masks, compaction for every scene and task), ONE lvq_nms_bev with
          G = B * n_tasks (two launches), ONE lvq_center_collect (gather + head-order concatenation + 1-based int64 labels).
  sync    exactly one device-to-host copy, the [B, n_tasks] keep counts; the per-scene tensors are slices of the collected buffers.
  writes  data_dict['final_box_dicts'] = B dicts of pred_boxes [n, 9 or 7], pred_scores [n], pred_labels [n] int64 (1-based), and, with
          predict_boxes_when_training, rois / roi_scores / roi_labels / has_class_labels through reorder_rois_for_refining (plain torch).
          (The reference writes the rois INSTEAD of final_box_dicts in that case; here both are written.)

Supported: SHARED_CONV_CHANNEL = 64; every branch (hm included: NUM_HM_CONV) with the same num_conv in {1, 2}; at most 64 output
channels per task; input channels <= 512; MAX_OBJ_PER_SAMPLE <= 1024; NMS_TYPE nms_gpu.  Anything else raises LvqError naming the limit.
`precision`: "bf16x3" (default) or "bf16", as on the backbones.  LVQ_HEAD_TORCH_POST=1 routes the post-processing through the reference's
own sequence of torch ops (two top-ks, gathers, masks per scene and task; NMS = lvq_boxes_iou_bev + a host walk): the cross-check and the
timing comparison, not a fallback (it needs the same library).

Shared with the other heads through head_common.py: guard, CenterStyleHead (class-id mappings, stubs), center_tasks, center_decode_args,
center_post_cfg, collect_kept, class_agnostic_nms_torch.  `_Fused` here is also anchor_head's and transfusion_head's fused conv.
"""
from __future__ import annotations

import copy
import os
from functools import partial
from typing import List, Optional

import torch
import torch.nn as nn
from torch.nn.init import kaiming_normal_

from . import _ffi as F
from . import ops
from .backbone2d import Planes, _Layer, to_planes
from .head_common import (BOX_BRANCHES, MAX_K, CenterStyleHead, _get, cached_plan, center_decode_args, center_post_cfg, center_tasks,  # noqa: F401
                          class_agnostic_nms_torch, collect_kept, guard)

SHARED_C = 64                  # SHARED_CONV_CHANNEL the fused convs are laid out for
TASK_C = 64                    # output channels of a task's last conv (lvq_conv2d: c_out a multiple of 64)


class SeparateHead(nn.Module):
    """center_head.py:12-46: one nn.Sequential per branch, (num_conv - 1) x [Conv2d 3 x 3, norm, ReLU] + Conv2d 3 x 3 with bias."""

    def __init__(self, input_channels, sep_head_dict, init_bias=-2.19, use_bias=False, norm_func=None):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        for cur_name in self.sep_head_dict:
            output_channels = self.sep_head_dict[cur_name]["out_channels"]
            num_conv = self.sep_head_dict[cur_name]["num_conv"]
            fc_list = []
            for _ in range(num_conv - 1):
                fc_list.append(nn.Sequential(
                    nn.Conv2d(input_channels, input_channels, kernel_size=3, stride=1, padding=1, bias=use_bias),
                    nn.BatchNorm2d(input_channels) if norm_func is None else norm_func(input_channels),
                    nn.ReLU()))
            fc_list.append(nn.Conv2d(input_channels, output_channels, kernel_size=3, stride=1, padding=1, bias=True))
            fc = nn.Sequential(*fc_list)
            if "hm" in cur_name:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d):
                        kaiming_normal_(m.weight.data)
                        if hasattr(m, "bias") and m.bias is not None:
                            nn.init.constant_(m.bias, 0)
            self.__setattr__(cur_name, fc)

    def forward(self, x):
        raise F.LvqError("SeparateHead: the branches run fused inside CenterHead.forward (there is no torch route)")


class _Fused(_Layer):
    """A 3 x 3 conv whose weight and epilogue are assembled from several containers: built by `weight()` / `affine()` from `params`,
    cached per parameter version like every packed operand (_ffi.derived)."""

    def __init__(self, convs: List[nn.Conv2d], c_in: int, c_out: int, relu: bool, weight, affine, params, extra=()):
        self.conv, self.bn, self.relu, self.transposed = convs[0], None, relu, False
        self.kernel, self.stride, self.padding = 3, 1, 1
        self.c_in, self.c_out = c_in, c_out
        self._weight, self._affine, self._params, self._extra = weight, affine, tuple(params), tuple(extra)
        self._cache = {}

    def packed(self, split: bool):
        def build():
            hi, lo = ops.conv2d_pack_weights(self._weight().contiguous(), self.c_out, self.c_in, self.kernel, False, split)
            return hi.view(torch.int16), None if lo is None else lo.view(torch.int16)
        return F.derived(self._cache, ("w", split), self._params, build)

    def folded(self):
        return F.derived(self._cache, "bn", self._params, self._affine, self._extra)


def _first_convs(seqs: List[nn.Sequential], k: int) -> _Fused:
    """Conv k of every branch as one conv C -> n_branch * C: weights along C_out, BatchNorm (and a conv bias) folded, ReLU."""
    convs, bns = [s[k][0] for s in seqs], [s[k][1] for s in seqs]
    c = convs[0].in_channels

    def weight():
        return torch.cat([m.weight.detach().float() for m in convs], dim=0)

    def affine():
        parts = [F.fold_batchnorm(bn) for bn in bns]
        scale = torch.cat([p[0] for p in parts])
        shift = torch.cat([p[1] if m.bias is None else m.bias.detach().float() * p[0] + p[1] for p, m in zip(parts, convs)])
        return scale.contiguous(), shift.contiguous()

    params = [m.weight for m in convs] + [m.bias for m in convs] + [t for bn in bns for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
    return _Fused(convs, c, c * len(convs), True, weight, affine, params, tuple(bn.eps for bn in bns))


def _last_convs(seqs: List[nn.Sequential], block_diagonal: bool) -> _Fused:
    """The last conv of every branch as one conv -> TASK_C fp32 channels, the biases as the shift.  block_diagonal: branch j reads
    input channels j C .. j C + C - 1 (the output of _first_convs) and every other weight is an exact zero; otherwise (num_conv = 1) all
    branches read the shared features."""
    convs = [s[len(s) - 1] for s in seqs]
    c, n = convs[0].in_channels, len(convs)
    c_in = c * n if block_diagonal else c

    def weight():
        w = convs[0].weight.new_zeros((TASK_C, c_in, 3, 3), dtype=torch.float32)
        row = 0
        for j, m in enumerate(convs):
            col = j * c if block_diagonal else 0
            w[row:row + m.out_channels, col:col + c] = m.weight.detach().float()
            row += m.out_channels
        return w

    def affine():
        shift = convs[0].weight.new_zeros((TASK_C,), dtype=torch.float32)
        row = 0
        for m in convs:
            shift[row:row + m.out_channels] = m.bias.detach().float()
            row += m.out_channels
        return torch.ones_like(shift), shift

    return _Fused(convs, c_in, TASK_C, False, weight, affine, [m.weight for m in convs] + [m.bias for m in convs])


class CenterHead(CenterStyleHead):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.grid_size = grid_size
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size
        self.feature_map_stride = _get(_get(model_cfg, "TARGET_ASSIGNER_CONFIG", {}), "FEATURE_MAP_STRIDE")
        self._init_class_maps(model_cfg, class_names)

        norm_func = partial(nn.BatchNorm2d, eps=_get(model_cfg, "BN_EPS", 1e-5), momentum=_get(model_cfg, "BN_MOM", 0.1))
        use_bias = _get(model_cfg, "USE_BIAS_BEFORE_NORM", False)
        self.shared_conv = nn.Sequential(
            nn.Conv2d(input_channels, model_cfg.SHARED_CONV_CHANNEL, 3, stride=1, padding=1, bias=use_bias),
            norm_func(model_cfg.SHARED_CONV_CHANNEL),
            nn.ReLU())
        self.heads_list = nn.ModuleList()
        self.separate_head_cfg = model_cfg.SEPARATE_HEAD_CFG
        for cur_class_names in self.class_names_each_head:
            cur_head_dict = copy.deepcopy(dict(self.separate_head_cfg.HEAD_DICT))
            cur_head_dict["hm"] = dict(out_channels=len(cur_class_names), num_conv=model_cfg.NUM_HM_CONV)
            self.heads_list.append(SeparateHead(input_channels=model_cfg.SHARED_CONV_CHANNEL, sep_head_dict=cur_head_dict, init_bias=-2.19,
                                                use_bias=use_bias, norm_func=norm_func))
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = {}
        self.build_losses()
        self.precision: Optional[str] = None          # None -> "bf16x3"

    # ------------------------------------------------------------------------------------------------------------------------------
    def _plan(self):
        return cached_plan(self, self._build_plan)

    def _build_plan(self):
        cfg = self.model_cfg
        if int(cfg.SHARED_CONV_CHANNEL) != SHARED_C:
            raise F.LvqError(f"CenterHead: SHARED_CONV_CHANNEL = {cfg.SHARED_CONV_CHANNEL}; the fused head convs are laid out for {SHARED_C}")
        if self.shared_conv[0].in_channels > 512:
            raise F.LvqError(f"CenterHead: {self.shared_conv[0].in_channels} input channels; lvq_conv2d takes at most 512")
        def one_num_conv(i, num_conv):
            if len(set(num_conv)) != 1 or not set(num_conv) <= {1, 2}:
                raise F.LvqError(f"CenterHead: task {i} has num_conv {sorted(num_conv)}; the fused convs take one num_conv for all "
                                 "branches (NUM_HM_CONV included), 1 or 2")

        plan = center_tasks("CenterHead", self.heads_list, self.class_names_each_head, TASK_C, self.separate_head_cfg.HEAD_ORDER, self.class_names,
                            no_kernel_note="an 'iou' branch with USE_IOU_TO_RECTIFY_SCORE is out of scope; ",
                            task_writes="one task's last conv writes", task_rule=one_num_conv)
        for head, t in zip(self.heads_list, plan["tasks"]):
            seqs = [getattr(head, n) for n in t["names"]]
            two = t["num_conv"][0] == 2
            t.update(first=_first_convs(seqs, 0) if two else None, last=_last_convs(seqs, two))
        plan["shared"] = _Layer(self.shared_conv[0], self.shared_conv[1], True)
        return plan

    def _post_cfg(self):
        return center_post_cfg("CenterHead", self.model_cfg.POST_PROCESSING, "lvq_center_decode", rectifier=True,
                               nms_note="; nms_normal_gpu, class_specific_nms and circle_nms are out of scope")

    def _maps(self, x: torch.Tensor, split: bool):
        """The conv stack: [B, C, H, W] fp32 -> maps [B, 64 n_tasks, H, W] fp32."""
        plan = self._plan()
        b, _, h, w = x.shape
        tasks = plan["tasks"]
        maps = torch.empty((b, TASK_C * len(tasks), h, w), dtype=torch.float32, device=x.device)
        shared: Planes = plan["shared"].run(to_planes(x, split), split)
        for i, t in enumerate(tasks):
            mid = t["first"].run(shared, split) if t["first"] is not None else shared
            t["last"].run(mid, split, f32=maps, c_off=TASK_C * i)
        return maps

    def _pred_dicts(self, maps):
        out = []
        for i, t in enumerate(self._plan()["tasks"]):
            out.append({n: maps[:, TASK_C * i + o:TASK_C * i + o + wd] for n, (o, wd) in t["offs"].items()})
        return out

    def forward(self, data_dict):
        x = data_dict["spatial_features_2d"]
        split = guard(self, "BatchNorm folded, no target assignment, no losses", x)
        post = self._post_cfg()                        # refusals come before any launch
        plan = self._plan()
        maps = self._maps(x.float().contiguous(), split)
        self.forward_ret_dict["pred_dicts"] = self._pred_dicts(maps)
        batch_size = int(data_dict["batch_size"])
        if batch_size != maps.shape[0]:
            raise F.LvqError(f"CenterHead: batch_size = {batch_size}, spatial_features_2d holds {maps.shape[0]} scenes")
        if os.environ.get("LVQ_HEAD_TORCH_POST"):
            pred_dicts = self._torch_post(batch_size, post)
        else:
            pred_dicts = self._kernel_post(maps, plan, post)
        data_dict["final_box_dicts"] = pred_dicts
        if self.predict_boxes_when_training:
            rois, roi_scores, roi_labels = self.reorder_rois_for_refining(batch_size, pred_dicts)
            data_dict["rois"], data_dict["roi_scores"], data_dict["roi_labels"] = rois, roi_scores, roi_labels
            data_dict["has_class_labels"] = True
        return data_dict

    def decode_args(self, plan=None):
        """What lvq_center_decode takes besides the maps (also used by tests and tools)."""
        return center_decode_args(self, plan or self._plan(), TASK_C)

    def _kernel_post(self, maps, plan, post):
        boxes, scores, labels, counts = ops.center_decode(maps, k=post["k"], limit_range=post["limit"], score_thresh=post["thresh"],
                                                          tag="center_decode", **self.decode_args(plan))
        self.forward_ret_dict["candidate_counts"] = counts                   # [B, n_tasks] int32 on the device: survivors before NMS
        b, t, k, d = boxes.shape
        keep, keep_count = ops.nms_bev(boxes.view(b * t, k, d), counts.view(-1), thresh=post["nms_thresh"], pre_max=post["pre"],
                                       post_max=post["post"], tag="center_nms")
        return collect_kept(boxes, scores, labels, keep, keep_count, "center_collect")      # holds THE device-to-host copy of a forward

    # ------------------------------------------------------------------------------------------------------------------------------
    # LVQ_HEAD_TORCH_POST=1: center_head.py:297-365 / centernet_utils.py:155-241 / model_nms_utils.py:6-25 as the reference's own torch ops
    # ------------------------------------------------------------------------------------------------------------------------------
    def _torch_post(self, batch_size, post):
        K, dev = post["k"], self.shared_conv[0].weight.device
        limit = torch.tensor(post["limit"], dtype=torch.float32, device=dev)
        stride, vs, rng = self.feature_map_stride, self.voxel_size, self.point_cloud_range
        ret = [dict(pred_boxes=[], pred_scores=[], pred_labels=[]) for _ in range(batch_size)]

        def gather(feat, ind):                                              # _transpose_and_gather_feat
            feat = feat.permute(0, 2, 3, 1).contiguous()
            feat = feat.view(feat.size(0), -1, feat.size(3))
            return feat.gather(1, ind.unsqueeze(2).expand(ind.size(0), ind.size(1), feat.size(2)))

        for idx, pd in enumerate(self.forward_ret_dict["pred_dicts"]):
            hm = pd["hm"].sigmoid()
            batch, n_cls, height, width = hm.shape
            topk_scores, topk_inds = torch.topk(hm.flatten(2, 3), K)
            topk_inds = topk_inds % (height * width)
            topk_ys = (topk_inds // width).float()
            topk_xs = (topk_inds % width).int().float()
            score, topk_ind = torch.topk(topk_scores.view(batch, -1), K)
            class_ids = (topk_ind // K).int()
            inds = topk_inds.view(batch, -1).gather(1, topk_ind)
            ys = topk_ys.view(batch, -1).gather(1, topk_ind).view(batch, K, 1)
            xs = topk_xs.view(batch, -1).gather(1, topk_ind).view(batch, K, 1)
            center, center_z = gather(pd["center"], inds), gather(pd["center_z"], inds)
            dim = gather(pd["dim"].exp(), inds)
            angle = torch.atan2(gather(pd["rot"][:, 1:2], inds), gather(pd["rot"][:, 0:1], inds))
            xs = (xs + center[:, :, 0:1]) * stride * vs[0] + rng[0]
            ys = (ys + center[:, :, 1:2]) * stride * vs[1] + rng[1]
            parts = [xs, ys, center_z, dim, angle] + ([gather(pd["vel"], inds)] if "vel" in pd else [])
            box_preds = torch.cat(parts, dim=-1)
            mask = (box_preds[..., :3] >= limit[:3]).all(2) & (box_preds[..., :3] <= limit[3:]).all(2)
            if post["thresh"] is not None:
                mask &= score > post["thresh"]
            mapping = self.class_id_mapping_each_head[idx]
            for k in range(batch_size):
                cur_boxes, cur_scores = box_preds[k, mask[k]], score[k, mask[k]]
                cur_labels = mapping[class_ids[k, mask[k]].long()]
                selected = class_agnostic_nms_torch(cur_boxes, cur_scores, post)
                ret[k]["pred_boxes"].append(cur_boxes[selected])
                ret[k]["pred_scores"].append(cur_scores[selected])
                ret[k]["pred_labels"].append(cur_labels[selected])
        for k in range(batch_size):
            ret[k]["pred_boxes"] = torch.cat(ret[k]["pred_boxes"], dim=0)
            ret[k]["pred_scores"] = torch.cat(ret[k]["pred_scores"], dim=0)
            ret[k]["pred_labels"] = torch.cat(ret[k]["pred_labels"], dim=0) + 1
        return ret


dense_heads_all = {"CenterHead": CenterHead}
