"""VoxelNeXtHead: `encoded_spconv_tensor` (the 2-D sparse tensor backbone3d.VoxelResBackBone8xVoxelNeXt writes) -> 3-D boxes, with the
reference's module API (pcdet/models/dense_heads/voxelnext_head.py:13-559), on csrc/sparse_head.hip and csrc/center_head.hip.  Inference only.

  SeparateHead(input_channels, sep_head_dict, kernel_size, init_bias, use_bias)   the sparse parameter containers of one task (:13-47)
  VoxelNeXtHead(model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size, predict_boxes_when_training)
  dense_heads_all    dense_head's registry + "VoxelNeXtHead": every head under the reference's NAME string

`heads_list.{i}.{name}` are nn.Sequential(SparseSequential(SubMConv2d, BatchNorm1d, ReLU), SubMConv2d) in the reference's construction
order, so state_dict() keys and shapes are the reference's (a checkpoint's `dense_head.*` keys load with strict=True) and the
initialisation (hm bias -2.19, kaiming_normal_ on the other branches) consumes the RNG as the reference does.  The constructor moves
nothing to a device: the class-id mappings are non-persistent buffers, as in CenterHead.

forward(data_dict), eval() under torch.no_grad():
  convs   ONE lvq_sparse_head launch runs every branch of every task over the N active rows (the 128-wide intermediates stay on chip);
          with KERNEL_SIZE_HEAD = 3 the subm 3 x 3 rule table is built once (sparse_conv_rules) and shared by all branches.  The result
          is ONE channel-major [16 n_tasks, N] fp32 buffer; forward_ret_dict['pred_dicts'] are [N, out] views of it.
  post    ONE lvq_voxel_decode (top-K over the scene's rows, gathers through the rows' own (y, x), exp / atan2, masks, compaction),
          ONE lvq_nms_bev with G = B * n_tasks, ONE lvq_center_collect, and exactly one device-to-host copy (the keep counts).
  writes  forward_ret_dict['pred_dicts' / 'voxel_indices' / 'batch_index']; data_dict['final_box_dicts'] = B dicts of pred_boxes,
          pred_scores, pred_labels (int64, 1-based) and pred_ious (a list of None per task, as the reference leaves it without an iou
          branch); with predict_boxes_when_training also rois / roi_scores / roi_labels / has_class_labels.

ONE DELIBERATE DIFFERENCE from the reference: when a scene has fewer than K = MAX_OBJ_PER_SAMPLE rows, centernet_utils._topk_1d still
computes class = ind // K on an [n_cls, n_b] matrix, which gives wrong classes, and when n_cls * n_b < K its torch.stack / .view(batch, K)
raise.  Here the class is the matrix row the candidate came from and the count is what there is.  With n_b >= K in every scene the two
agree.

Supported: SHARED_CONV_CHANNEL = 128 (= input_channels); KERNEL_SIZE_HEAD in {1, 3}; one num_conv in {1, 2} for all branches (NUM_HM_CONV
included); branches center, center_z, dim, rot[, vel] and hm; at most 16 output channels and 8 branches per task, 16 tasks;
MAX_OBJ_PER_SAMPLE <= 1024; NMS_TYPE nms_gpu.  IOU_BRANCH (the Waymo configs: class-specific NMS with a rectifier), DOUBLE_FLIP and
anything else raise LvqError naming the limit, before any launch.  `precision`: "bf16x3" or "bf16"; None follows the input tensor's
`precision` (default "bf16x3").  LVQ_HEAD_TORCH_POST=1 routes the post-processing through the reference's own sequence of torch ops
(_topk_1d with the corrected class, gather_feat_idx, masks per scene, NMS = lvq_boxes_iou_bev + a host walk): the cross-check and the
timing baseline, not a fallback.

What this head shares with CenterHead is head_common.py's: CenterStyleHead (class-id mappings, stubs, reorder_rois_for_refining),
center_tasks (the branch tables; the owner table, br_stride and the all-tasks num_conv rule are this head's own), center_decode_args,
center_post_cfg, collect_kept and class_agnostic_nms_torch; the preamble is inference_split (a sparse tensor is not [B, C, H, W]).
"""
from __future__ import annotations

import copy
import os
from typing import Optional

import torch
import torch.nn as nn
from torch.nn.init import kaiming_normal_

from . import _ffi as F
from . import dense_head as DH
from . import ops
from .backbone3d import SparseSequential, SubMConv2d, sparse_conv_rules
from .head_common import (CenterStyleHead, _get, cached_plan, center_decode_args, center_post_cfg, center_tasks, class_agnostic_nms_torch,
                          collect_kept, inference_split)

HEAD_C = 128                   # SHARED_CONV_CHANNEL lvq_sparse_head is laid out for
TASK_C = ops.HEAD_TASK_C       # output channels of a task in the head buffer
MAX_BR = 8
MAX_TASKS = 16


class SeparateHead(nn.Module):
    """voxelnext_head.py:13-47: per branch nn.Sequential((num_conv - 1) x SparseSequential(SubMConv2d k x k, BatchNorm1d, ReLU),
    SubMConv2d 1 x 1 with bias)."""

    def __init__(self, input_channels, sep_head_dict, kernel_size, init_bias=-2.19, use_bias=False):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        for cur_name in self.sep_head_dict:
            output_channels = self.sep_head_dict[cur_name]["out_channels"]
            num_conv = self.sep_head_dict[cur_name]["num_conv"]
            fc_list = []
            for _ in range(num_conv - 1):
                fc_list.append(SparseSequential(
                    SubMConv2d(input_channels, input_channels, kernel_size, padding=int(kernel_size // 2), bias=use_bias, indice_key=cur_name),
                    nn.BatchNorm1d(input_channels),
                    nn.ReLU()))
            fc_list.append(SubMConv2d(input_channels, output_channels, 1, bias=True, indice_key=cur_name + "out"))
            fc = nn.Sequential(*fc_list)
            if "hm" in cur_name:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, SubMConv2d):
                        kaiming_normal_(m.weight.data)
                        if hasattr(m, "bias") and m.bias is not None:
                            nn.init.constant_(m.bias, 0)
            self.__setattr__(cur_name, fc)

    def forward(self, x):
        raise F.LvqError("SeparateHead: the branches run fused inside VoxelNeXtHead.forward (there is no torch route)")


class VoxelNeXtHead(CenterStyleHead):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=False):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.grid_size = grid_size
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size
        self.feature_map_stride = _get(_get(model_cfg, "TARGET_ASSIGNER_CONFIG", {}), "FEATURE_MAP_STRIDE")
        self.gaussian_ratio = _get(model_cfg, "GAUSSIAN_RATIO", 1)
        self.gaussian_type = _get(model_cfg, "GAUSSIAN_TYPE", ["nearst", "gt_center"])
        self.iou_branch = _get(model_cfg, "IOU_BRANCH", False)
        self.double_flip = _get(model_cfg, "DOUBLE_FLIP", False)
        self._init_class_maps(model_cfg, class_names)

        self.kernel_size_head = int(_get(model_cfg, "KERNEL_SIZE_HEAD", 3))
        self.shared_channel = int(_get(model_cfg, "SHARED_CONV_CHANNEL", 128))
        self.heads_list = nn.ModuleList()
        self.separate_head_cfg = model_cfg.SEPARATE_HEAD_CFG
        for cur_class_names in self.class_names_each_head:
            cur_head_dict = copy.deepcopy(dict(self.separate_head_cfg.HEAD_DICT))
            cur_head_dict["hm"] = dict(out_channels=len(cur_class_names), num_conv=model_cfg.NUM_HM_CONV)
            self.heads_list.append(SeparateHead(input_channels=self.shared_channel, sep_head_dict=cur_head_dict,
                                                kernel_size=self.kernel_size_head, init_bias=-2.19,
                                                use_bias=_get(model_cfg, "USE_BIAS_BEFORE_NORM", False)))
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = {}
        self.build_losses()
        self.precision: Optional[str] = None          # None -> the input tensor's precision, else "bf16x3"
        object.__setattr__(self, "_cache", {})

    # ------------------------------------------------------------------------------------------------------------------------------
    def _plan(self):
        return cached_plan(self, self._build_plan)

    def _build_plan(self):
        if self.iou_branch:
            raise F.LvqError("VoxelNeXtHead: IOU_BRANCH (the Waymo configs: an 'iou' branch, class-specific NMS with a rectifier) has no kernel")
        if self.double_flip:
            raise F.LvqError("VoxelNeXtHead: DOUBLE_FLIP (test-time augmentation merged over four flipped copies) has no kernel")
        if self.shared_channel != HEAD_C:
            raise F.LvqError(f"VoxelNeXtHead: SHARED_CONV_CHANNEL = {self.shared_channel}; lvq_sparse_head is laid out for {HEAD_C}")
        if self.kernel_size_head not in (1, 3):
            raise F.LvqError(f"VoxelNeXtHead: KERNEL_SIZE_HEAD = {self.kernel_size_head}; lvq_sparse_head takes 1 or 3")
        if len(self.heads_list) > MAX_TASKS:
            raise F.LvqError(f"VoxelNeXtHead: {len(self.heads_list)} tasks; lvq_sparse_head takes at most {MAX_TASKS}")
        def one_num_conv(tasks):
            all_convs = {c for t in tasks for c in t["num_conv"]}
            if len(all_convs) != 1 or not all_convs <= {1, 2}:
                raise F.LvqError(f"VoxelNeXtHead: num_conv {sorted(all_convs)}; the fused convs take one num_conv for all branches of all "
                                 "tasks (NUM_HM_CONV included), 1 or 2")

        plan = center_tasks("VoxelNeXtHead", self.heads_list, self.class_names_each_head, TASK_C, self.separate_head_cfg.HEAD_ORDER,
                            self.class_names, max_branches=MAX_BR, head_rule=one_num_conv)
        for head, t in zip(self.heads_list, plan["tasks"]):
            owner = [j for j, wd in enumerate(t["widths"]) for _ in range(wd)]
            t.update(seqs=[getattr(head, n) for n in t["names"]], owner=owner + [-1] * (TASK_C - len(owner)))
        plan.update(num_conv=plan["tasks"][0]["num_conv"][0], br_stride=max(len(t["names"]) for t in plan["tasks"]))
        return plan

    def _post_cfg(self):
        return center_post_cfg("VoxelNeXtHead", self.model_cfg.POST_PROCESSING, "lvq_voxel_decode", positive_k=True)

    def _operands(self, plan, split: bool):
        """Packed first-conv weights, folded norms, last-conv weights and biases of all tasks: one entry per precision form, rebuilt when
        a parameter's version moves (_ffi.derived)."""
        two = plan["num_conv"] == 2
        firsts = [s[0] for t in plan["tasks"] for s in t["seqs"]] if two else []
        lasts = [s[len(s) - 1] for t in plan["tasks"] for s in t["seqs"]]
        params = [m.weight for m in lasts] + [m.bias for m in lasts]
        for f in firsts:
            params += [f[0].weight, f[0].bias, f[1].weight, f[1].bias, f[1].running_mean, f[1].running_var]

        def build():
            dev = lasts[0].weight.device
            n_tasks, bs = len(plan["tasks"]), plan["br_stride"]
            w_last = torch.zeros((n_tasks, TASK_C, HEAD_C), dtype=torch.float32, device=dev)
            bias = torch.zeros((n_tasks, TASK_C), dtype=torch.float32, device=dev)
            w_hi = w_lo = scale = shift = None
            if two:
                kvol = self.kernel_size_head ** 2
                per = kvol * HEAD_C * HEAD_C
                w_hi = torch.zeros((n_tasks, bs, per), dtype=torch.int16, device=dev)
                w_lo = torch.zeros_like(w_hi) if split else None
                scale = torch.zeros((n_tasks, bs, HEAD_C), dtype=torch.float32, device=dev)
                shift = torch.zeros_like(scale)
            for i, t in enumerate(plan["tasks"]):
                for j, (name, seq) in enumerate(zip(t["names"], t["seqs"])):
                    o, wd = t["offs"][name]
                    last = seq[len(seq) - 1]
                    w_last[i, o:o + wd] = last.weight.detach().float().reshape(wd, HEAD_C)
                    bias[i, o:o + wd] = last.bias.detach().float()
                    if two:
                        conv, bn = seq[0][0], seq[0][1]
                        hi, lo = conv._packed(split)
                        w_hi[i, j] = hi
                        if split:
                            w_lo[i, j] = lo
                        sc, sh = F.fold_batchnorm(bn)
                        scale[i, j] = sc
                        shift[i, j] = sh if conv.bias is None else conv.bias.detach().float() * sc + sh
            return dict(w_hi=w_hi, w_lo=w_lo, scale=scale, shift=shift, w_last=w_last, bias=bias)

        return F.derived(self._cache, ("operands", split), params, build, tuple(f[1].eps for f in firsts))

    def head_rows(self, feats: torch.Tensor, indices: torch.Tensor, spatial_shape, batch_size: int, split: bool, nbr=None):
        """The conv stack: [N, 128] fp32 rows -> the head buffer [16 n_tasks, N] fp32 (also used by tests and tools)."""
        plan = self._plan()
        ops_ = self._operands(plan, split)
        kvol = 1
        if plan["num_conv"] == 2 and self.kernel_size_head == 3:
            kvol = 9
            if nbr is None:
                nbr = sparse_conv_rules(indices, spatial_shape, batch_size, 3, 1, 1, True)[1]
        return ops.sparse_head(feats, nbr if kvol == 9 else None, k_vol=kvol, task_n_br=[len(t["names"]) for t in plan["tasks"]],
                               chan_owner=[t["owner"] for t in plan["tasks"]], num_conv=plan["num_conv"], br_stride=plan["br_stride"],
                               tag="voxelnext_head_convs", **ops_)

    def _pred_dicts(self, buf):
        out = []
        for i, t in enumerate(self._plan()["tasks"]):
            out.append({n: buf[TASK_C * i + o:TASK_C * i + o + wd].t() for n, (o, wd) in t["offs"].items()})
        return out

    def decode_args(self, plan=None):
        """What lvq_voxel_decode takes besides the head buffer and the indices (also used by tests and tools)."""
        return center_decode_args(self, plan or self._plan(), TASK_C)

    def forward(self, data_dict):
        x = data_dict["encoded_spconv_tensor"]
        feats = x.features
        split = inference_split(self, "BatchNorm folded, no target assignment, no losses", feats,
                                mode=self.precision or getattr(x, "precision", None))
        post = self._post_cfg()                      # refusals come before any launch
        plan = self._plan()
        if feats.dim() != 2 or feats.shape[1] != HEAD_C or len(x.spatial_shape) != 2:
            raise F.LvqError(f"VoxelNeXtHead: expected a 2-D sparse tensor with {HEAD_C} channels, got features {tuple(feats.shape)} on "
                             f"{list(x.spatial_shape)}")
        F.require_cuda(feats.contiguous(), x.indices.contiguous(), *self.parameters())
        feats = feats.float().contiguous()
        indices = x.indices if x.indices.dtype == torch.int32 else x.indices.to(torch.int32)
        indices = indices.contiguous()
        batch_size = int(data_dict["batch_size"])
        buf = self.head_rows(feats, indices, x.spatial_shape, int(x.batch_size), split)
        self.forward_ret_dict["pred_dicts"] = self._pred_dicts(buf)
        self.forward_ret_dict["voxel_indices"] = x.indices
        self.forward_ret_dict["batch_index"] = x.indices[:, 0]
        if os.environ.get("LVQ_HEAD_TORCH_POST"):
            pred_dicts = self._torch_post(batch_size, indices, post)
        else:
            pred_dicts = self._kernel_post(buf, indices, batch_size, plan, post)
        data_dict["final_box_dicts"] = pred_dicts
        if self.predict_boxes_when_training:
            rois, roi_scores, roi_labels = self.reorder_rois_for_refining(batch_size, pred_dicts)
            data_dict["rois"], data_dict["roi_scores"], data_dict["roi_labels"] = rois, roi_scores, roi_labels
            data_dict["has_class_labels"] = True
        return data_dict

    def _kernel_post(self, buf, indices, batch_size, plan, post):
        boxes, scores, labels, counts = ops.voxel_decode(buf, indices, batch_size, k=post["k"], limit_range=post["limit"],
                                                         score_thresh=post["thresh"], tag="voxel_decode", **self.decode_args(plan))
        self.forward_ret_dict["candidate_counts"] = counts                   # [B, n_tasks] int32 on the device: survivors before NMS
        b, t, k, d = boxes.shape
        keep, keep_count = ops.nms_bev(boxes.view(b * t, k, d), counts.view(-1), thresh=post["nms_thresh"], pre_max=post["pre"],
                                       post_max=post["post"], tag="voxel_nms")
        kept = collect_kept(boxes, scores, labels, keep, keep_count, "voxel_collect")      # holds THE device-to-host copy of a forward
        return [dict(d, pred_ious=[None] * t) for d in kept]

    # ------------------------------------------------------------------------------------------------------------------------------
    # LVQ_HEAD_TORCH_POST=1: voxelnext_head.py:418-488 / centernet_utils.py:243-354 / model_nms_utils.py:6-25 as the reference's own torch ops
    # (class = the matrix row of _topk_1d's [n_cls, n_b] score matrix: the corrected class of the module docstring)
    # ------------------------------------------------------------------------------------------------------------------------------
    def _torch_post(self, batch_size, indices, post):
        K, dev = post["k"], indices.device
        limit = torch.tensor(post["limit"], dtype=torch.float32, device=dev)
        stride, vs, rng = self.feature_map_stride, self.voxel_size, self.point_cloud_range
        batch_idx, spatial = indices[:, 0], indices[:, 1:]
        n_tasks = len(self.heads_list)
        ret = [dict(pred_boxes=[], pred_scores=[], pred_labels=[], pred_ious=[]) for _ in range(batch_size)]
        for idx, pd in enumerate(self.forward_ret_dict["pred_dicts"]):
            hm, dim = pd["hm"].sigmoid(), pd["dim"].exp()
            mapping = self.class_id_mapping_each_head[idx]
            for k in range(batch_size):
                rows = batch_idx == k
                score = hm[rows].permute(1, 0)                                  # [n_cls, n_b]
                n_b = score.shape[-1]
                kk = min(K, n_b)
                topk_scores, topk_inds = torch.topk(score, kk)
                sc, topk_ind = torch.topk(topk_scores.reshape(-1), min(K, topk_scores.numel()))
                class_ids = (topk_ind // max(kk, 1)).int()                      # the row of the [n_cls, kk] matrix (the reference: // K)
                inds = topk_inds.reshape(-1).gather(0, topk_ind)

                def gather(feat):                                               # gather_feat_idx
                    return feat[rows][inds]

                center, center_z = gather(pd["center"]), gather(pd["center_z"])
                sp = gather(spatial)
                angle = torch.atan2(gather(pd["rot"][:, 1:2]), gather(pd["rot"][:, 0:1]))
                xs = (sp[:, -1:] + center[:, 0:1]) * stride * vs[0] + rng[0]
                ys = (sp[:, -2:-1] + center[:, 1:2]) * stride * vs[1] + rng[1]
                parts = [xs, ys, center_z, gather(dim), angle] + ([gather(pd["vel"])] if "vel" in pd else [])
                box_preds = torch.cat(parts, dim=-1)
                mask = (box_preds[:, :3] >= limit[:3]).all(1) & (box_preds[:, :3] <= limit[3:]).all(1)
                if post["thresh"] is not None:
                    mask &= sc > post["thresh"]
                cur_boxes, cur_scores = box_preds[mask], sc[mask]
                cur_labels = mapping[class_ids[mask].long()]
                selected = class_agnostic_nms_torch(cur_boxes, cur_scores, post)
                ret[k]["pred_boxes"].append(cur_boxes[selected])
                ret[k]["pred_scores"].append(cur_scores[selected])
                ret[k]["pred_labels"].append(cur_labels[selected])
                ret[k]["pred_ious"].append(None)
        for k in range(batch_size):
            ret[k]["pred_boxes"] = torch.cat(ret[k]["pred_boxes"], dim=0)
            ret[k]["pred_scores"] = torch.cat(ret[k]["pred_scores"], dim=0)
            ret[k]["pred_labels"] = torch.cat(ret[k]["pred_labels"], dim=0) + 1
        return ret


dense_heads_all = dict(DH.dense_heads_all, VoxelNeXtHead=VoxelNeXtHead)
