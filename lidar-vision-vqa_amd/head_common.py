"""What the detection heads share in Python (dense_head, sparse_head, anchor_head, transfusion_head) and, for `_get`, `guard` and
`cached_plan`, backbone2d.  It imports none of them; they import from here.  The kernels' shared side is csrc/head_common.h.

  _get(cfg, key, default)                       a configuration value from a dict or an attribute object; None counts as missing
  guard(module, why, *tensors, extra_cuda=())   the forward preamble: inference only, a known precision, [B, C, H, W] on the device
  inference_split(module, why, *tensors)        its first half (inference only, a known precision) -> True for "bf16x3"
  cached_plan(module, build)                    the plan of a module, built once (`_plan_cache` in the instance's __dict__)
  CenterStyleHead                               base of CenterHead and VoxelNeXtHead: class-id mappings, the inference-only stubs,
                                                reorder_rois_for_refining
  center_tasks, center_decode_args, center_post_cfg     the branch tables, decode arguments and post-processing limits of those two
  collect_kept                                  lvq_center_collect + THE one device-to-host copy of a forward + the per-scene slices
  class_agnostic_nms_torch, greedy_keep         the reference's class_agnostic_nms as torch ops (LVQ_HEAD_TORCH_POST=1) and its host walk
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _ffi as F
from . import autograd_route as AG
from . import ops

MODES = ("bf16x3", "bf16")
DEFAULT_MODE = "bf16x3"
MAX_K = 1024                   # rows of the decode kernels' sort buffer
BOX_BRANCHES = {"center": 2, "center_z": 1, "dim": 3, "rot": 2, "vel": 2}


def _get(cfg, key, default=None):
    v = cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)
    return default if v is None else v


def cached_plan(module, build):
    plan = module.__dict__.get("_plan_cache")
    if plan is None:
        plan = module.__dict__["_plan_cache"] = build()
    return plan


def inference_split(module, why: str, *tensors, mode=None) -> bool:
    """Refuses train() mode / gradients in reach and an unknown precision.  `why` is the class's own reason inside the message;
    `mode` overrides module.precision (None: the default).  Returns True for "bf16x3"."""
    name = type(module).__name__
    if AG.wanted(module, *tensors):
        raise F.LvqError(f"{name}: inference-only kernels ({why}); call it in eval() mode under torch.no_grad()")
    mode = mode or module.precision or DEFAULT_MODE
    if mode not in MODES:
        raise F.LvqError(f"{name} runs in {MODES}, not {mode!r}")
    return mode == "bf16x3"


def guard(module, why: str, *tensors, extra_cuda=()) -> bool:
    """inference_split, then: every tensor is [B, C, H, W], and the tensors, the module's parameters and `extra_cuda` are on the device."""
    split = inference_split(module, why, *tensors)
    for t in tensors:
        if t.dim() != 4:
            raise F.LvqError(f"{type(module).__name__}: expected [B, C, H, W], got {tuple(t.shape)}")
    F.require_cuda(*[t.contiguous() for t in tensors], *module.parameters(), *extra_cuda)
    return split


class CenterStyleHead(nn.Module):
    """What CenterHead and VoxelNeXtHead register besides their convs: `class_names_each_head`, the non-persistent `class_id_mapping_{i}`
    buffers (they follow .to() and are no state_dict keys) and the parameter-free loss placeholders.  Nothing here draws from the RNG."""

    def _init_class_maps(self, model_cfg, class_names):
        self.class_names = class_names
        self.class_names_each_head = []
        for i, cur_class_names in enumerate(model_cfg.CLASS_NAMES_EACH_HEAD):
            self.class_names_each_head.append([x for x in cur_class_names if x in class_names])
            mapping = torch.tensor([self.class_names.index(x) for x in cur_class_names if x in class_names], dtype=torch.int64)
            self.register_buffer(f"class_id_mapping_{i}", mapping, persistent=False)
        total_classes = sum(len(x) for x in self.class_names_each_head)
        assert total_classes == len(self.class_names), f"class_names_each_head={self.class_names_each_head}"

    @property
    def class_id_mapping_each_head(self):
        return [getattr(self, f"class_id_mapping_{i}") for i in range(len(self.class_names_each_head))]

    def build_losses(self):
        """The reference registers a focal and a regression loss here; they hold no parameters, and there is no training route."""
        self.add_module("hm_loss_func", nn.Module())
        self.add_module("reg_loss_func", nn.Module())

    def assign_targets(self, *args, **kwargs):
        raise F.LvqError(f"{type(self).__name__}.assign_targets: training targets are out of scope (inference-only kernels)")

    def get_loss(self, *args, **kwargs):
        raise F.LvqError(f"{type(self).__name__}.get_loss: the losses are out of scope (inference-only kernels)")

    @staticmethod
    def reorder_rois_for_refining(batch_size, pred_dicts):
        """center_head.py:367-383, plain torch."""
        num_max_rois = max(1, max(len(d["pred_boxes"]) for d in pred_dicts))        # at least one faked roi
        pred_boxes = pred_dicts[0]["pred_boxes"]
        rois = pred_boxes.new_zeros((batch_size, num_max_rois, pred_boxes.shape[-1]))
        roi_scores = pred_boxes.new_zeros((batch_size, num_max_rois))
        roi_labels = pred_boxes.new_zeros((batch_size, num_max_rois)).long()
        for b in range(batch_size):
            n = len(pred_dicts[b]["pred_boxes"])
            rois[b, :n, :] = pred_dicts[b]["pred_boxes"]
            roi_scores[b, :n] = pred_dicts[b]["pred_scores"]
            roi_labels[b, :n] = pred_dicts[b]["pred_labels"]
        return rois, roi_scores, roi_labels


def center_tasks(name, heads_list, class_names_each_head, task_c, head_order, class_names, max_branches=None, no_kernel_note="",
                 task_writes="a task writes", task_rule=None, head_rule=None):
    """The branch tables of a centre-style head, validated: per task `names`, `offs` {branch: (first channel, width)}, `widths`, `n_cls`,
    `num_conv` (per branch); for the head `vel` and `class_map`.  `name` prefixes the refusals; no_kernel_note and task_writes are the
    caller's words inside two of them.  Which num_conv values are served is the caller's rule: task_rule(i, num_conv) runs per task
    in front of the width check, head_rule(tasks) once in front of the vel check."""
    tasks = []
    for i, head in enumerate(heads_list):
        names = list(head.sep_head_dict)
        for n in names:
            if n != "hm" and n not in BOX_BRANCHES:
                raise F.LvqError(f"{name}: branch {n!r} has no kernel ({no_kernel_note}the branches are {sorted(BOX_BRANCHES)} and hm)")
            if n != "hm" and head.sep_head_dict[n]["out_channels"] != BOX_BRANCHES[n]:
                raise F.LvqError(f"{name}: branch {n!r} has {head.sep_head_dict[n]['out_channels']} channels, the decode reads {BOX_BRANCHES[n]}")
        missing = [n for n in ("center", "center_z", "dim", "rot") if n not in names]
        if missing:
            raise F.LvqError(f"{name}: task {i} lacks the branches {missing}")
        if max_branches is not None and len(names) > max_branches:
            raise F.LvqError(f"{name}: task {i} has {len(names)} branches; lvq_sparse_head takes at most {max_branches}")
        num_conv = [int(head.sep_head_dict[n]["num_conv"]) for n in names]
        if task_rule is not None:
            task_rule(i, num_conv)
        widths = [int(head.sep_head_dict[n]["out_channels"]) for n in names]
        if sum(widths) > task_c:
            raise F.LvqError(f"{name}: task {i} has {sum(widths)} output channels; {task_writes} at most {task_c}")
        offs, o = {}, 0
        for n, wd in zip(names, widths):
            offs[n], o = (o, wd), o + wd
        tasks.append(dict(names=names, offs=offs, widths=widths, n_cls=len(class_names_each_head[i]), num_conv=num_conv))
    if head_rule is not None:
        head_rule(tasks)
    vel = "vel" in list(head_order)
    if any(("vel" in t["offs"]) != vel for t in tasks):
        raise F.LvqError(f"{name}: 'vel' is in HEAD_ORDER of some tasks' branches only")
    return dict(tasks=tasks, vel=vel, class_map=[class_names.index(x) for names in class_names_each_head for x in names])


def center_decode_args(head, plan, task_c):
    """What lvq_center_decode / lvq_voxel_decode take besides their maps: task i's channels start at task_c * i."""
    chans = []
    for i, t in enumerate(plan["tasks"]):
        o = t["offs"]
        chans.append([task_c * i + o[n][0] if n in o else -1 for n in ("center", "center_z", "dim", "rot", "vel", "hm")])
    return dict(task_channels=chans, task_n_cls=[t["n_cls"] for t in plan["tasks"]], class_map=plan["class_map"],
                box_dim=9 if plan["vel"] else 7, stride=int(head.feature_map_stride),
                voxel_xy=[float(head.voxel_size[0]), float(head.voxel_size[1])],
                range_xy=[float(head.point_cloud_range[0]), float(head.point_cloud_range[1])])


def center_post_cfg(name, post, decode_symbol, nms_note="", rectifier=False, positive_k=False):
    """POST_PROCESSING of a centre-style head as the dict its post-processing reads, after the refusals.  nms_note: the caller's own
    words behind the NMS_TYPE refusal; rectifier: refuse USE_IOU_TO_RECTIFY_SCORE; positive_k: refuse MAX_OBJ_PER_SAMPLE <= 0 too."""
    nms = post.NMS_CONFIG
    if nms.NMS_TYPE != "nms_gpu":
        raise F.LvqError(f"{name}: NMS_TYPE {nms.NMS_TYPE!r} has no kernel (nms_gpu under class_agnostic_nms only{nms_note})")
    if rectifier and _get(post, "USE_IOU_TO_RECTIFY_SCORE", False):
        raise F.LvqError(f"{name}: USE_IOU_TO_RECTIFY_SCORE needs an 'iou' branch, which is out of scope")
    k = int(post.MAX_OBJ_PER_SAMPLE)
    if k > MAX_K or (positive_k and k <= 0):
        raise F.LvqError(f"{name}: MAX_OBJ_PER_SAMPLE = {k}; {decode_symbol} sorts {'1 ..' if positive_k else 'at most'} {MAX_K} candidates")
    return dict(k=k, thresh=_get(post, "SCORE_THRESH"), limit=[float(v) for v in post.POST_CENTER_LIMIT_RANGE],
                nms_thresh=float(nms.NMS_THRESH), pre=int(nms.NMS_PRE_MAXSIZE), post=int(nms.NMS_POST_MAXSIZE))


def collect_kept(boxes, scores, labels, keep, keep_count, tag, pred_scores=None):
    """boxes [B, T, K, D], scores / labels [B, T, K], keep [B * T, post_max], keep_count [B * T] -> per scene a dict of pred_boxes,
    pred_scores, pred_labels (int64, 1-based): ONE lvq_center_collect, then THE device-to-host copy of a forward (the keep counts) and
    slices of the collected buffers.  pred_scores [B, T * post_max] stands in for the collected scores (OUTPUT_RAW_SCORE)."""
    out_b, out_s, out_l, _ = ops.center_collect(boxes, scores, labels, keep, keep_count, tag=tag)
    out_s = out_s if pred_scores is None else pred_scores
    b, t = boxes.shape[:2]
    totals = keep_count.view(b, t).cpu().sum(dim=1).tolist()
    return [dict(pred_boxes=out_b[s, :n], pred_scores=out_s[s, :n], pred_labels=out_l[s, :n]) for s, n in enumerate(totals)]


def greedy_keep(over, post_max):
    """The host walk of nms_gpu over a boolean [n, n] matrix (`over[i, j]`: row i suppresses row j; only j > i is read), rows in
    descending score order: the kept row numbers, ascending, at most post_max of them."""
    if over.shape[0] == 0:
        return []
    kept, gone = [], over[0] & False
    for i in range(over.shape[0]):
        if not gone[i]:
            kept.append(i)
            gone[i + 1:] |= over[i, i + 1:]
    return kept[:post_max]


def class_agnostic_nms_torch(boxes, scores, post):
    """model_nms_utils.py:6-25 with score_thresh=None as torch ops (IoU = lvq_boxes_iou_bev): the selected rows of `boxes`, int64."""
    if scores.shape[0] == 0:
        return torch.zeros((0,), dtype=torch.int64, device=boxes.device)
    nms_scores, indices = torch.topk(scores, k=min(post["pre"], scores.shape[0]))
    order = nms_scores.sort(0, descending=True)[1]                          # nms_gpu's own sort
    nms_boxes = boxes[indices][order][:, :7].float().contiguous()
    over = (ops.boxes_iou_bev(nms_boxes, nms_boxes) > post["nms_thresh"]).cpu().numpy()
    kept = greedy_keep(over, post["post"])
    return indices[order[torch.tensor(kept, dtype=torch.int64, device=boxes.device)]]
