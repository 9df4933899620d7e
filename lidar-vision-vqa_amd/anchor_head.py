"""AnchorHeadSingle: `spatial_features_2d` -> a box for every anchor -> 3-D boxes, with the reference's module API
(pcdet/models/dense_heads/anchor_head_single.py, anchor_head_template.py:11-72 / 225-272) and the class-agnostic route of
Detector3DTemplate.post_processing (detectors/detector3d_template.py:178-283), on lvq_conv2d and the kernels of csrc/anchor_head.hip.
Inference only.

  AnchorGenerator(anchor_range, anchor_generator_config)       target_assigner/anchor_generator.py:17-60 in plain torch, on any device
  ResidualCoder(code_size=7)                                    box_coder_utils.py:45-80, decode_torch only
  AnchorHeadSingle(model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, predict_boxes_when_training)
  post_processing(batch_dict, post_process_cfg, num_class)      -> (pred_dicts, recall_dict = {})
  dense_heads_all                                               the registry of sparse_head plus AnchorHeadSingle

`conv_cls`, `conv_box`, `conv_dir_cls` are the reference's nn.Conv2d(kernel_size=1) in the reference's order, so state_dict() keys and
shapes are the reference's (a checkpoint's `dense_head.*` keys load with strict=True) and the initialisation (cls bias -log(99), box
weight N(0, 0.001)) consumes the RNG as the reference does.  The constructor moves nothing to a device: `anchors`, the reference's list
of [1, H, W, 1, n_rot, 7] tensors, are non-persistent buffers (`anchors_{i}`) that follow .to().

forward(data_dict), eval() under torch.no_grad():
  convs   spatial_features_2d goes once through lvq_conv2d_to_planes; the three 1 x 1 convs are ONE lvq_conv2d launch (kernel = stride =
          1): weights concatenated along C_out in the order cls | box | dir and zero-padded to a multiple of 64, the biases as the shift,
          fp32 NCHW output.  forward_ret_dict['cls_preds' | 'box_preds' | 'dir_cls_preds'] are [B, H, W, C] permuted views of it.
  decode  ONE lvq_anchor_decode: every anchor's box, max_k sigmoid and argmax, and -- when `candidate_score_thresh` is set on the module
          (POST_PROCESSING.SCORE_THRESH lives outside the head's own configuration) -- the set of anchors that reach it.
  writes  the reference's contract: data_dict['batch_cls_preds'] [B, N, n_cls] (raw logits), ['batch_box_preds'] [B, N, 7],
          ['cls_preds_normalized'] = False; and ours: ['anchor_scores'], ['anchor_labels'] [B, N] (also in forward_ret_dict) and
          ['anchor_candidates'] (the threshold, the list, its counts) or None, and ['anchor_source'], the two dense tensors themselves
          and the version of batch_cls_preds (_ffi.version_of), by which post_processing recognises that scores and labels belong to
          the batch_cls_preds it was given: another tensor, or the same one edited in place since, takes the "from elsewhere" route.
          batch_box_preds is read as it is at the call, so an edit of it needs no such check.  Under torch.inference_mode() the
          outputs are inference tensors, which count no versions: no version is recorded and post_processing always takes the "from
          elsewhere" route for them (an in-place edit could not be seen there).

post_processing, MULTI_CLASSES_NMS False, NMS_TYPE nms_gpu:
  ONE lvq_anchor_select (score mask `>=`, top NMS_PRE_MAXSIZE, equal scores towards the lower anchor index), ONE lvq_nms_bev_wide (two
  launches), ONE lvq_center_collect (n_tasks = 1; labels + 1 as int64) and exactly one device-to-host copy, of the keep counts.  When
  batch_dict carries the scores and labels of the forward that made its batch_cls_preds, the select reads them (and the candidate list, if
  its threshold is SCORE_THRESH); otherwise they are computed with torch ops first.  OUTPUT_RAW_SCORE replaces the scores by a torch
  gather of the max raw logit at the selected anchors.  LVQ_HEAD_TORCH_POST=1 routes through the reference's own sequence of torch ops
  (NMS = lvq_boxes_iou_bev + a host walk): the cross-check and the timing comparison, not a fallback (it needs the same library).

Supported: ResidualCoder with code_size 7 and no encode_angle_by_sincos; one anchor size and one bottom height per class, the same number
of rotations for every class; input channels <= 512; NMS_PRE_MAXSIZE <= 4096.  Anything else raises LvqError naming the limit, before any
launch.  `precision`: "bf16x3" (default) or "bf16", as on the other heads.

Shared with the other heads through head_common.py: the forward preamble (guard), the end of post_processing (collect_kept: the collect,
the copy, the slices) and the torch route's NMS (class_agnostic_nms_torch); the fused conv is dense_head._Fused with a 1 x 1 kernel.
"""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _ffi as F
from . import ops
from . import sparse_head as SH
from .backbone2d import to_planes
from .dense_head import _Fused
from .head_common import _get, cached_plan, class_agnostic_nms_torch, collect_kept, guard

MAX_PRE = 4096                 # lvq_anchor_select's sort rows and lvq_nms_bev_wide's 64 mask words
CODE_SIZE = 7


class AnchorGenerator:
    """target_assigner/anchor_generator.py:4-60.  `device` is where the anchors are built (the reference calls .cuda())."""

    def __init__(self, anchor_range, anchor_generator_config):
        self.anchor_generator_cfg = anchor_generator_config
        self.anchor_range = anchor_range
        self.anchor_sizes = [config["anchor_sizes"] for config in anchor_generator_config]
        self.anchor_rotations = [config["anchor_rotations"] for config in anchor_generator_config]
        self.anchor_heights = [config["anchor_bottom_heights"] for config in anchor_generator_config]
        self.align_center = [config.get("align_center", False) for config in anchor_generator_config]
        assert len(self.anchor_sizes) == len(self.anchor_rotations) == len(self.anchor_heights)
        self.num_of_anchor_sets = len(self.anchor_sizes)

    def generate_anchors(self, grid_sizes, device=None):
        assert len(grid_sizes) == self.num_of_anchor_sets
        all_anchors, num_anchors_per_location = [], []
        rng = self.anchor_range
        for grid_size, anchor_size, anchor_rotation, anchor_height, align_center in zip(
                grid_sizes, self.anchor_sizes, self.anchor_rotations, self.anchor_heights, self.align_center):
            num_anchors_per_location.append(len(anchor_rotation) * len(anchor_size) * len(anchor_height))
            if align_center:
                x_stride = (rng[3] - rng[0]) / grid_size[0]
                y_stride = (rng[4] - rng[1]) / grid_size[1]
                x_offset, y_offset = x_stride / 2, y_stride / 2
            else:
                x_stride = (rng[3] - rng[0]) / (grid_size[0] - 1)
                y_stride = (rng[4] - rng[1]) / (grid_size[1] - 1)
                x_offset, y_offset = 0, 0
            x_shifts = torch.arange(rng[0] + x_offset, rng[3] + 1e-5, step=x_stride, dtype=torch.float32).to(device)
            y_shifts = torch.arange(rng[1] + y_offset, rng[4] + 1e-5, step=y_stride, dtype=torch.float32).to(device)
            z_shifts = x_shifts.new_tensor(anchor_height)
            n_size, n_rot = len(anchor_size), len(anchor_rotation)
            rot = x_shifts.new_tensor(anchor_rotation)
            size = x_shifts.new_tensor(anchor_size)
            x_shifts, y_shifts, z_shifts = torch.meshgrid([x_shifts, y_shifts, z_shifts], indexing="ij")      # [x, y, z]
            anchors = torch.stack((x_shifts, y_shifts, z_shifts), dim=-1)
            anchors = anchors[:, :, :, None, :].repeat(1, 1, 1, size.shape[0], 1)
            size = size.view(1, 1, 1, -1, 3).repeat([*anchors.shape[0:3], 1, 1])
            anchors = torch.cat((anchors, size), dim=-1)
            anchors = anchors[:, :, :, :, None, :].repeat(1, 1, 1, 1, n_rot, 1)
            rot = rot.view(1, 1, 1, 1, -1, 1).repeat([*anchors.shape[0:3], n_size, 1, 1])
            anchors = torch.cat((anchors, rot), dim=-1)                       # [x, y, z, n_size, n_rot, 7]
            anchors = anchors.permute(2, 1, 0, 3, 4, 5).contiguous()          # [z, y, x, n_size, n_rot, 7]
            anchors[..., 2] += anchors[..., 5] / 2                            # bottom heights -> box centres
            all_anchors.append(anchors)
        return all_anchors, num_anchors_per_location


class ResidualCoder:
    """box_coder_utils.py:6-80, the decoding half."""

    def __init__(self, code_size=7, encode_angle_by_sincos=False, **kwargs):
        self.code_size = code_size
        self.encode_angle_by_sincos = encode_angle_by_sincos
        if encode_angle_by_sincos:
            raise F.LvqError("ResidualCoder: encode_angle_by_sincos is out of scope (lvq_anchor_decode reads one heading residual)")
        if code_size != CODE_SIZE:
            raise F.LvqError(f"ResidualCoder: code_size = {code_size}; lvq_anchor_decode decodes {CODE_SIZE}-wide boxes only")

    def decode_torch(self, box_encodings, anchors):
        xa, ya, za, dxa, dya, dza, ra = torch.split(anchors, 1, dim=-1)
        xt, yt, zt, dxt, dyt, dzt, rt = torch.split(box_encodings, 1, dim=-1)
        diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
        xg = xt * diagonal + xa
        yg = yt * diagonal + ya
        zg = zt * dza + za
        dxg = torch.exp(dxt) * dxa
        dyg = torch.exp(dyt) * dya
        dzg = torch.exp(dzt) * dza
        rg = rt + ra
        return torch.cat([xg, yg, zg, dxg, dyg, dzg, rg], dim=-1)

    def encode_torch(self, *args, **kwargs):
        raise F.LvqError("ResidualCoder.encode_torch: training targets are out of scope (inference-only kernels)")


def _fused_1x1(convs: List[nn.Conv2d], c_in: int, c_out: int) -> _Fused:
    """dense_head._Fused with a 1 x 1 kernel: the head's convs as one conv C -> c_out, the biases as the shift."""
    def weight():
        w = convs[0].weight.new_zeros((c_out, c_in, 1, 1), dtype=torch.float32)
        row = 0
        for m in convs:
            w[row:row + m.out_channels] = m.weight.detach().float()
            row += m.out_channels
        return w

    def affine():
        shift = convs[0].weight.new_zeros((c_out,), dtype=torch.float32)
        row = 0
        for m in convs:
            shift[row:row + m.out_channels] = m.bias.detach().float()
            row += m.out_channels
        return torch.ones_like(shift), shift

    fused = _Fused(convs, c_in, c_out, False, weight, affine, [m.weight for m in convs] + [m.bias for m in convs])
    fused.kernel, fused.stride, fused.padding = 1, 1, 0
    return fused


class AnchorHeadSingle(nn.Module):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, predict_boxes_when_training=True,
                 **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.class_names = class_names
        self.predict_boxes_when_training = predict_boxes_when_training
        self.use_multihead = _get(model_cfg, "USE_MULTIHEAD", False)
        if self.use_multihead:
            raise F.LvqError("AnchorHeadSingle: USE_MULTIHEAD (AnchorHeadMulti's anchor layout) is out of scope")
        target_cfg = model_cfg.TARGET_ASSIGNER_CONFIG
        coder = _get(target_cfg, "BOX_CODER", "ResidualCoder")
        if coder != "ResidualCoder":
            raise F.LvqError(f"AnchorHeadSingle: BOX_CODER {coder!r} has no kernel (ResidualCoder only; PreviousResidualDecoder and the "
                             "other coders are out of scope)")
        self.box_coder = ResidualCoder(num_dir_bins=_get(target_cfg, "NUM_DIR_BINS", 6), **dict(_get(target_cfg, "BOX_CODER_CONFIG", {})))
        gen_cfg = model_cfg.ANCHOR_GENERATOR_CONFIG
        for c in gen_cfg:
            if len(c["anchor_bottom_heights"]) != 1:
                raise F.LvqError(f"AnchorHeadSingle: {len(c['anchor_bottom_heights'])} anchor_bottom_heights for {c.get('class_name')!r}; one per "
                                 "class (the reference's flat view of [nz, ny, nx, ...] anchors does not match its channel layout otherwise)")
            if len(c["anchor_sizes"]) != 1:
                raise F.LvqError(f"AnchorHeadSingle: {len(c['anchor_sizes'])} anchor_sizes for {c.get('class_name')!r}; one per class")
        if len({len(c["anchor_rotations"]) for c in gen_cfg}) != 1:
            raise F.LvqError("AnchorHeadSingle: the classes have different numbers of anchor_rotations; the anchors of a cell are "
                             "[n_classes, n_rot] with one n_rot")
        anchors, per_location = self.generate_anchors(gen_cfg, grid_size=grid_size, point_cloud_range=point_cloud_range,
                                                      anchor_ndim=self.box_coder.code_size)
        for i, a in enumerate(anchors):
            self.register_buffer(f"anchors_{i}", a, persistent=False)         # follows .to(); not a state_dict key
        self._n_anchor_sets = len(anchors)
        self.forward_ret_dict = {}
        self.build_losses(_get(model_cfg, "LOSS_CONFIG", {}))

        self.num_anchors_per_location = sum(per_location)
        self.conv_cls = nn.Conv2d(input_channels, self.num_anchors_per_location * self.num_class, kernel_size=1)
        self.conv_box = nn.Conv2d(input_channels, self.num_anchors_per_location * self.box_coder.code_size, kernel_size=1)
        if _get(model_cfg, "USE_DIRECTION_CLASSIFIER", None) is not None:
            self.conv_dir_cls = nn.Conv2d(input_channels, self.num_anchors_per_location * model_cfg.NUM_DIR_BINS, kernel_size=1)
        else:
            self.conv_dir_cls = None
        self.init_weights()
        self.precision: Optional[str] = None          # None -> "bf16x3"
        self.candidate_score_thresh: Optional[float] = None      # POST_PROCESSING.SCORE_THRESH, when the decode should list who reaches it

    @property
    def anchors(self):
        return [getattr(self, f"anchors_{i}") for i in range(self._n_anchor_sets)]

    @staticmethod
    def generate_anchors(anchor_generator_cfg, grid_size, point_cloud_range, anchor_ndim=7):
        generator = AnchorGenerator(anchor_range=point_cloud_range, anchor_generator_config=anchor_generator_cfg)
        grid = np.asarray(grid_size)
        feature_map_size = [grid[:2] // config["feature_map_stride"] for config in anchor_generator_cfg]
        return generator.generate_anchors(feature_map_size)

    def init_weights(self):
        pi = 0.01
        nn.init.constant_(self.conv_cls.bias, -np.log((1 - pi) / pi))
        nn.init.normal_(self.conv_box.weight, mean=0, std=0.001)

    def build_losses(self, losses_cfg):
        """The reference registers a focal, a smooth-L1 and a cross-entropy loss here; they hold no parameters, and there is no training route."""
        self.add_module("cls_loss_func", nn.Module())
        self.add_module("reg_loss_func", nn.Module())
        self.add_module("dir_loss_func", nn.Module())

    def assign_targets(self, *args, **kwargs):
        raise F.LvqError("AnchorHeadSingle.assign_targets: training targets are out of scope (inference-only kernels)")

    def get_loss(self, *args, **kwargs):
        raise F.LvqError("AnchorHeadSingle.get_loss: the losses are out of scope (inference-only kernels)")

    # ------------------------------------------------------------------------------------------------------------------------------
    def _plan(self):
        return cached_plan(self, self._build_plan)

    def _build_plan(self):
        c_in = self.conv_cls.in_channels
        if c_in > 512:
            raise F.LvqError(f"AnchorHeadSingle: {c_in} input channels; lvq_conv2d takes at most 512")
        convs = [self.conv_cls, self.conv_box] + ([self.conv_dir_cls] if self.conv_dir_cls is not None else [])
        offs, o = [], 0
        for m in convs:
            offs.append(o)
            o += m.out_channels
        c_out = (o + 63) // 64 * 64
        if c_out > 512:
            raise F.LvqError(f"AnchorHeadSingle: {o} output channels in all; one lvq_conv2d launch writes at most 512")
        return dict(fused=_fused_1x1(convs, c_in, c_out), c_out=c_out, cls=offs[0], box=offs[1], dir=offs[2] if len(convs) == 3 else -1)

    def flat_anchors(self):
        """The anchors as generate_predicted_boxes flattens them: [H * W * A, 7] in the order (y, x, class, rotation); cached per version."""
        bufs = self.anchors
        return F.derived(self.__dict__.setdefault("_anchor_cache", {}), str(bufs[0].device), tuple(bufs),
                         lambda: torch.cat(bufs, dim=-3).reshape(-1, bufs[0].shape[-1]).float().contiguous())

    def decode_args(self, plan=None):
        """What lvq_anchor_decode takes besides the maps and the anchors (also used by tests and tools)."""
        plan = plan or self._plan()
        has_dir = self.conv_dir_cls is not None
        return dict(n_anchors=self.num_anchors_per_location, n_cls=self.num_class, cls_channel=plan["cls"], box_channel=plan["box"],
                    dir_channel=plan["dir"], n_dir_bins=int(self.model_cfg.NUM_DIR_BINS) if has_dir else 0,
                    dir_offset=float(self.model_cfg.DIR_OFFSET) if has_dir else 0.0,
                    dir_limit_offset=float(self.model_cfg.DIR_LIMIT_OFFSET) if has_dir else 0.0)

    def _maps(self, x: torch.Tensor, split: bool):
        """[B, C, H, W] fp32 -> maps [B, c_out, H, W] fp32: cls | box | dir channels, zeros behind them."""
        plan = self._plan()
        b, _, h, w = x.shape
        maps = torch.empty((b, plan["c_out"], h, w), dtype=torch.float32, device=x.device)
        plan["fused"].run(to_planes(x, split), split, f32=maps)
        return maps

    def forward(self, data_dict):
        x = data_dict["spatial_features_2d"]
        split = guard(self, "no target assignment, no losses", x, extra_cuda=self.anchors)
        plan = self._plan()                            # refusals come before any launch
        a0 = self.anchors[0]
        if tuple(x.shape[2:]) != tuple(a0.shape[1:3]):
            raise F.LvqError(f"AnchorHeadSingle: spatial_features_2d is {x.shape[2]} x {x.shape[3]}, the anchors were built for "
                             f"{a0.shape[1]} x {a0.shape[2]} (grid_size // feature_map_stride)")
        batch_size = int(data_dict["batch_size"])
        if batch_size != x.shape[0]:
            raise F.LvqError(f"AnchorHeadSingle: batch_size = {batch_size}, spatial_features_2d holds {x.shape[0]} scenes")
        maps = self._maps(x.float().contiguous(), split)
        ret, A = self.forward_ret_dict, self.num_anchors_per_location
        ret["cls_preds"] = maps[:, plan["cls"]:plan["cls"] + A * self.num_class].permute(0, 2, 3, 1)
        ret["box_preds"] = maps[:, plan["box"]:plan["box"] + A * CODE_SIZE].permute(0, 2, 3, 1)
        if self.conv_dir_cls is not None:
            ret["dir_cls_preds"] = maps[:, plan["dir"]:plan["dir"] + A * int(self.model_cfg.NUM_DIR_BINS)].permute(0, 2, 3, 1)
        thresh = self.candidate_score_thresh
        cls_preds, box_preds, scores, labels, cand, cand_count = ops.anchor_decode(
            maps, self.flat_anchors(), score_thresh=None if thresh is None else float(thresh), tag="anchor_decode", **self.decode_args(plan))
        ret["anchor_scores"], ret["anchor_labels"] = scores, labels
        data_dict["batch_cls_preds"], data_dict["batch_box_preds"] = cls_preds, box_preds
        data_dict["cls_preds_normalized"] = False
        data_dict["anchor_scores"], data_dict["anchor_labels"] = scores, labels
        data_dict["anchor_candidates"] = None if cand is None else (float(thresh), cand, cand_count)
        data_dict["anchor_source"] = (cls_preds, box_preds, None if cls_preds.is_inference() else F.version_of((cls_preds,)))
        return data_dict


# ----------------------------------------------------------------------------------------------------------------------------------
# Detector3DTemplate.post_processing, MULTI_CLASSES_NMS False
# ----------------------------------------------------------------------------------------------------------------------------------
def _post_cfg(post_process_cfg):
    nms = post_process_cfg.NMS_CONFIG
    if _get(nms, "MULTI_CLASSES_NMS", False):
        raise F.LvqError("post_processing: MULTI_CLASSES_NMS is out of scope (the class-agnostic route only)")
    if nms.NMS_TYPE != "nms_gpu":
        raise F.LvqError(f"post_processing: NMS_TYPE {nms.NMS_TYPE!r} has no kernel (nms_gpu only; nms_normal_gpu is out of scope)")
    pre = int(nms.NMS_PRE_MAXSIZE)
    if pre > MAX_PRE:
        raise F.LvqError(f"post_processing: NMS_PRE_MAXSIZE = {pre}; lvq_anchor_select and lvq_nms_bev_wide take at most {MAX_PRE} rows")
    if pre <= 0 or int(nms.NMS_POST_MAXSIZE) <= 0:
        raise F.LvqError(f"post_processing: NMS_PRE_MAXSIZE = {pre}, NMS_POST_MAXSIZE = {nms.NMS_POST_MAXSIZE}")
    return dict(thresh=_get(post_process_cfg, "SCORE_THRESH"), nms_thresh=float(nms.NMS_THRESH), pre=pre, post=int(nms.NMS_POST_MAXSIZE),
                raw=bool(_get(post_process_cfg, "OUTPUT_RAW_SCORE", False)))


def post_processing(batch_dict, post_process_cfg, num_class):
    """detector3d_template.py:178-283 without MULTI_CLASSES_NMS.  Returns (pred_dicts, recall_dict): per scene pred_boxes [n, 7],
    pred_scores [n], pred_labels [n] int64 (1-based); recall_dict is {} (the recall bookkeeping is out of scope)."""
    post = _post_cfg(post_process_cfg)                 # refusals come before any launch
    if batch_dict.get("has_class_labels", False) or "roi_labels" in batch_dict:
        raise F.LvqError("post_processing: has_class_labels / roi_labels (second-stage use) are out of scope")
    cls, box = batch_dict["batch_cls_preds"], batch_dict["batch_box_preds"]
    if isinstance(cls, (list, tuple)) or batch_dict.get("batch_index", None) is not None or box.dim() != 3:
        raise F.LvqError("post_processing: a list of batch_cls_preds (multi-head) and the flat batch_index form are out of scope; "
                         "expected batch_cls_preds [B, N, n_cls] and batch_box_preds [B, N, 7]")
    if cls.shape[-1] not in (1, num_class) or box.shape[-1] != CODE_SIZE or cls.shape[:2] != box.shape[:2]:
        raise F.LvqError(f"post_processing: batch_cls_preds {tuple(cls.shape)} / batch_box_preds {tuple(box.shape)} with num_class = {num_class}")
    batch_size = int(batch_dict["batch_size"])
    if batch_size != box.shape[0]:
        raise F.LvqError(f"post_processing: batch_size = {batch_size}, batch_box_preds holds {box.shape[0]} scenes")
    for t in (cls, box):                               # a view such as batch_cls_preds[..., :1] is fine: nothing below needs its layout
        if not t.is_cuda:
            F.require_cuda(t)
    normalized = bool(batch_dict.get("cls_preds_normalized", False))
    if os.environ.get("LVQ_HEAD_TORCH_POST"):
        return _torch_post(cls, box, normalized, post), {}
    src = batch_dict.get("anchor_source")
    cand = cand_count = None
    if src is not None and src[0] is cls and src[1] is box and not normalized and not cls.is_inference() and \
            src[2] is not None and F.version_of((cls,)) == src[2]:
        scores, labels = batch_dict["anchor_scores"], batch_dict["anchor_labels"]
        listed = batch_dict.get("anchor_candidates")
        if listed is not None and post["thresh"] is not None and np.float32(listed[0]) == np.float32(post["thresh"]):
            cand, cand_count = listed[1], listed[2]
    else:                                              # batch_cls_preds from elsewhere
        scores, labels = (cls if normalized else torch.sigmoid(cls)).float().max(dim=-1)
        scores, labels = scores.contiguous(), labels.to(torch.int32).contiguous()
    box = box.float().contiguous()
    sel_boxes, sel_scores, sel_labels, sel_index, sel_count = ops.anchor_select(
        scores, labels, box, score_thresh=post["thresh"], pre_max=post["pre"], cand=cand, cand_count=cand_count, tag="anchor_select")
    keep, keep_count = ops.nms_bev_wide(sel_boxes, sel_count, thresh=post["nms_thresh"], pre_max=post["pre"], post_max=post["post"],
                                        tag="anchor_nms")
    b, k = sel_scores.shape
    raw = None
    if post["raw"]:                                    # max_k of the raw logits at the selected anchors
        anchor = sel_index.gather(1, keep.clamp(min=0).long()).clamp(min=0).long()
        raw = cls.gather(1, anchor.unsqueeze(-1).expand(-1, -1, cls.shape[-1])).max(dim=-1)[0]
    return collect_kept(sel_boxes.view(b, 1, k, CODE_SIZE), sel_scores.view(b, 1, k), sel_labels.view(b, 1, k), keep, keep_count,
                        "anchor_collect", pred_scores=raw), {}      # holds THE device-to-host copy


def _torch_post(cls, box, normalized, post):
    """LVQ_HEAD_TORCH_POST=1: detector3d_template.py:207-282 / model_nms_utils.py:6-25 as the reference's own torch ops."""
    out = []
    for index in range(box.shape[0]):
        box_preds, src_cls_preds = box[index], cls[index]
        cls_preds = src_cls_preds if normalized else torch.sigmoid(src_cls_preds)
        cls_preds, label_preds = torch.max(cls_preds, dim=-1)
        label_preds = label_preds + 1
        box_scores, boxes_m = cls_preds, box_preds
        if post["thresh"] is not None:
            scores_mask = box_scores >= post["thresh"]
            box_scores, boxes_m = box_scores[scores_mask], box_preds[scores_mask]
        selected = class_agnostic_nms_torch(boxes_m, box_scores, post)
        if post["thresh"] is not None:
            selected = scores_mask.nonzero().view(-1)[selected]
        final_scores = torch.max(src_cls_preds, dim=-1)[0][selected] if post["raw"] else cls_preds[selected]
        out.append(dict(pred_boxes=box_preds[selected], pred_scores=final_scores, pred_labels=label_preds[selected]))
    return out


dense_heads_all = dict(SH.dense_heads_all, AnchorHeadSingle=AnchorHeadSingle)
