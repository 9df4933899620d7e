#!/usr/bin/env python3
"""tools/make_center_head_golden.py -- tests/golden/center_head_<case>.npz from the UNMODIFIED reference CenterHead
(pcdet/models/dense_heads/center_head.py:49-416) and centernet_utils.decode_bbox_from_heatmap (centernet_utils.py:155-241).

Runs only where the reference is mounted (tools/make_goldens.py explains the pattern: empty parent packages are registered so that no
pcdet/**/__init__.py is executed; weights and inputs come from seeds).  What the generator's environment lacks is stubbed in sys.modules before the
import: `numba` (an identity `jit`: centernet_utils decorates two numpy helpers the head never calls at inference), `easydict`,
`SharedArray`, and the compiled `pcdet.ops.iou3d_nms.iou3d_nms_cuda` / `pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda` extensions.
The constructor's and generate_predicted_boxes' `.cuda()` calls run inside ref_standins.cuda_is_identity().

What the fixtures pin, and what they do not (compare tools/ref_standins.py).  The raw maps (`pred_dicts` of the reference's own forward)
and the pre-NMS lists (decode_bbox_from_heatmap, called with the arguments of center_head.py:317-326) come from the reference's code
with no stand-in.  The ONE stand-in that does arithmetic is `iou3d_nms_cuda.nms_gpu`: a greedy walk over the fp64 rectangle-clipping IoU
of tests/center_head_cases.py.  The final lists therefore pin the reference's WIRING around that call -- orders, masks, the pre- and
post-NMS truncations, label mapping, concatenation in head order, the 1-based labels -- and NOT the rounding of the CUDA kernel, whose
1 cm corner margin nothing on this side can reproduce; the cases keep every IoU 0.02 away from the threshold so that it cannot matter.

Per case of center_head_cases.MODULE_CASES the file keeps: `x` (the input), `keys` / `shapes` (the reference class's state_dict; the
values are center_head_cases.case_state(name), loaded with strict=True -- 5 MB of seeded weights stay out of the repository),
`maps_<task>_<branch>`, `pre_<task>_<scene>_{boxes,scores,labels}` and `final_<scene>_{boxes,scores,labels}`.

    python tools/make_center_head_golden.py            # rewrites the fixtures, asserts the margin conditions
    python tools/make_center_head_golden.py --search   # first input seed per case (from the case's xseed upwards) that meets them;
                                                        # restatement only, the reference is not needed

Printed on the last run (survivors before NMS -> kept, per scene; margins: K-th gap, |score - 0.1|, |iou - 0.2|, |centre - limit|):
    nusc     scene 0: 184 -> 170   scene 1: 179 -> 169   margins 1.42e-03 2.06e-01 2.05e-02 1.86e-02   292 KiB
    single   scene 0: 30 -> 29   scene 1: 32 -> 29   margins 4.26e-03 6.72e-01 8.58e-02 1.44e-01   147 KiB
    waymo    scene 0: 96 -> 90   scene 1: 92 -> 88   margins 1.51e-03 5.42e-01 1.60e-01 1.93e-02   223 KiB   (|iou - 0.7|)
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import center_head_cases as CC  # noqa: E402

REF = "/root/reference/src"
OUT = os.path.join(ROOT, "tests", "golden")
MARGINS = (1e-3, 1e-3, 0.02, 1e-2)              # K-th gap, |score - SCORE_THRESH|, |iou - NMS_THRESH|, |centre - limit|


def margins_ok(m):
    return all(a >= b for a, b in zip(m, MARGINS))


def search():
    for name, c in CC.MODULE_CASES.items():
        cfg = CC.case_cfg(name)
        for seed in range(c["xseed"], c["xseed"] + 100000):
            maps = CC.f32_maps(CC.head_maps(cfg, CC.case_state(name), CC.case_input(name, seed)))
            pre, final, near = CC.head_final(cfg, c["class_names"], maps, c["stride"], c["voxel_size"], c["point_cloud_range"])
            m = CC.module_margins(cfg, pre, near)
            if margins_ok(m):
                print(name, "xseed", seed, "margins", " ".join(f"{v:.2e}" for v in m), "kept", [len(f["pred_scores"]) for f in final],
                      "pre", [sum(len(t[s]["scores"]) for t in pre) for s in range(len(final))])
                break


def _stub(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def nms_gpu_standin(boxes, keep, thresh):
    """iou3d_nms_cuda.nms_gpu(boxes [n, 7] sorted, keep LongTensor [n] (written), thresh) -> number kept: the greedy walk in fp64."""
    kept, _ = CC.greedy_nms(boxes.detach().cpu().numpy().astype(np.float64), float(thresh), 10 ** 9, 10 ** 9)
    keep[:len(kept)] = torch.tensor(kept, dtype=torch.long)
    return len(kept)


def import_reference():
    def jit(*args, **kwargs):
        return args[0] if len(args) == 1 and callable(args[0]) and not kwargs else (lambda f: f)

    _stub("numba", jit=jit, njit=jit)
    _stub("easydict", EasyDict=CC.Cfg)
    _stub("SharedArray")
    le = os.path.join(REF, "lidar-encoder", "pcdet")
    for n, p in [("pcdet", le), ("pcdet.models", le + "/models"), ("pcdet.models.dense_heads", le + "/models/dense_heads"),
                 ("pcdet.models.model_utils", le + "/models/model_utils"), ("pcdet.utils", le + "/utils"), ("pcdet.ops", le + "/ops"),
                 ("pcdet.ops.iou3d_nms", le + "/ops/iou3d_nms"), ("pcdet.ops.roiaware_pool3d", le + "/ops/roiaware_pool3d")]:
        _stub(n, p)
    _stub("pcdet.ops.iou3d_nms.iou3d_nms_cuda", nms_gpu=nms_gpu_standin)
    _stub("pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda")
    head = importlib.import_module("pcdet.models.dense_heads.center_head")
    return head.CenterHead, importlib.import_module("pcdet.models.model_utils.centernet_utils")


@torch.no_grad()
def main():
    import ref_standins as RS
    torch.set_num_threads(8)
    cls, cu = import_reference()
    for name, c in CC.MODULE_CASES.items():
        cfg = CC.case_cfg(name)
        with RS.cuda_is_identity():
            m = cls(cfg, c["input_channels"], len(c["class_names"]), c["class_names"], np.array(c["grid_size"]), c["point_cloud_range"],
                    c["voxel_size"], predict_boxes_when_training=False)
            sd = m.state_dict()
            seeded = CC.case_state(name)
            m.load_state_dict({k: torch.from_numpy(np.asarray(seeded[k])).to(v.dtype).reshape(v.shape) for k, v in sd.items()}, strict=True)
            m.eval()
            x = CC.case_input(name)
            out = m(dict(spatial_features_2d=torch.from_numpy(x), batch_size=x.shape[0]))
            post = cfg.POST_PROCESSING
            store = dict(x=x, keys=np.array(list(sd.keys())), shapes=np.array([",".join(str(d) for d in v.shape) for v in sd.values()]))
            for i, pd in enumerate(m.forward_ret_dict["pred_dicts"]):
                for n, v in pd.items():
                    store[f"maps_{i}_{n}"] = v.numpy()
                pre = cu.decode_bbox_from_heatmap(
                    heatmap=pd["hm"].sigmoid(), rot_cos=pd["rot"][:, 0].unsqueeze(dim=1), rot_sin=pd["rot"][:, 1].unsqueeze(dim=1), center=pd["center"],
                    center_z=pd["center_z"], dim=pd["dim"].exp(), vel=pd["vel"] if "vel" in pd else None, iou=None,
                    point_cloud_range=m.point_cloud_range, voxel_size=m.voxel_size, feature_map_stride=m.feature_map_stride,
                    K=post.MAX_OBJ_PER_SAMPLE, circle_nms=False, score_thresh=post.SCORE_THRESH,
                    post_center_limit_range=torch.tensor(post.POST_CENTER_LIMIT_RANGE).float())
                for s, d in enumerate(pre):
                    store[f"pre_{i}_{s}_boxes"] = d["pred_boxes"].numpy()
                    store[f"pre_{i}_{s}_scores"] = d["pred_scores"].numpy()
                    store[f"pre_{i}_{s}_labels"] = d["pred_labels"].numpy().astype(np.int64)          # class ids inside the task, unmapped
            for s, d in enumerate(out["final_box_dicts"]):
                store[f"final_{s}_boxes"] = d["pred_boxes"].numpy()
                store[f"final_{s}_scores"] = d["pred_scores"].numpy()
                store[f"final_{s}_labels"] = d["pred_labels"].numpy().astype(np.int64)
        maps = [{n: store[f"maps_{i}_{n}"] for n in CC.branch_names(cfg)} for i in range(len(cfg.CLASS_NAMES_EACH_HEAD))]
        pre, final, near = CC.head_final(cfg, c["class_names"], maps, c["stride"], c["voxel_size"], c["point_cloud_range"])
        mg = CC.module_margins(cfg, pre, near)
        path = os.path.join(OUT, CC.golden_name(name))
        np.savez_compressed(path, **store)
        counts = "   ".join(f"scene {s}: {sum(len(t[s]['scores']) for t in pre)} -> {len(store[f'final_{s}_scores'])}" for s in range(x.shape[0]))
        print(f"    {name:8s} {counts}   margins {' '.join(f'{v:.2e}' for v in mg)}   {os.path.getsize(path) / 1024:.0f} KiB")
        assert margins_ok(mg), "a margin condition fails on the reference's maps: run --search and move the case's xseed"
        assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    search() if "--search" in sys.argv[1:] else main()
