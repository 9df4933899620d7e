#!/usr/bin/env python3
"""tools/make_anchor_head_golden.py -- tests/golden/anchor_head_<case>.npz from the UNMODIFIED reference AnchorHeadSingle
(pcdet/models/dense_heads/anchor_head_single.py, anchor_head_template.py) and Detector3DTemplate.post_processing
(pcdet/models/detectors/detector3d_template.py:178-283).

Runs only where the reference is mounted (tools/make_goldens.py explains the pattern: empty parent packages are registered so that no
pcdet/**/__init__.py is executed; weights and inputs come from seeds).  What the generator's environment lacks is stubbed in sys.modules
before the import, as tools/make_center_head_golden.py does: `numba`, `easydict`, `SharedArray`, `spconv` (ref_standins.install_spconv), the
compiled `iou3d_nms_cuda` / `roiaware_pool3d_cuda` extensions and the detector template's sibling packages (backbones, roi heads), which the
post-processing never touches.  The constructor's `.cuda()` calls run inside ref_standins.cuda_is_identity().  post_processing is called as
an unbound function on a stand-in `self` that carries model_cfg, num_class and a generate_recall_record returning its recall_dict.

What the fixtures pin, and what they do not: exactly what DESIGN says of the CenterHead fixtures.  The dense outputs come from the
reference's code with no stand-in; the ONE stand-in that does arithmetic is `iou3d_nms_cuda.nms_gpu`, a greedy walk over the fp64
rectangle-clipping IoU of tests/center_head_cases.py, so the final lists pin the reference's WIRING around that call (the inclusive score
mask, torch.topk, the pre- and post-NMS cuts, the index mapping back, labels + 1) and not the rounding of the CUDA kernel.

Per case of anchor_head_cases.MODULE_CASES the file keeps: `x`, `keys` / `shapes` (the reference class's state_dict; the values are
anchor_head_cases.case_state(name), loaded with strict=True), `anchors` (the concatenated flat view), `batch_cls_preds`, `batch_box_preds`
and `final_<scene>_{boxes,scores,labels}`.

    python tools/make_anchor_head_golden.py            # rewrites the fixtures, asserts the margin conditions
    python tools/make_anchor_head_golden.py --search   # first input seed per case (from the case's xseed upwards) that meets them;
                                                        # restatement only, the reference is not needed

Printed on the last run (survivors -> selected -> kept per scene; margins: |score - thresh|, cut gap, |iou - thresh|, cluster gap, heading):
    kitti    scene 0: 37 -> 37 -> 37   scene 1: 31 -> 31 -> 30   margins 2.99e-03 inf 2.87e-01 8.90e-01 2.45e-02   351 KiB
    wide     scene 0: 1535 -> 1400 -> 764   scene 1: 1535 -> 1400 -> 765   margins 7.96e-03 2.64e-03 8.62e-02 2.91e-04 2.37e-01   388 KiB
    nodir    scene 0: 768 -> 768 -> 40   scene 1: 768 -> 768 -> 40   margins inf 5.78e-03 1.90e-01 2.84e-04 inf   228 KiB
(x alone is 192 KiB of seeded fp32 noise, the dense boxes of 2304 anchors 126 KiB: the two three-class fixtures end above the CenterHead ones.)
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

import anchor_head_cases as AC  # noqa: E402
import center_head_cases as CC  # noqa: E402

REF = "/root/reference/src"
OUT = os.path.join(ROOT, "tests", "golden")


def fmt(m):
    return " ".join(f"{m[k]:.2e}" for k in AC.MARGINS)


def search():
    for name, c in AC.MODULE_CASES.items():
        for seed in range(c["xseed"], c["xseed"] + 100000):
            _, dec, final = AC.case_ref(name, seed)
            m = AC.module_margins(dec, final, AC.case_post(name))
            AC.case_ref.cache_clear()
            if AC.margins_ok(m):
                print(name, "xseed", seed, "margins", fmt(m), "survivors", [f["survivors"] for f in final], "final",
                      [len(f["index"]) for f in final], flush=True)
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
    import ref_standins as RS

    def jit(*args, **kwargs):
        return args[0] if len(args) == 1 and callable(args[0]) and not kwargs else (lambda f: f)

    _stub("numba", jit=jit, njit=jit)
    _stub("easydict", EasyDict=CC.Cfg)
    _stub("SharedArray")
    RS.install_spconv()
    le = os.path.join(REF, "lidar-encoder", "pcdet")
    for n, p in [("pcdet", le), ("pcdet.models", le + "/models"), ("pcdet.models.dense_heads", le + "/models/dense_heads"),
                 ("pcdet.models.dense_heads.target_assigner", le + "/models/dense_heads/target_assigner"),
                 ("pcdet.models.detectors", le + "/models/detectors"), ("pcdet.models.model_utils", le + "/models/model_utils"),
                 ("pcdet.utils", le + "/utils"), ("pcdet.ops", le + "/ops"), ("pcdet.ops.iou3d_nms", le + "/ops/iou3d_nms"),
                 ("pcdet.ops.roiaware_pool3d", le + "/ops/roiaware_pool3d")]:
        _stub(n, p)
    _stub("pcdet.ops.iou3d_nms.iou3d_nms_cuda", nms_gpu=nms_gpu_standin)
    _stub("pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda")
    # the detector template's siblings: imported by name at its top, never used by post_processing
    _stub("pcdet.models.backbones_2d", map_to_bev=_stub("pcdet.models.backbones_2d.map_to_bev"))
    _stub("pcdet.models.backbones_3d", pfe=_stub("pcdet.models.backbones_3d.pfe"), vfe=_stub("pcdet.models.backbones_3d.vfe"))
    _stub("pcdet.models.roi_heads")
    head = importlib.import_module("pcdet.models.dense_heads.anchor_head_single")
    det = importlib.import_module("pcdet.models.detectors.detector3d_template")
    return head.AnchorHeadSingle, det.Detector3DTemplate


@torch.no_grad()
def main():
    import ref_standins as RS
    torch.set_num_threads(8)
    cls, det = import_reference()
    for name, c in AC.MODULE_CASES.items():
        cfg, post = AC.case_cfg(name), AC.case_post(name)
        with RS.cuda_is_identity():
            m = cls(cfg, c["shape"][1], len(c["class_names"]), c["class_names"], np.array(c["grid_size"]), np.array(c["point_cloud_range"]),
                    predict_boxes_when_training=False)
            sd = m.state_dict()
            seeded = AC.case_state(name)
            m.load_state_dict({k: torch.from_numpy(np.asarray(seeded[k])).to(v.dtype).reshape(v.shape) for k, v in sd.items()}, strict=True)
            m.eval()
            x = AC.case_input(name)
            out = m(dict(spatial_features_2d=torch.from_numpy(x), batch_size=x.shape[0]))
            stand_in = types.SimpleNamespace(model_cfg=AC.Cfg(POST_PROCESSING=post), num_class=len(c["class_names"]),
                                             generate_recall_record=lambda box_preds, recall_dict, **kw: recall_dict)
            pred_dicts, _ = det.post_processing(stand_in, out)
        store = dict(x=x, keys=np.array(list(sd.keys())), shapes=np.array([",".join(str(d) for d in v.shape) for v in sd.values()]),
                     anchors=torch.cat(m.anchors, dim=-3).reshape(-1, 7).numpy(), batch_cls_preds=out["batch_cls_preds"].numpy(),
                     batch_box_preds=out["batch_box_preds"].numpy())
        for s, d in enumerate(pred_dicts):
            store[f"final_{s}_boxes"] = d["pred_boxes"].numpy()
            store[f"final_{s}_scores"] = d["pred_scores"].numpy()
            store[f"final_{s}_labels"] = d["pred_labels"].numpy().astype(np.int64)
        _, dec, final = AC.case_ref(name)
        mg = AC.module_margins(dec, final, post)
        path = os.path.join(OUT, AC.golden_name(name))
        np.savez_compressed(path, **store)
        counts = "   ".join(f"scene {s}: {f['survivors']} -> {len(f['sel'])} -> {len(store[f'final_{s}_scores'])}" for s, f in enumerate(final))
        print(f"    {name:8s} {counts}   margins {fmt(mg)}   {os.path.getsize(path) / 1024:.0f} KiB")
        assert AC.margins_ok(mg), "a margin condition fails: run --search and move the case's xseed"
        assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    search() if "--search" in sys.argv[1:] else main()
