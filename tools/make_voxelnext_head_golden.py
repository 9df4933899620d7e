#!/usr/bin/env python3
"""tools/make_voxelnext_head_golden.py -- tests/golden/voxelnext_head_<case>.npz from the UNMODIFIED reference VoxelNeXtHead
(pcdet/models/dense_heads/voxelnext_head.py:13-559) and centernet_utils.decode_bbox_from_voxels_nuscenes (centernet_utils.py:243-354).

Runs only where the reference is mounted.  The reference class runs on tools/ref_standins.install_spconv(): its dense-form SubMConv2d
pins the reference's WIRING (which layers, kernel, padding, bias, order, state_dict keys), as that file's docstring explains.  What the
generator's environment lacks is stubbed as in tools/make_center_head_golden.py (whose import_reference stubs are reused): `numba`,
`easydict`, `SharedArray`, the two compiled extensions, and `iou3d_nms_cuda.nms_gpu` as the greedy walk over the fp64 IoU.  `.cuda()` runs
inside ref_standins.cuda_is_identity().  Every scene of every case has n_b >= K rows, where the reference's class = ind // K is the
matrix row (tests/voxelnext_head_cases.py: decode_ref).

Per case of voxelnext_head_cases.CASES the file keeps: `feats` / `indices` (the input rows), `keys` / `shapes` (the reference class's
state_dict; the values are voxelnext_head_cases.case_state(name), loaded with strict=True), `rng_next` (torch.rand(1) drawn right after
the reference's constructor under torch.manual_seed(0)), `rows_<task>_<branch>` (the raw branch outputs), `pre_<task>_<scene>_{boxes,
scores,labels}` and `final_<scene>_{boxes,scores,labels}`.

    python tools/make_voxelnext_head_golden.py            # rewrites the fixtures, asserts the margin conditions
    python tools/make_voxelnext_head_golden.py --search   # first input seed per case (from the case's xseed upwards) that meets them;
                                                           # restatement only, the reference is not needed

Margin conditions: center_head's MARGINS (K-th gap, |score - 0.1|, |iou - 0.2|, |centre - limit|), n_b >= K in every scene, NMS removes
at least one candidate, at least one candidate falls to the limit range.

Printed on the last run (survivors before NMS -> kept, per scene; margins as above; candidates lost to the limit range):
    nusc     scene 0: 172 -> 165   scene 1: 169 -> 165   margins 1.25e-03 4.26e-01 2.11e-02 1.61e-02   limit 43   259 KiB
    k3       scene 0: 93 -> 69   scene 1: 86 -> 72   margins 2.51e-03 4.10e-01 2.33e-02 3.22e-02   limit 13   241 KiB
    nc1      scene 0: 30 -> 28   scene 1: 29 -> 24   margins 3.58e-03 4.95e-01 5.19e-02 4.23e-01   limit 5   143 KiB
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_center_head_golden as MC  # noqa: E402
import voxelnext_head_cases as VC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def conditions(name, cfg, pre, near, removed):
    c = VC.CASES[name]
    m = VC.module_margins(cfg, pre, near)
    drops = VC.limit_drops(cfg, pre)
    ok = MC.margins_ok(m) and removed >= 1 and drops >= 1 and all(d["n_b"] >= c["k"] for task in pre for d in task)
    return ok, m, drops


def search():
    for name, c in VC.CASES.items():
        cfg = VC.case_cfg(name)
        for seed in range(c["xseed"], c["xseed"] + 100000):
            _, pre, final, near, removed = VC.case_eval(name, seed)
            ok, m, drops = conditions(name, cfg, pre, near, removed)
            if ok:
                print(name, "xseed", seed, "margins", " ".join(f"{v:.2e}" for v in m), "kept", [len(f["pred_scores"]) for f in final],
                      "pre", [sum(len(t[s]["scores"]) for t in pre) for s in range(len(final))], "removed", removed, "limit", drops)
                break


def import_reference():
    import ref_standins as RS
    RS.install_spconv()
    MC.import_reference()                                   # the stubs, the package skeleton and centernet_utils
    head = importlib.import_module("pcdet.models.dense_heads.voxelnext_head")
    return head.VoxelNeXtHead, importlib.import_module("pcdet.models.model_utils.centernet_utils"), sys.modules["spconv.pytorch"]


@torch.no_grad()
def main():
    import ref_standins as RS
    torch.set_num_threads(8)
    cls, cu, spconv = import_reference()
    for name, c in VC.CASES.items():
        cfg = VC.case_cfg(name)
        with RS.cuda_is_identity():
            torch.manual_seed(0)
            m = cls(cfg, VC.C, len(c["class_names"]), c["class_names"], np.array(c["grid_size"]), c["point_cloud_range"], c["voxel_size"],
                    predict_boxes_when_training=False)
            rng_next = torch.rand(1).numpy()
            sd = m.state_dict()
            seeded = VC.case_state(name)
            m.load_state_dict({k: torch.from_numpy(np.asarray(seeded[k])).to(v.dtype).reshape(v.shape) for k, v in sd.items()}, strict=True)
            m.eval()
            feats, idx = VC.case_input(name)
            x = spconv.SparseConvTensor(torch.from_numpy(feats), torch.from_numpy(idx), list(c["grid"]), 2)
            out = m(dict(encoded_spconv_tensor=x, batch_size=2))
            post = cfg.POST_PROCESSING
            store = dict(feats=feats, indices=idx, rng_next=rng_next, keys=np.array(list(sd.keys())),
                         shapes=np.array([",".join(str(d) for d in v.shape) for v in sd.values()]))
            for i, pd in enumerate(m.forward_ret_dict["pred_dicts"]):
                for n, v in pd.items():
                    store[f"rows_{i}_{n}"] = v.numpy()
                pre = cu.decode_bbox_from_voxels_nuscenes(
                    batch_size=2, indices=torch.from_numpy(idx), obj=pd["hm"].sigmoid(), rot_cos=pd["rot"][:, 0].unsqueeze(dim=1),
                    rot_sin=pd["rot"][:, 1].unsqueeze(dim=1), center=pd["center"], center_z=pd["center_z"], dim=pd["dim"].exp(),
                    vel=pd["vel"] if "vel" in pd else None, iou=None, point_cloud_range=m.point_cloud_range, voxel_size=m.voxel_size,
                    feature_map_stride=m.feature_map_stride, K=post.MAX_OBJ_PER_SAMPLE, score_thresh=post.SCORE_THRESH,
                    post_center_limit_range=torch.tensor(post.POST_CENTER_LIMIT_RANGE).float())
                for s, d in enumerate(pre):
                    store[f"pre_{i}_{s}_boxes"] = d["pred_boxes"].numpy()
                    store[f"pre_{i}_{s}_scores"] = d["pred_scores"].numpy()
                    store[f"pre_{i}_{s}_labels"] = d["pred_labels"].numpy().astype(np.int64)          # class ids inside the task, unmapped
            for s, d in enumerate(out["final_box_dicts"]):
                store[f"final_{s}_boxes"] = d["pred_boxes"].numpy()
                store[f"final_{s}_scores"] = d["pred_scores"].numpy()
                store[f"final_{s}_labels"] = d["pred_labels"].numpy().astype(np.int64)
                assert all(v is None for v in d["pred_ious"]) and len(d["pred_ious"]) == len(cfg.CLASS_NAMES_EACH_HEAD)
        rows = [{n: store[f"rows_{i}_{n}"] for n in VC.branch_names(cfg)} for i in range(len(cfg.CLASS_NAMES_EACH_HEAD))]
        pre, final, near, removed = VC.head_final(cfg, c["class_names"], rows, idx, 2, c["stride"], c["voxel_size"], c["point_cloud_range"])
        ok, mg, drops = conditions(name, cfg, pre, near, removed)
        path = os.path.join(OUT, VC.golden_name(name))
        np.savez_compressed(path, **store)
        counts = "   ".join(f"scene {s}: {sum(len(t[s]['scores']) for t in pre)} -> {len(store[f'final_{s}_scores'])}" for s in range(2))
        print(f"    {name:8s} {counts}   margins {' '.join(f'{v:.2e}' for v in mg)}   limit {drops}   {os.path.getsize(path) / 1024:.0f} KiB")
        assert ok, "a margin condition fails on the reference's rows: run --search and move the case's xseed"
        assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    search() if "--search" in sys.argv[1:] else main()
