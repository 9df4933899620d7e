#!/usr/bin/env python3
"""tools/make_transfusion_head_golden.py -- tests/golden/transfusion_head_<case>.npz from the UNMODIFIED reference TransFusionHead
(pcdet/models/dense_heads/transfusion_head.py with model_utils/transfusion_utils.py and basic_block_2d.py).

Runs only where the reference is mounted (tools/make_goldens.py explains the pattern: empty parent packages are registered so that no
pcdet/**/__init__.py is executed; weights and inputs come from seeds).  What the generator's environment lacks is stubbed in sys.modules
before the import, as tools/make_anchor_head_golden.py does: `numba`, `easydict`, `SharedArray`, `spconv` (ref_standins.install_spconv) and the
compiled `iou3d_nms_cuda` / `roiaware_pool3d_cuda` extensions (the Hungarian assigner imports one; inference never calls it).  decode_bbox's
`.cuda()` runs inside ref_standins.cuda_is_identity().  No stand-in does arithmetic: every stored number is the reference's own.

Per case of transfusion_head_cases.MODULE_CASES the file keeps: `x`, `keys` / `shapes` (the reference class's state_dict; the values are
transfusion_head_cases.case_state(name), loaded with strict=True), `init_sums` (per key, the sum of what the
constructor drew after torch.manual_seed(0)), `dense_heatmap`, `query_labels`, `query_heatmap_score`, the five or six
res_layer tensors as predict() returns them (center with + query_pos, before get_bboxes rescales it in place) and
`final_<scene>_{boxes,scores,labels}`.  The reference's argsort is unstable among equal heats; the margin conditions keep the cut and every
decision near it clear of that (and tests match proposals by their (class, cell) key, not by position).

    python tools/make_transfusion_head_golden.py            # rewrites the fixtures, asserts the margin conditions
    python tools/make_transfusion_head_golden.py --search   # first input seed per case (from the case's xseed upwards) that meets them;
                                                             # restatement only, the reference is not needed

Printed on the last run (kept rows per scene; margins: cut gap, local-maximum margin, |score - thresh|, range distance; positive candidates):
    nusc   scene 0: 33 of 48   scene 1: 33 of 48   margins 6.19e-04 4.86e-03 4.28e-03 1.64e-02 1579   190 KiB
    waymo  scene 0: 32 of 32   scene 1: 32 of 32   margins 5.21e-04 4.23e-03 7.04e-02 9.15e+00 934   123 KiB
    plain  scene 0: 40 of 40   margins 7.25e-04 2.20e-03 9.35e-02 9.54e+00 81   67 KiB
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
import transfusion_head_cases as TC  # noqa: E402

REF = "/root/reference/src"
OUT = os.path.join(ROOT, "tests", "golden")


def fmt(m):
    return " ".join(f"{m[k]:.2e}" for k in TC.MARGINS) + f" {m['positive']}"


def search():
    for name, c in TC.MODULE_CASES.items():
        for seed in range(c["xseed"], c["xseed"] + 100000):
            m = TC.case_margins(name, seed)
            kept = TC.case_ref(name, seed)["keep"].sum(axis=1).tolist()
            TC.case_ref.cache_clear()
            mixed = name != "nusc" or all(0 < k < c["p"] for k in kept)          # nusc: the mask drops some rows and keeps some in each scene
            if TC.margins_ok(m, c["p"]) and mixed:
                print(name, "xseed", seed, "margins", fmt(m), "kept", kept, flush=True)
                break


def _stub(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


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
                 ("pcdet.models.model_utils", le + "/models/model_utils"), ("pcdet.utils", le + "/utils"), ("pcdet.ops", le + "/ops"),
                 ("pcdet.ops.iou3d_nms", le + "/ops/iou3d_nms"), ("pcdet.ops.roiaware_pool3d", le + "/ops/roiaware_pool3d")]:
        _stub(n, p)
    _stub("pcdet.ops.iou3d_nms.iou3d_nms_cuda")
    _stub("pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda")
    return importlib.import_module("pcdet.models.dense_heads.transfusion_head").TransFusionHead


@torch.no_grad()
def main():
    import ref_standins as RS
    torch.set_num_threads(8)
    cls = import_reference()
    for name, c in TC.MODULE_CASES.items():
        with RS.cuda_is_identity():
            torch.manual_seed(0)
            m = cls(**TC.case_args(name))
            sd = m.state_dict()
            init_sums = np.array([float(v.double().sum()) for v in sd.values()])      # the constructor's own draws: pins the RNG order
            TC.load_state(m, TC.case_state(name))
            m.eval()
            x = TC.case_input(name)
            res = m.predict(torch.from_numpy(x))
            store = dict(x=x, keys=np.array(list(sd.keys())), shapes=np.array([",".join(str(d) for d in v.shape) for v in sd.values()]),
                         query_labels=m.query_labels.numpy().astype(np.int64), init_sums=init_sums)
            for k, v in res.items():
                store[k] = v.clone().numpy()
            bboxes = m.get_bboxes(res)
        for s, d in enumerate(bboxes):
            store[f"final_{s}_boxes"] = d["pred_boxes"].numpy()
            store[f"final_{s}_scores"] = d["pred_scores"].numpy()
            store[f"final_{s}_labels"] = d["pred_labels"].numpy()
            assert d["pred_labels"].dtype == torch.int32
        mg = TC.case_margins(name)
        path = os.path.join(OUT, TC.golden_name(name))
        np.savez_compressed(path, **store)
        kept = "   ".join(f"scene {s}: {len(store[f'final_{s}_scores'])} of {c['p']}" for s in range(len(bboxes)))
        print(f"    {name:6s} {kept}   margins {fmt(mg)}   {os.path.getsize(path) / 1024:.0f} KiB")
        assert TC.margins_ok(mg, c["p"]), "a margin condition fails: run --search and move the case's xseed"
        assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    search() if "--search" in sys.argv[1:] else main()
