#!/usr/bin/env python3
"""tools/make_vision_tower_golden.py -- tests/golden/vision_tower_*.npz from the UNMODIFIED reference image encoder
(deepencoder/sam_vary_sdpa.py:100-511).

Runs only where the reference is mounted.  The module is imported by file path (it needs torch alone), so nothing of its package is
executed.  Per case of tests/vision_tower_cases.py: ImageEncoderViT is built from the configuration (the three small cases with
norm_layer = LayerNorm(eps 1e-6), use_rel_pos, qkv_bias, as build_sam_vit_b sets them; `vit_b_1024` through build_sam_vit_b()), every
parameter is loaded strictly from vision_tower_cases.case_state (synth.seeded_array per key; rel-pos tables ~ N(0, 0.25^2), pos_embed ~
N(0, 0.5^2)), the module runs in eval() under no_grad() on the seeded input in fp32, and the file keeps `out` with the state_dict's key
list and shapes.  No weights and no reference code are stored.

Printed on the last run (output shape, max|out|, size of the file):
    pad          [2, 1024, 3, 3]    max 3.602   68 KiB
    w14          [1, 1024, 5, 5]    max 4.023   94 KiB
    resized      [2, 1024, 2, 2]    max 3.496   31 KiB
    vit_b_1024   [1, 1024, 16, 16]  max 4.821  950 KiB

    python tools/make_vision_tower_golden.py [case ...]
"""
from __future__ import annotations

import importlib.util
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import vision_tower_cases as VC  # noqa: E402
import make_goldens as MG  # noqa: E402


def import_reference():
    spec = importlib.util.spec_from_file_location("ref_sam_vary_sdpa", os.path.join(MG.REF, "deepencoder", "sam_vary_sdpa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@torch.no_grad()
def main(names):
    torch.set_num_threads(8)
    ref = import_reference()
    for name in names:
        cfg, shape, _, _ = VC.CASES[name]
        if name == "vit_b_1024":
            m = ref.build_sam_vit_b()
        else:
            m = ref.ImageEncoderViT(**cfg, qkv_bias=True, use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
        sd = m.state_dict()
        seeded = VC.case_state(name)                 # keyed and shaped from the configuration alone: strict loading checks both
        m.load_state_dict({k: torch.from_numpy(seeded[k]) for k in seeded}, strict=True)
        m.eval()
        out = m(torch.from_numpy(VC.case_input(name))).numpy()
        assert out.shape[:2] == (shape[0], 1024) and out.dtype == np.float32
        keys = np.array(list(sd.keys()))
        shapes = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        path = os.path.join(MG.OUT, VC.golden_name(name))
        np.savez_compressed(path, out=out, keys=keys, shapes=shapes)
        print(f"  {name:12s} {list(out.shape)}  max {np.abs(out).max():.3f}  {os.path.getsize(path) / 1024:.0f} KiB")
        assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main(sys.argv[1:] or list(VC.CASES))
