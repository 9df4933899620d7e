#!/usr/bin/env python3
"""tools/make_clip_tower_golden.py -- tests/golden/clip_tower_*.npz and deepencoder_*.npz from the UNMODIFIED reference modules
(deepencoder/clip_sdpa.py, deepencoder/deepencoder_infer.py).

Runs only where the reference is mounted.  The reference files are imported by path; what they import and this machine lacks gets a
stub of this tool's own: `easydict` (an attribute dict), `nuscenes.nuscenes` (an empty NuScenes class) and the `deepencoder` parent
package (a bare namespace over the reference's directory, so its __init__ does not run).  Nothing that reaches the network is ever
called: not DeepEncoderRuntime.__init__, not download_sam_if_needed, not load_openclip_vitl14_into_vitmodel, not deepencoder_infer.

  clip_tower_<case>   per case of tests/clip_tower_cases.py (CASES, and DEEP: the 24-layer tower build_clip_l() ships): VitModel built
                      from the configuration, every parameter loaded strictly from clip_tower_cases.case_state, eval() under no_grad()
                      in fp32 -> `out` (the rows clip_tower_cases.kept_rows names), `rows`, and the state_dict's key list and shapes
  deepencoder_runtime a DeepEncoderRuntime made with object.__new__ whose sam / clip_vit / projector / device / dtype / grid / image_size
                      are set here (small SAM, CLIP of width 1024 and two layers, 2048 x 2048 projector, all seeded), and the unmodified
                      encode_image on a temporary PNG of clip_tower_cases.runtime_image() -> every fourth token row
  deepencoder_runtime_full   the same at the size DeepEncoderRuntime() builds: the reference's ImageEncoderViT at the ViT-B geometry
                      with the state of vision_tower_cases' `vit_b_1024` case, the 24-layer VitModel of DEEP, the same projector
  deepencoder_prep    resize_and_pad_to_square(im, target=64) and _pil_to_tensor_og_norm on a seeded 96 x 40 image

Every file is data only and stays under 1 MiB (asserted).  No weights and no reference code are stored.

    python tools/make_clip_tower_golden.py [case ... | runtime | runtime_full | prep]
"""
from __future__ import annotations

import importlib
import os
import sys
import tempfile
import types
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import clip_tower_cases as CC  # noqa: E402
import vision_tower_cases as VC  # noqa: E402
import make_goldens as MG  # noqa: E402


class _AttrDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None

    __setattr__ = dict.__setitem__


def install_stubs():
    ed = types.ModuleType("easydict")
    ed.EasyDict = _AttrDict
    sys.modules.setdefault("easydict", ed)
    nu, nn_ = types.ModuleType("nuscenes"), types.ModuleType("nuscenes.nuscenes")
    nn_.NuScenes = type("NuScenes", (), {})
    nu.nuscenes = nn_
    sys.modules.setdefault("nuscenes", nu)
    sys.modules.setdefault("nuscenes.nuscenes", nn_)
    pkg = types.ModuleType("deepencoder")
    pkg.__path__ = [os.path.join(MG.REF, "deepencoder")]
    sys.modules["deepencoder"] = pkg


def save(path, **arrays):
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 1024 * 1024, (path, size)
    return size


def key_lists(sd):
    return np.array(list(sd.keys())), np.array([",".join(str(d) for d in v.shape) for v in sd.values()])


def load_strict(m, seeded):
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded.items()}, strict=True)
    return m.eval()


@torch.no_grad()
def tower_case(clip, name):
    cfg = CC.case(name)[0]
    m = load_strict(clip.VitModel(_AttrDict(cfg)), CC.case_state(name))
    x, pe = CC.case_inputs(name)
    out = m(torch.from_numpy(x), None if pe is None else torch.from_numpy(pe)).numpy()
    rows = np.array(CC.kept_rows(name, out.shape[1]))
    keys, shapes = key_lists(m.state_dict())
    size = save(os.path.join(MG.OUT, CC.golden_name(name)), out=out[:, rows], rows=rows, full_shape=np.array(out.shape), keys=keys, shapes=shapes)
    print(f"  {name:10s} {list(out.shape)}  max {np.abs(out).max():.3f}  {size / 1024:.0f} KiB")


@torch.no_grad()
def runtime_case(clip, full=False):
    from PIL import Image
    di = importlib.import_module("deepencoder.deepencoder_infer")
    sam_mod = importlib.import_module("deepencoder.sam_vary_sdpa")
    rt = object.__new__(di.DeepEncoderRuntime)
    if full:                                             # what DeepEncoderRuntime() builds: SAM ViT-B and the 24-layer CLIP
        rt.sam = load_strict(sam_mod.ImageEncoderViT(**VC.VIT_B, qkv_bias=True, use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6)),
                             VC.case_state(CC.RUNTIME_FULL_SAM))
        rt.clip_vit = load_strict(clip.VitModel(_AttrDict(CC.DEEP[CC.RUNTIME_FULL_CLIP][0])), CC.case_state(CC.RUNTIME_FULL_CLIP))
    else:
        rt.sam = load_strict(sam_mod.ImageEncoderViT(**CC.RUNTIME_SAM, qkv_bias=True, use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6)),
                             VC.state(CC.RUNTIME_SAM, CC.RUNTIME_SEEDS["sam"]))
        rt.clip_vit = load_strict(clip.VitModel(_AttrDict(CC.WIDE)), CC.state(CC.WIDE, CC.RUNTIME_SEEDS["clip"]))
    rt.projector = load_strict(di.MlpProjector(di.EasyDict(projector_type="linear", input_dim=2048, n_embed=2048)), CC.projector_state())
    rt.device, rt.dtype, rt.grid, rt.image_size = "cpu", torch.float32, (di.FIXED_GRID_SIDE, di.FIXED_GRID_SIDE), di.FIXED_IMAGE_SIZE
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "view.png")
        Image.fromarray(CC.runtime_image()).save(path)
        res = rt.encode_image(path)
        x = di._pil_to_tensor_og_norm(di.resize_and_pad_to_square(Image.open(path)))
    assert torch.equal(x, CC.runtime_pixels())           # the resize is the identity at this size: the GPU test feeds the same pixels
    tok = res["tokens"].numpy()
    assert tok.shape == (256, 2048) and tuple(res["grid"]) == (16, 16) and res["image_size"] == 1024
    rows = np.arange(0, 256, CC.RUNTIME_ROW_STEP)
    size = save(os.path.join(MG.OUT, CC.RUNTIME_FULL_GOLDEN if full else "deepencoder_runtime.npz"), out=tok[rows], rows=rows, full_shape=np.array(tok.shape),
                result_keys=np.array(sorted(res)))
    print(f"  {'runtime_full' if full else 'runtime':12s} {list(tok.shape)}  max {np.abs(tok).max():.3f}  {size / 1024:.0f} KiB")


def prep_case():
    from PIL import Image
    di = importlib.import_module("deepencoder.deepencoder_infer")
    src = np.random.default_rng(65).integers(0, 256, size=(40, 96, 3), dtype=np.uint8)          # 96 wide, 40 high
    sq = di.resize_and_pad_to_square(Image.fromarray(src), target=64)
    size = save(os.path.join(MG.OUT, "deepencoder_prep.npz"), src=src, square=np.array(sq), tensor=di._pil_to_tensor_og_norm(sq).numpy())
    print(f"  prep       square {sq.size}  {size / 1024:.0f} KiB")


def main(names):
    torch.set_num_threads(8)
    install_stubs()
    clip = importlib.import_module("deepencoder.clip_sdpa")
    for name in names:
        if name in ("runtime", "runtime_full"):
            runtime_case(clip, full=name == "runtime_full")
        elif name == "prep":
            prep_case()
        else:
            tower_case(clip, name)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CC.CASES) + list(CC.DEEP) + ["runtime", "runtime_full", "prep"])
