"""deepencoder.DeepEncoderRuntime on the MI355X at a small SAM geometry (tests/clip_tower_cases.py: RUNTIME_SAM, a CLIP of width 1024 and
two layers, the 2048 x 2048 projector): encode_pixels against the golden of the unmodified reference's encode_image
(tests/golden/deepencoder_runtime.npz), encode_views on six temporary PNGs with two views missing, and InferenceEngine.process_vision
through a runtime.  bf16x3 at the parity bar 1e-3 max(1, max|ref|); plain bf16 at the bound of tests/test_gpu_clip_tower.py."""
import functools
import os
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_tower_cases as CC  # noqa: E402
import vision_tower_cases as VC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import clip_tower as CT, deepencoder as DE, engine, fusion, synth, vision_tower as VT  # noqa: E402

DEV = "cuda:0"
BAR = 1e-3
PLAIN_BOUND = 2 * 9.00e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel(out, ref):
    return float(np.abs(out - ref).max()) / max(1.0, float(np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def runtime():
    sam = VT.ImageEncoderViT(**CC.RUNTIME_SAM, qkv_bias=True, use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    sam.load_state_dict({k: t(v) for k, v in VC.state(CC.RUNTIME_SAM, CC.RUNTIME_SEEDS["sam"]).items()}, strict=True)
    clip = CT.VitModel(CT._Cfg(CC.WIDE))
    clip.load_state_dict({k: t(v) for k, v in CC.state(CC.WIDE, CC.RUNTIME_SEEDS["clip"]).items()}, strict=True)
    proj = fusion.MlpProjectorLinear(2048, 2048)
    proj.load_state_dict({k: t(v) for k, v in CC.projector_state().items()}, strict=True)
    return DE.DeepEncoderRuntime.from_modules(sam, clip, proj, device=DEV)


view_image = CC.view_image                               # view v: the runtime image with its 64 x 64 blocks rolled by v


def test_encode_pixels_reproduces_the_reference_runtime():
    g = np.load(os.path.join(GOLDEN, "deepencoder_runtime.npz"))
    rt = runtime()
    x = CC.runtime_pixels().to(DEV)
    for mode, bound in (("bf16x3", BAR), ("bf16", PLAIN_BOUND)):
        rt.precision = mode
        out = rt.encode_pixels(x)
        assert tuple(out.shape) == (1, 256, 2048) and out.dtype == torch.float32
        err = rel(out[0].cpu().numpy()[g["rows"]], g["out"])
        print(f"runtime {mode}: vs the reference's encode_image {err:.3e} (bound {bound:.1e}, max|golden| {np.abs(g['out']).max():.3f})")
        assert err <= bound, (mode, err)
    # the join against the existing torch-assembled form on the same towers: cat(clip[:, 1:], sam^T) -> projector
    rt.precision = "bf16x3"
    mine = rt.encode_pixels(x)                            # hands the mode to the three modules
    with torch.no_grad():
        feats = rt.sam(x)
        fused = fusion.deepencoder_fuse(rt.projector, rt.clip_vit(x, feats), feats)
    e = rel(mine.cpu().numpy(), fused.cpu().numpy())
    print(f"two half-K products vs cat + one K = 2048 product: {e:.3e}")
    assert e <= 2e-4


def test_encode_views_batches_the_present_views(tmp_path):
    from PIL import Image
    rt = runtime()
    paths = []
    for v in range(6):
        p = tmp_path / f"view{v}.png"
        if v not in (1, 4):
            Image.fromarray(view_image(v)).save(p)
        paths.append(p if v != 4 else None)
    with pytest.raises(FileNotFoundError):
        rt.encode_views(paths, strict=True)
    for mode, bound in (("bf16x3", BAR), ("bf16", PLAIN_BOUND)):
        rt.precision = mode
        res = rt.encode_views(paths, strict=False)
        assert sorted(res) == ["grid", "image_size", "present_mask", "tokens", "view_names"]
        assert res["present_mask"] == [True, False, True, True, False, True] and res["view_names"] == list(DE.DEFAULT_VIEW_ORDER)
        assert tuple(res["grid"]) == (16, 16) and res["image_size"] == 1024 and len(res["tokens"]) == 6
        for v, tok in enumerate(res["tokens"]):
            assert tuple(tok.shape) == (256, 2048) and tok.dtype == torch.float32
            if not res["present_mask"][v]:
                assert not bool(tok.any())
                continue
            x = DE._pil_to_tensor_og_norm(Image.fromarray(view_image(v))).to(DEV)
            alone = rt.encode_pixels(x)[0]
            e = rel(tok.cpu().numpy(), alone.cpu().numpy())
            print(f"{mode} view {v}: batched vs alone {e:.3e}")
            assert e <= bound, (mode, v, e)
        one = rt.encode_image(paths[0])
        assert sorted(one) == ["grid", "image_size", "tokens"] and torch.equal(one["tokens"], rt.encode_pixels(
            DE._pil_to_tensor_og_norm(Image.fromarray(view_image(0))).to(DEV))[0])
    assert rel(res["tokens"][0].cpu().numpy(), res["tokens"][2].cpu().numpy()) > 0.05      # the views differ


def test_engine_process_vision_through_the_runtime(tmp_path):
    from PIL import Image
    rt = runtime()
    rt.precision = "bf16x3"
    paths = []
    for v in range(6):
        p = tmp_path / f"cam{v}.png"
        if v != 3:
            Image.fromarray(view_image(v)).save(p)
        paths.append(p)
    va = synth.load_seeded(fusion.VisionAdapter(2048), 71).to(DEV).eval()
    vv = synth.load_seeded(fusion.VATVision(d_in=2048, d_model=128, n_input_tokens=6 * 256, compression_factor=8, n_layers=1, n_heads=32), 72).to(DEV).eval()
    eng = object.__new__(engine.InferenceEngine)          # process_vision reads these members only
    eng.use_vision, eng.multiview_tokens_fn, eng.runtime, eng.nusc, eng.device = True, None, rt, None, torch.device(DEV)
    eng.vat_vision, eng.vision_adapter = vv, va
    seen = []
    eng.view_paths_fn = lambda tok: (seen.append(tok), paths)[1]
    out = eng.process_vision("sample-7")
    assert seen == ["sample-7"]
    with torch.no_grad():
        want = vv(va(rt.encode_views(paths, strict=False)["tokens"])[None])
    assert tuple(out.shape) == (1, vv.n_queries, 128) and torch.equal(out, want)
    eng.runtime = None
    with pytest.raises(F.LvqError):
        eng.process_vision("sample-7")
    eng.multiview_tokens_fn = lambda tok: rt.encode_views(paths, strict=False)["tokens"]
    assert torch.equal(eng.process_vision("sample-7"), want)
