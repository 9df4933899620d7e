"""clip_tower.VitModel (the CLIP-L tower on liblvq_hip.so) against the goldens of the unmodified reference module
(tests/golden/clip_tower_*.npz) and the fp64 restatement of tests/clip_tower_cases.py; its sub-modules against the restatement.

bf16x3 (hi + lo operands) is held to the project's parity bar, 1e-3 max(1, max|ref|).  Plain bf16 is held to the bound
tests/test_gpu_vision_tower.py applies to that mode: twice the error that file records for the SAM tower on the MI355X -- PLAIN_BOUND
is twice the largest of its PLAIN_MEASURED values (9.00e-3), a figure of the same operand rounding through the same GEMM and attention
kernels at the same depth of two blocks, and not one taken from this tower's own output.  Every error is printed before it is asserted."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_tower_cases as CC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import clip_tower as CT  # noqa: E402

DEV = "cuda:0"
BAR = 1e-3
PLAIN_BOUND = 2 * 9.00e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def _model(cfg_key):
    name = "l2_w1024" if cfg_key == "wide" else "same"
    m = CT.VitModel(CT._Cfg(CC.CASES[name][0]))
    m.load_state_dict({k: t(v) for k, v in CC.case_state(name).items()}, strict=True)
    return m.to(DEV).eval().requires_grad_(False)


def model(name):
    return _model("wide" if name == "l2_w1024" else "base")


def inputs(name):
    x, pe = CC.case_inputs(name)
    return t(x).to(DEV), (None if pe is None else t(pe).to(DEV))


def run(m, mode, *args, **kw):
    m.precision = mode
    with torch.no_grad():
        return m(*args, **kw)


def rel(out, ref):
    return float(np.abs(out - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("name", list(CC.CASES))
def test_both_modes_reproduce_the_reference_module(name):
    g = np.load(os.path.join(GOLDEN, CC.golden_name(name)))
    want, rows = g["out"], g["rows"]
    ref = CC.case_ref(name)
    x, pe = inputs(name)
    m = model(name)
    out = run(m, "bf16x3", x, pe).cpu().numpy()
    assert list(out.shape) == list(g["full_shape"]) and out.dtype == np.float32
    err, err64 = rel(out[:, rows], want), rel(out, ref)
    print(f"{name} bf16x3: vs golden {err:.3e}, vs fp64 restatement {err64:.3e} (max|ref| {np.abs(want).max():.3f})")
    assert err <= BAR and err64 <= BAR, (err, err64)
    out1 = run(m, "bf16", x, pe).cpu().numpy()
    e1, e164 = rel(out1[:, rows], want), rel(out1, ref)
    print(f"{name} bf16: vs golden {e1:.3e}, vs fp64 restatement {e164:.3e} (bound {PLAIN_BOUND:.1e})")
    assert e1 <= PLAIN_BOUND and e164 <= PLAIN_BOUND, (e1, e164)
    assert err64 < e164


def test_keyword_form_and_batch_independence():
    x, pe = inputs("same")
    m = model("same")
    a = run(m, "bf16x3", x, pe)
    assert torch.equal(a, run(m, "bf16x3", pixel_values=x, patch_embeds=pe)) and torch.equal(a, run(m, "bf16x3", x=x, patch_embeds=pe))
    assert torch.equal(a, run(m, "bf16x3", x, patch_embeds=pe))
    for i in (0, 1):
        assert torch.equal(a[i:i + 1], run(m, "bf16x3", x[i:i + 1].contiguous(), pe[i:i + 1].contiguous()))
    xo, _ = inputs("own_patch")
    assert torch.equal(run(m, "bf16x3", pixel_values=xo), run(m, "bf16x3", xo, None))
    with pytest.raises(ValueError):
        run(m, "bf16x3", patch_embeds=pe)


def test_a_weight_update_in_place_is_seen_by_the_next_forward():
    name = "down"
    x, pe = inputs(name)
    m = CT.VitModel(CT._Cfg(CC.BASE))
    sd = {k: v.copy() for k, v in CC.case_state(name).items()}
    m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval().requires_grad_(False)
    first = run(m, "bf16x3", x, pe)
    assert rel(first.cpu().numpy(), CC.case_ref(name)) <= BAR
    touched = ("embeddings.class_embedding", "embeddings.position_embedding.weight", "transformer.layers.1.mlp.fc1.weight",
               "transformer.layers.0.self_attn.qkv_proj.weight", "pre_layrnorm.weight")
    with torch.no_grad():
        for k in touched:
            p = dict(m.named_parameters())[k]
            p.mul_(1.25)
            sd[k] = p.detach().cpu().numpy()
    second = run(m, "bf16x3", x, pe)
    ref2 = CC.vit(sd, CC.BASE, *CC.case_inputs(name)).numpy()
    e = rel(second.cpu().numpy(), ref2)
    moved = rel(second.cpu().numpy(), first.cpu().numpy())
    print(f"after the update: vs fp64 of the new weights {e:.3e}; moved by {moved:.3f}")
    assert e <= BAR and moved > 0.05


# ------------------------------------------------------------------------------------------------------------------------------------
# single modules against the fp64 restatement
# ------------------------------------------------------------------------------------------------------------------------------------
def hold(case, fn, ref):
    o3, o1 = fn("bf16x3").cpu().numpy(), fn("bf16").cpu().numpy()
    assert o3.shape == ref.shape and o3.dtype == np.float32
    e3, e1 = rel(o3, ref), rel(o1, ref)
    print(f"MODULE {case}: bf16x3 {e3:.3e} (bar {BAR:.0e}), bf16 {e1:.3e} (bound {PLAIN_BOUND:.1e}), max|ref| {np.abs(ref).max():.3f}")
    assert e3 <= BAR and e1 <= PLAIN_BOUND and e3 < e1, (case, e3, e1)


@pytest.mark.parametrize("s", [7, 65])
def test_modules_feed_forward_attention_block(s):
    """S = 7 (one partial key tile) and S = 65 (a second key tile of one key) on [2, S, 128] rows with a per-row offset."""
    m = model("same")
    sd, cfg = CC.case_state("same"), CC.BASE
    h = CC.synth.randn((2, s, 128), 170 + s) + np.linspace(-1, 1, s, dtype=np.float32)[None, :, None]
    hd, x = torch.from_numpy(h).double(), t(h).to(DEV)
    layer, p = m.transformer.layers[1], "transformer.layers.1."
    with torch.no_grad():
        hold(f"feed_forward S={s}", lambda mode: run(layer.mlp, mode, x), CC.feed_forward(sd, p + "mlp.", hd).numpy())
        hold(f"attention S={s}", lambda mode: run(layer.self_attn, mode, x), CC.attention(sd, p + "self_attn.", cfg, hd).numpy())
        hold(f"block S={s}", lambda mode: run(layer, mode, x), CC.block(sd, p, cfg, hd).numpy())
        ref = CC.block(sd, "transformer.layers.1.", cfg, CC.block(sd, "transformer.layers.0.", cfg, hd))
        hold(f"transformer S={s}", lambda mode: run(m.transformer, mode, x), ref.numpy())


@pytest.mark.parametrize("name", ["same", "down", "zeropad", "own_patch"])
def test_embeddings_with_pre_layrnorm(name):
    """VitModel.embed = pre_layrnorm(CLIPVisionEmbeddings): fp32 in, fp32 out -- with patch_embeds given no operand is rounded, so both
    modes agree bit for bit and sit at fp32 accuracy; the tower's own patch conv is a GEMM and carries the mode's operand rounding."""
    m = model(name)
    x, pe = inputs(name)
    ref = CC.embed(CC.case_state(name), CC.BASE, *CC.case_inputs(name)).numpy()
    m.precision = "bf16x3"
    with torch.no_grad():
        o3 = m.embed(x, pe)
        m.precision = "bf16"
        o1 = m.embed(x, pe)
    e3, e1 = rel(o3.cpu().numpy(), ref), rel(o1.cpu().numpy(), ref)
    print(f"MODULE embed {name}: bf16x3 {e3:.3e}, bf16 {e1:.3e}")
    if pe is not None:
        assert torch.equal(o3, o1) and e3 <= 1e-5, e3
    else:
        assert e3 <= BAR and e1 <= PLAIN_BOUND


def test_families_without_a_kernel_are_named():
    cfg = CT._Cfg(dict(CC.BASE, num_heads=4, num_attention_heads=4))                # head dim 32
    m = CT.VitModel(cfg).to(DEV).eval().requires_grad_(False)
    x, pe = inputs("same")
    with pytest.raises(F.LvqError, match="head dim"), torch.no_grad():
        m(x, pe)
    m = model("same")
    with pytest.raises(F.LvqError), torch.no_grad():
        m(x, pe.cpu())
    m.precision = "fp8"
    with pytest.raises(F.LvqError), torch.no_grad():
        m(x, pe)
    m.precision = None
    m.train()
    try:
        with pytest.raises(F.LvqError), torch.no_grad():
            m(x, pe)
    finally:
        m.eval()
