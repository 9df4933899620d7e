"""vision_tower.ImageEncoderViT (the SAM ViT image encoder on liblvq_hip.so, attention by csrc/vit_attention.hip) against the goldens of
the unmodified reference module (tests/golden/vision_tower_*.npz) and the fp64 restatement of tests/vision_tower_cases.py.

bf16x3 (hi + lo operands) is held to the project's parity bar, 1e-3 max(1, max|ref|).  The plain bf16 form has no bar known in advance:
PLAIN_MEASURED holds the error measured on the MI355X (against the restatement for the three small cases, against the golden for the
full geometry, whose restatement differs from its golden by 6e-6), and the test asserts twice that value as a regression guard, as
tests/test_gpu_backbone2d.py does."""
import functools
import os
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vision_tower_cases as VC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import vision_tower as VT  # noqa: E402

DEV = "cuda:0"
BAR = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = [n for n in VC.CASES if n != "vit_b_1024"]
# max |out - ref| / max(1, max|ref|) in the plain bf16 form, measured on the MI355X
PLAIN_MEASURED = {"pad": 7.46e-3, "w14": 6.80e-3, "resized": 6.80e-3, "vit_b_1024": 9.00e-3}     # (bf16x3: 1.29e-5, 1.24e-5, 1.39e-5, 1.74e-5)
DENSE_BIAS_BYTES = 12 * 4096 * 4096 * 4            # ONE dense fp32 bias array of one global block of SAM-B: 805 306 368


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def _model(name):
    m = VT.build_sam_vit_b() if name == "vit_b_1024" else \
        VT.ImageEncoderViT(**VC.CASES[name][0], qkv_bias=True, use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    m.load_state_dict({k: t(v) for k, v in VC.case_state(name).items()}, strict=True)
    return m.to(DEV).eval()


def model(name):
    return _model("pad" if name == "resized" else name)         # one model, two input sizes


def run(m, x, mode):
    m.precision = mode
    with torch.no_grad():
        return m(x if torch.is_tensor(x) else t(x).to(DEV))


def rel(out, ref):
    return float(np.abs(out - ref).max()) / max(1.0, float(np.abs(ref).max()))


def golden(name):
    return np.load(os.path.join(GOLDEN, VC.golden_name(name)))["out"]


@pytest.mark.parametrize("name", SMALL)
def test_bf16x3_reproduces_the_reference_module(name):
    want, ref = golden(name), VC.case_ref(name)
    out = run(model(name), VC.case_input(name), "bf16x3").cpu().numpy()
    assert out.shape == want.shape and out.dtype == np.float32
    err, err64 = rel(out, want), rel(out, ref)
    print(f"{name} bf16x3: vs golden {err:.3e}, vs fp64 restatement {err64:.3e} (max|ref| {np.abs(want).max():.3f})")
    assert err <= BAR and err64 <= BAR, (err, err64)


@pytest.mark.parametrize("name", SMALL)
def test_plain_bf16_regression_guard(name):
    ref = VC.case_ref(name)
    err = rel(run(model(name), VC.case_input(name), "bf16").cpu().numpy(), ref)
    print(f"{name} bf16: vs fp64 restatement {err:.3e} (max|ref| {np.abs(ref).max():.3f})")
    assert err <= 2 * PLAIN_MEASURED[name], err


def test_full_geometry_both_modes_and_peak_memory():
    """build_sam_vit_b() at 1024 x 1024 against its golden: bf16x3 at the parity bar, plain bf16 at its regression guard, and the
    memory condition -- after a warm-up forward (weights packed and cached) a second forward raises max_memory_allocated by less than ONE
    dense [12, 4096, 4096] fp32 bias array, which the reference materialises per global block."""
    name = "vit_b_1024"
    want = golden(name)
    m, x = model(name), t(VC.case_input(name)).to(DEV)
    out = run(m, x, "bf16x3").cpu().numpy()
    assert out.shape == want.shape == (1, 1024, 16, 16) and out.dtype == np.float32
    err = rel(out, want)
    print(f"{name} bf16x3: vs golden {err:.3e} (max|ref| {np.abs(want).max():.3f})")
    assert err <= BAR, err
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out2 = run(m, x, "bf16x3")
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"{name}: second forward raises max_memory_allocated by {rise / 2 ** 20:.1f} MiB (one dense bias array: {DENSE_BIAS_BYTES / 2 ** 20:.0f} MiB)")
    assert rise < DENSE_BIAS_BYTES
    assert np.array_equal(out2.cpu().numpy(), out)
    errp = rel(run(m, x, "bf16").cpu().numpy(), want)
    print(f"{name} bf16: vs golden {errp:.3e}")
    assert errp <= 2 * PLAIN_MEASURED[name], errp


def test_state_dict_round_trip_and_checkpoint_prefixes(tmp_path):
    """build_sam_vit_b()'s state_dict loads back strictly, and the three checkpoint key layouts of the reference's builder load from a file:
    "image_encoder." (official SAM, other modules' keys beside it), "vision_tower_high." (strict) and bare keys -- on a two-block geometry
    of the same builder, so that the files stay small."""
    sd = {k: v.detach().cpu() for k, v in model("vit_b_1024").state_dict().items()}
    fresh = VT.build_sam_vit_b()
    assert list(fresh.state_dict()) == list(sd)
    fresh.load_state_dict(sd, strict=True)
    assert torch.equal(fresh.blocks[11].attn.rel_pos_h, sd["blocks.11.attn.rel_pos_h"])
    geo = dict(encoder_embed_dim=128, encoder_depth=2, encoder_num_heads=2, encoder_global_attn_indexes=[1])
    torch.manual_seed(3)
    small = {k: torch.randn_like(v) for k, v in VT._build_sam(**geo).state_dict().items()}
    for prefix in ("image_encoder.", "vision_tower_high.", ""):
        path = os.path.join(tmp_path, f"ckpt_{len(prefix)}.pth")
        extra = {"mask_decoder.x": torch.zeros(1)} if prefix == "image_encoder." else {}
        torch.save({**{prefix + k: v for k, v in small.items()}, **extra}, path)
        got = VT._build_sam(**geo, checkpoint=path).state_dict()
        assert list(got) == list(small) and all(torch.equal(got[k], small[k]) for k in small)
    with pytest.raises(FileNotFoundError):
        VT.build_sam_vit_b(checkpoint=os.path.join(tmp_path, "missing.pth"))


def test_modes_inputs_and_batching():
    m = model("pad")
    x = t(VC.case_input("pad")).to(DEV)
    with pytest.raises(F.LvqError), torch.no_grad():
        m(x.cpu())                                                              # CPU input: no fallback
    m.train()
    try:
        with pytest.raises(F.LvqError), torch.no_grad():
            m(x)                                                                # train() mode
    finally:
        m.eval()
    with pytest.raises(F.LvqError):
        m(x)                                                                    # gradients in reach
    m.precision = "fp8"
    with pytest.raises(F.LvqError), torch.no_grad():
        m(x)
    for mode in VT.MODES:                                                       # a batch of 2 equals two batches of 1 bit for bit
        both = run(m, x, mode)
        assert torch.equal(both[0:1], run(m, x[0:1].contiguous(), mode)) and torch.equal(both[1:2], run(m, x[1:2].contiguous(), mode))


def test_families_without_a_kernel_are_named():
    x = torch.zeros(1, 3, 64, 64, device=DEV)
    kw = dict(img_size=64, patch_size=16, embed_dim=128, depth=1, out_chans=256)
    with pytest.raises(F.LvqError, match="kernel family"), torch.no_grad():
        VT.ImageEncoderViT(**kw, num_heads=2, use_rel_pos=False).to(DEV).eval()(x)
    with pytest.raises(F.LvqError, match="kernel family"), torch.no_grad():
        VT.ImageEncoderViT(**kw, num_heads=4, use_rel_pos=True).to(DEV).eval()(x)       # head dim 32
