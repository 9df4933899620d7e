"""The fp64 restatement of tests/vision_tower_cases.py against the goldens of the unmodified reference image encoder
(tests/golden/vision_tower_*.npz, tools/make_vision_tower_golden.py), the parameter layout of vision_tower.ImageEncoderViT against the key
list the goldens record, the sensitivity of the fixtures to every term a kernel could drop, and the host-only entry points of the fused
relative-position attention.  No GPU.

Bar: 2e-5 max(1, max|ref|), the one tests/test_bev_backbone_restatements.py holds fp64 restatements to against fp32-torch goldens."""
import ctypes
import os
from functools import partial

import numpy as np
import pytest
import torch

import vision_tower_cases as VC
from lidar_vision_vqa_amd import _ffi
from lidar_vision_vqa_amd import vision_tower as VT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 2e-5
GPU_BAR = 1e-3
SMALL = [n for n in VC.CASES if n != "vit_b_1024"]


def golden(name):
    return np.load(os.path.join(GOLDEN, VC.golden_name(name)))


def build(name):
    cfg = VC.CASES[name][0]
    if name == "vit_b_1024":
        return VT.build_sam_vit_b()
    return VT.ImageEncoderViT(**cfg, qkv_bias=True, use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))


@pytest.mark.parametrize("name", list(VC.CASES))
def test_restatement_agrees_with_the_reference_module(name):
    want = golden(name)["out"]
    ref = VC.case_ref(name)
    assert ref.shape == want.shape and want.dtype == np.float32
    mag = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(ref - want).max())
    print(f"{name}: restatement vs golden {err:.3e} (bar {BAR * mag:.3e}, max|ref| {mag:.3f})")
    assert err <= BAR * mag
    assert mag > 1.0


def test_restatement_forms_its_bias_from_shifted_tables():
    """bias_terms reads reversed windows of T = q [Rh; Rw]^T (shapes [.., gh] and [.., gw] per query); it agrees with the dense gather
    Rh[y - ky + gh - 1] . q written out here on a non-square grid, where a swap of the two axes would show."""
    gh, gw, dh = 3, 5, 8
    rng = np.random.default_rng(5)
    q = torch.from_numpy(rng.standard_normal((2, 1, gh * gw, dh)))
    rh, rw = torch.from_numpy(rng.standard_normal((2 * gh - 1, dh))), torch.from_numpy(rng.standard_normal((2 * gw - 1, dh)))
    bh, bw = VC.bias_terms(q, rh, rw, gh, gw)
    assert tuple(bh.shape) == (2, 1, gh, gw, gh) and tuple(bw.shape) == (2, 1, gh, gw, gw)
    ys, xs = np.arange(gh), np.arange(gw)
    dense_h = torch.einsum("bnyxc,ykc->bnyxk", q.view(2, 1, gh, gw, dh), rh[ys[:, None] - ys[None, :] + gh - 1])
    dense_w = torch.einsum("bnyxc,xkc->bnyxk", q.view(2, 1, gh, gw, dh), rw[xs[:, None] - xs[None, :] + gw - 1])
    assert float((bh - dense_h).abs().max()) < 1e-12 and float((bw - dense_w).abs().max()) < 1e-12
    d = VC.dense_bias(q.numpy(), rh.numpy(), rw.numpy(), gh, gw)
    assert d.shape == (2, 1, gh * gw, gh * gw)
    assert abs(d[1, 0, 1 * gw + 2, 2 * gw + 4] - float(q[1, 0, gw + 2] @ (rh[1 - 2 + gh - 1] + rw[2 - 4 + gw - 1]))) < 1e-12


@pytest.mark.parametrize("name", list(VC.CASES))
def test_state_dict_keys_order_and_shapes_are_the_reference_s(name):
    g = golden(name)
    want = [(str(k), tuple(int(d) for d in str(s).split(",") if d)) for k, s in zip(g["keys"], g["shapes"])]
    m = build(name)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want                                                          # same keys, same order, same shapes
    assert got == [(k, tuple(s)) for k, s in VC.state_shapes(VC.CASES[name][0])]
    if name != "vit_b_1024":                                                    # (seeding 95.6 M parameters again would only cost time)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in VC.case_state(name).items()}, strict=True)


def test_default_init_consumes_the_rng_in_torch_s_order():
    """The containers are built in the reference's order: patch_embed.proj, then per block attn.qkv, attn.proj, mlp.lin1, mlp.lin2, then
    the neck convs, net_2, net_3; pos_embed and the rel-pos tables start at zero and take nothing from the generator."""
    import torch.nn as nn
    torch.manual_seed(11)
    ours = build("pad")
    torch.manual_seed(11)
    pe = nn.Conv2d(3, 128, kernel_size=(16, 16), stride=(16, 16), padding=(0, 0))
    qkv, proj, lin1, lin2 = nn.Linear(128, 384), nn.Linear(128, 128), nn.Linear(128, 512), nn.Linear(512, 128)
    assert torch.equal(ours.patch_embed.proj.weight, pe.weight) and torch.equal(ours.patch_embed.proj.bias, pe.bias)
    b0 = ours.blocks[0]
    assert torch.equal(b0.attn.qkv.weight, qkv.weight) and torch.equal(b0.attn.proj.weight, proj.weight)
    assert torch.equal(b0.mlp.lin1.weight, lin1.weight) and torch.equal(b0.mlp.lin2.bias, lin2.bias)
    assert float(ours.pos_embed.detach().abs().max()) == 0.0 and float(b0.attn.rel_pos_h.detach().abs().max()) == 0.0
    assert tuple(b0.attn.rel_pos_h.shape) == (7, 64) and tuple(ours.blocks[1].attn.rel_pos_w.shape) == (19, 64)
    assert b0.window_size == 4 and ours.blocks[1].window_size == 0 and b0.norm1.eps == 1e-6


def test_module_refuses_what_has_no_kernel():
    with pytest.raises(_ffi.LvqError):                                          # CPU tensors: no fallback
        with torch.no_grad():
            build("pad").eval()(torch.zeros(1, 3, 160, 160))
    with pytest.raises(_ffi.LvqError):                                          # train() mode
        build("pad")(torch.zeros(1, 3, 160, 160))


@pytest.mark.parametrize("variant", ["no_rel", "swap", "mask_pad", "no_pos"])
@pytest.mark.parametrize("name", SMALL)
def test_fixtures_notice_every_term(name, variant):
    """A restatement without the term differs from the golden by at least 100 x the GPU bar, so no kernel that ignores it can pass.
    (`resized` has an 8 x 8 grid and windows of 4: nothing is padded there, so masking pad keys changes nothing and is not asked.)"""
    if variant == "mask_pad" and name == "resized":
        assert np.array_equal(VC.case_ref(name, variant), VC.case_ref(name))
        return
    want = golden(name)["out"]
    mag = max(1.0, float(np.abs(want).max()))
    diff = float(np.abs(VC.case_ref(name, variant) - want).max())
    print(f"{name} / {variant}: moves the output by {diff:.3f} (needs {100 * GPU_BAR * mag:.3f})")
    assert diff >= 100 * GPU_BAR * mag


def test_host_only_entry_points():
    L = _ffi.lib()
    ok = L.lvq_attention_relpos_ok
    for shape in ((14, 14, 64), (64, 64, 64), (1, 1, 64), (5, 7, 64)):
        assert ok(*map(ctypes.c_int, shape)) == 1, shape
    for shape in ((14, 14, 80), (65, 14, 64), (14, 65, 64), (0, 4, 64)):
        assert ok(*map(ctypes.c_int, shape)) == 0, shape
    for prec in (1, 3):
        n = L.lvq_attention_relpos_workspace_bytes(*map(ctypes.c_int, (1, 12, 64, 64, 64, prec)))
        assert 0 <= n < 12 * 64 * 64 * 64 * 64 * 4
