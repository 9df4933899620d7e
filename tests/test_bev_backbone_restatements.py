"""The fp64 restatement of tests/bev_backbone_cases.py against the goldens of the unmodified reference class
(tests/golden/bev_backbone_*.npz, tools/make_bev_backbone_golden.py), and the parameter layout of backbone2d.BaseBEVBackbone against
the key list the goldens record.  No GPU.

Bar: 2e-5 max(1, max|ref|), the one tests/test_oracle_vat.py holds fp64 restatements to against fp32-torch goldens."""
import os

import numpy as np
import pytest
import torch

import bev_backbone_cases as BC
from lidar_vision_vqa_amd import backbone2d as B2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 2e-5


def golden(name):
    return np.load(os.path.join(GOLDEN, BC.golden_name(name)))


@pytest.mark.parametrize("name", list(BC.CASES))
def test_restatement_agrees_with_the_reference_class(name):
    want = golden(name)["out"]
    ref = BC.case_ref(name)
    assert ref.shape == want.shape and want.dtype == np.float32
    mag = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(ref - want).max())
    zeros = float((want == 0).mean())
    print(f"{name}: restatement vs golden {err:.3e} (bar {BAR * mag:.3e}, max|ref| {mag:.3f}, zeros {zeros:.3f})")
    assert err <= BAR * mag
    assert zeros < 0.9 and mag > 1.0                                            # a golden of dead ReLUs would test nothing


@pytest.mark.parametrize("name", list(BC.CASES))
def test_state_dict_keys_and_shapes_are_the_reference_s(name):
    g = golden(name)
    want = [(str(k), tuple(int(d) for d in str(s).split(",") if d)) for k, s in zip(g["keys"], g["shapes"])]
    cfg, cin, _, _, _ = BC.CASES[name]
    m = B2.BaseBEVBackbone(BC.Cfg(cfg), cin)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want                                                          # same keys, same order, same shapes
    assert got == [(k, tuple(s)) for k, s in BC.state_shapes(*BC.structure(BC.Cfg(cfg), cin))]
    assert "blocks.0.1.weight" in dict(got) and "blocks.0.2.running_var" in dict(got)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in BC.case_state(name).items()}, strict=True)
    assert m.num_bev_features == sum(cfg["NUM_UPSAMPLE_FILTERS"]) == g["out"].shape[1]
    assert isinstance(m.blocks[0][0], torch.nn.ZeroPad2d) and isinstance(m.blocks[0][1], torch.nn.Conv2d)


def test_default_init_consumes_the_rng_in_torch_s_order():
    """The containers are built in the reference's order (base_bev_backbone.py:30-77), so one seed gives the weights of that order."""
    import torch.nn as nn
    cfg = BC.case_cfg("nusc_pp")
    torch.manual_seed(7)
    ours = B2.BaseBEVBackbone(cfg, 64)
    torch.manual_seed(7)
    first = nn.Conv2d(64, 64, kernel_size=3, stride=2, padding=0, bias=False)
    second = nn.Conv2d(64, 64, kernel_size=3, padding=1, bias=False)
    assert torch.equal(ours.blocks[0][1].weight, first.weight) and torch.equal(ours.blocks[0][4].weight, second.weight)
    assert isinstance(ours.deblocks[0][0], nn.Conv2d) and ours.deblocks[0][0].kernel_size == (2, 2) and ours.deblocks[0][0].stride == (2, 2)
    assert isinstance(ours.deblocks[2][0], nn.ConvTranspose2d)


def test_optional_layers_of_the_config():
    """USE_CONV_FOR_NO_STRIDE, the extra final deblock (one more UPSAMPLE_STRIDES entry than levels), and BaseBEVBackboneV1."""
    import torch.nn as nn
    cfg = BC.Cfg(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[64, 128], UPSAMPLE_STRIDES=[1, 2, 2], NUM_UPSAMPLE_FILTERS=[64, 64],
                 USE_CONV_FOR_NO_STRIDE=True)
    with pytest.raises(AssertionError):
        B2.BaseBEVBackbone(cfg, 64)                                             # base_bev_backbone.py:20
    cfg = BC.Cfg(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[64, 128], UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[64, 64],
                 USE_CONV_FOR_NO_STRIDE=True)
    m = B2.BaseBEVBackbone(cfg, 64)
    assert isinstance(m.deblocks[0][0], nn.Conv2d) and m.deblocks[0][0].kernel_size == (1, 1)
    assert isinstance(m.deblocks[1][0], nn.ConvTranspose2d) and m.num_bev_features == 128
    v1 = B2.BaseBEVBackboneV1(BC.Cfg(BC.V1_CASE[0]))
    got = [(k, tuple(v.shape)) for k, v in v1.state_dict().items()]
    assert got == [(k, tuple(s)) for k, s in BC.state_shapes(*BC.structure_v1(BC.V1_CASE[0]))]
    assert v1.num_bev_features == 256
