"""BaseBEVBackbone / BaseBEVBackboneV1 (lidar-vision-vqa_amd/backbone2d.py on csrc/conv2d.hip) against the goldens of the unmodified
reference class (tests/golden/bev_backbone_*.npz) and the fp64 restatement of tests/bev_backbone_cases.py, and the hand-over through the
pillar path (PillarVFE -> PointPillarScatter -> BaseBEVBackbone -> fp16 store -> VATLiDAR).

bf16x3 (hi + lo operands) is held to the project's parity bar, 1e-3 max(1, max|ref|).  The plain bf16 form has no bar known in advance:
PLAIN_MEASURED holds the error measured against the restatement, and the test asserts twice that value as a regression
guard, as tests/test_gpu_backbone3d.py does."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bev_backbone_cases as BC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import backbone2d as B2  # noqa: E402
from lidar_vision_vqa_amd import synth  # noqa: E402

DEV = "cuda:0"
BAR = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# max |out - restatement| / max(1, max|restatement|) of spatial_features_2d in the plain bf16 form, measured on the MI355X
PLAIN_MEASURED = {"kitti_pp": 6.84e-3, "nusc_pp": 8.16e-3, "nusc_second": 7.09e-3}     # (bf16x3 on the same cases: 1.27e-5, 1.28e-5, 1.42e-5)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def model(name):
    cfg, cin, _, _, _ = BC.CASES[name]
    m = B2.backbones_2d_all["BaseBEVBackbone"](BC.Cfg(cfg), cin)
    m.load_state_dict({k: t(v) for k, v in BC.case_state(name).items()}, strict=True)
    return m.to(DEV).eval()


def run(m, x, mode):
    m.precision = mode
    with torch.no_grad():
        return m(dict(spatial_features=t(x).to(DEV)))["spatial_features_2d"]


def rel(out, ref):
    return float(np.abs(out - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("name", list(BC.CASES))
def test_backbone_bf16x3_reproduces_the_reference_class(name):
    want = np.load(os.path.join(GOLDEN, BC.golden_name(name)))["out"]
    out = run(model(name), BC.case_input(name), "bf16x3").cpu().numpy()
    assert out.shape == want.shape and out.dtype == np.float32
    err, err64 = rel(out, want), rel(out, BC.case_ref(name))
    print(f"{name} bf16x3: vs golden {err:.3e}, vs fp64 restatement {err64:.3e} (max|ref| {np.abs(want).max():.3f})")
    assert err <= BAR, err


@pytest.mark.parametrize("name", list(BC.CASES))
def test_backbone_plain_bf16_regression_guard(name):
    ref = BC.case_ref(name)
    err = rel(run(model(name), BC.case_input(name), "bf16").cpu().numpy(), ref)
    print(f"{name} bf16: vs fp64 restatement {err:.3e} (max|ref| {np.abs(ref).max():.3f})")
    assert err <= 2 * PLAIN_MEASURED[name], err


def test_backbone_v1_two_level_case():
    cfg, s4, s5, wseed, xseed = BC.V1_CASE
    sd = BC.state(*BC.structure_v1(cfg), wseed)
    m = B2.backbones_2d_all["BaseBEVBackboneV1"](BC.Cfg(cfg))
    m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    x4, x5 = synth.randn(s4, xseed), synth.randn(s5, xseed + 1)
    ref = BC.backbone_v1(cfg, sd, x4, x5)
    with torch.no_grad():
        out = m(dict(multi_scale_2d_features=dict(x_conv4=t(x4).to(DEV), x_conv5=t(x5).to(DEV))))["spatial_features_2d"].cpu().numpy()
    err = rel(out, ref)
    print(f"BaseBEVBackboneV1 bf16x3: vs fp64 restatement {err:.3e} (max|ref| {np.abs(ref).max():.3f})")
    assert out.shape == ref.shape == (2, 256, 10, 12) and err <= BAR
    with pytest.raises(F.LvqError, match="9 x 12, 10 x 12"), torch.no_grad():     # x_conv5 not at half of x_conv4's size
        m(dict(multi_scale_2d_features=dict(x_conv4=t(x4[:, :, :9]).to(DEV), x_conv5=t(x5).to(DEV))))


def test_extra_final_deblock_and_use_conv_for_no_stride():
    """One more UPSAMPLE_STRIDES entry than levels (a ConvTranspose2d over the concat: the concat then stays operand planes) and the 1 x 1
    strided-conv deblock of USE_CONV_FOR_NO_STRIDE."""
    cfg = BC.Cfg(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[64, 128], UPSAMPLE_STRIDES=[1, 2, 2], NUM_UPSAMPLE_FILTERS=[64, 64, 0],
                 USE_CONV_FOR_NO_STRIDE=True)
    blocks, deblocks = BC.structure(cfg, 40)
    sd = BC.state(blocks, deblocks, 41)
    m = B2.BaseBEVBackbone(cfg, 40)
    m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    x = synth.randn((2, 40, 8, 10), 42)
    ref = BC.backbone(cfg, 40, sd, x)
    out = run(m.to(DEV).eval(), x, "bf16x3").cpu().numpy()
    assert out.shape == ref.shape == (2, 128, 16, 20) and rel(out, ref) <= BAR


def test_no_deblocks_concatenates_the_block_outputs():
    """Without UPSAMPLE_STRIDES the reference concatenates the blocks' own outputs (base_bev_backbone.py:97-103): a block's last conv then
    feeds the next block and its channel range of the result."""
    cfg = BC.Cfg(LAYER_NUMS=[1, 0], LAYER_STRIDES=[1, 1], NUM_FILTERS=[64, 128])
    sd = BC.state(*BC.structure(cfg, 64), 43)
    m = B2.BaseBEVBackbone(cfg, 64)
    m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    x = synth.randn((2, 64, 9, 11), 44)
    ref = BC.backbone(cfg, 64, sd, x)
    out = run(m.to(DEV).eval(), x, "bf16x3").cpu().numpy()
    assert out.shape == ref.shape == (2, 192, 9, 11) and rel(out, ref) <= BAR and m.num_bev_features == 0


def test_error_paths():
    name = "nusc_pp"
    cfg, cin, shape, _, _ = BC.CASES[name]
    x = t(BC.case_input(name)).to(DEV)
    m = B2.BaseBEVBackbone(BC.Cfg(cfg), cin).to(DEV)
    with pytest.raises(F.LvqError), torch.no_grad():
        m(dict(spatial_features=x))                                             # train() mode
    m.eval()
    with pytest.raises(F.LvqError):
        m(dict(spatial_features=x))                                             # gradients in reach
    with pytest.raises(F.LvqError, match="5 x 5, 5 x 5, 6 x 6"), torch.no_grad():
        m(dict(spatial_features=x[:, :, :20, :20].contiguous()))                # 20 is not divisible by the total stride 8: blocks 10, 5, 3 -> deblocks 5, 5, 6
    m.precision = "fp8"
    with pytest.raises(F.LvqError), torch.no_grad():
        m(dict(spatial_features=x))
    m.precision = None
    with torch.no_grad():
        assert tuple(m(dict(spatial_features=x))["spatial_features_2d"].shape) == (1, 384, 8, 8)
    odd = B2.BaseBEVBackbone(BC.Cfg(LAYER_NUMS=[1], LAYER_STRIDES=[1], NUM_FILTERS=[48], UPSAMPLE_STRIDES=[1], NUM_UPSAMPLE_FILTERS=[64]), 64)
    with pytest.raises(F.LvqError, match="outside the kernel family"), torch.no_grad():
        odd.to(DEV).eval()(dict(spatial_features=x))                            # C_out = 48


def test_state_dict_reload_is_bit_identical_and_weight_updates_are_picked_up():
    name = "nusc_pp"
    cfg, cin, _, _, _ = BC.CASES[name]
    x = BC.case_input(name)
    a = run(model(name), x, "bf16x3").clone()
    assert torch.equal(a, run(model(name), x, "bf16x3"))                        # run to run
    m2 = B2.BaseBEVBackbone(BC.Cfg(cfg), cin).to(DEV).eval()
    m2.load_state_dict(model(name).state_dict(), strict=True)
    assert torch.equal(a, run(m2, x, "bf16x3"))
    layer = m2._plan()["blocks"][1][2][0]
    packed = layer.packed(True)
    assert layer.packed(True)[0] is packed[0]
    with torch.no_grad():
        m2.blocks[1][7].weight.mul_(1.5)                                        # the third conv of block 1, in place: a new parameter version
        m2.blocks[0][2].running_var.mul_(2.0)
    assert layer.packed(True)[0] is not packed[0]
    b = run(m2, x, "bf16x3")
    sd = {k: v.cpu().numpy() for k, v in m2.state_dict().items()}
    ref = BC.backbone(BC.Cfg(cfg), cin, sd, x)
    assert not torch.equal(a, b) and rel(b.cpu().numpy(), ref) <= BAR


def test_pillar_path_hands_over_to_the_store_and_vat_lidar(tmp_path):
    """points -> pillars on a 32 x 32 grid -> PillarVFE -> PointPillarScatter -> BaseBEVBackbone (nuScenes PointPillars config) ->
    bev.save_bev_feature -> BevFeatureStore: the stored canvas is the fp16 rounding of spatial_features_2d; VATLiDAR takes the 384-channel
    canvas on its dense route and meets oracle.vat_oracle.vat_lidar at 1e-3."""
    from lidar_vision_vqa_amd import bev, fusion, lidar
    from oracle import vat_oracle as VO
    rng, vs = list(synth.PC_RANGE_NUSC), (3.2, 3.2, 8.0)
    assert lidar.grid_size_from(rng, vs).tolist() == [32, 32, 1]
    scenes = [t(synth.scene_points("C", 4096, 50 + s)).to(DEV) for s in range(2)]
    bd = lidar.voxelize_batch(lidar.VoxelGeneratorWrapper(vs, rng, 4, 20, 2048), scenes)
    vfe_cfg = BC.Cfg(USE_NORM=True, WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, NUM_FILTERS=[64])
    vfe = synth.load_seeded(lidar.__all__["PillarVFE"](model_cfg=vfe_cfg, num_point_features=4, voxel_size=list(vs), point_cloud_range=rng,
                                                       grid_size=[32, 32, 1]), 51).to(DEV).eval()
    scatter = lidar.map_to_bev_all["PointPillarScatter"](BC.Cfg(NUM_BEV_FEATURES=64), [32, 32, 1])
    m = model("nusc_pp")
    m.precision = None
    with torch.no_grad():
        bd = m(scatter(vfe(bd)))
    canvas, feats2d = bd["spatial_features"], bd["spatial_features_2d"]
    assert tuple(canvas.shape) == (2, 64, 32, 32) and tuple(feats2d.shape) == (2, 384, 8, 8) and bool(torch.isfinite(feats2d).all())
    ref = BC.backbone(BC.case_cfg("nusc_pp"), 64, BC.case_state("nusc_pp"), canvas.cpu().numpy())
    assert rel(feats2d.cpu().numpy(), ref) <= BAR and float(np.abs(ref).max()) > 0.5
    for s in range(2):
        bev.save_bev_feature(tmp_path / f"tok{s}.npy", feats2d[s])
    loaded = bev.BevFeatureStore([str(tmp_path)], DEV).load(["tok0", "tok1"])
    assert torch.equal(loaded, feats2d.half().float())                          # the fp16 rounding, exactly
    vat = synth.load_seeded(fusion.VATLiDAR(c_in=384, d_model=96, n_queries=12, n_layers=1, n_heads=4), 52).to(DEV).eval()
    with torch.no_grad():
        tok = vat(loaded)
    want = VO.vat_lidar(loaded.cpu(), {k: v.detach().cpu() for k, v in vat.state_dict().items()}, 4)
    err = float((tok.cpu() - want).abs().max()) / max(1.0, float(want.abs().max()))
    print(f"VATLiDAR on the 384-channel canvas: {err:.3e}")
    assert tuple(tok.shape) == (2, 12, 96) and err <= 1e-3
