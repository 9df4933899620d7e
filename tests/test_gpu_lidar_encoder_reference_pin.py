"""The HIP sparse backbones, the dynamic VFEs and the LiDAR-encoder chain of every nuScenes model config on the MI355X, held directly to
what the reference's UNMODIFIED classes returned (tests/golden/lidar_pin_*, made by tools/make_lidar_encoder_goldens.py through the
stand-ins of tools/ref_standins.py; tests/test_lidar_encoder_reference_pin.py holds the CPU restatements to the same files).

Bars, none of them new:
  backbones, bf16x3    max|out - ref| / max(1, max|ref|) <= 1e-3 at every stage, the parity bar of tests/test_gpu_second_pillarnet.py and
                       tests/test_gpu_backbone3d.py; active sets equal after sorting.  Plain bf16 stays recorded-only in those files.
  config chains        the same measure and bar on spatial_features_2d (test_second_chain_end_to_end's); coordinates and row counts exact
  dynamic VFEs         coordinates bit-equal; features within 5e-5 absolute of the fp32 fixture (test_dynamic_pfn_vs_oracle's bar)
A stage too large to keep whole is held as tests/conftest.py's golden_error holds a sliced fixture (lidar_encoder_pin_cases.held).

Measured on the MI355X (the figures each test prints):
  backbone stages, worst stage of each case   VoxelBackBone8x 6.9e-6 (x_conv1; out 4.3e-6), VoxelResBackBone8x 1.1e-5 (out, USE_BIAS False;
                                              HeightCompression 9.3e-6), PillarBackBone8x 1.5e-5 (x_conv3), PillarRes18BackBone8x 1.2e-5
                                              (x_conv4), VoxelResBackBone8xVoxelNeXt 6.6e-6 (out; merged 3.4e-6)
  config chains                               bevfusion / transfusion_lidar 2.0e-5, cbgs_dyn_pp_centerpoint 1.3e-5,
                                              cbgs_pillar0075_res2d_centerpoint 2.5e-5, cbgs_pp_multihead 2.6e-5, cbgs_second_multihead /
                                              cbgs_voxel01_res3d_centerpoint 2.4e-5, cbgs_voxel0075_res3d_centerpoint 2.0e-5,
                                              cbgs_voxel0075_voxelnext (and _doubleflip) 7.5e-6
  dynamic VFEs against the fp32 fixture       DynMeanVFE 1.9e-6; DynPillarVFE, DynamicVoxelVFE and DynamicPillarVFESimple2D at most 1.53e-5
                                              (two fp32 ulps at |x| in [32, 64)) over the four flag settings: every class meets 5e-5
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bev_backbone_cases as BC  # noqa: E402
import lidar_encoder_pin_cases as P  # noqa: E402
import second_pillarnet_cases as C  # noqa: E402
from lidar_vision_vqa_amd import backbone2d as B2  # noqa: E402
from lidar_vision_vqa_amd import backbone3d as B3  # noqa: E402
from lidar_vision_vqa_amd import lidar  # noqa: E402
from test_gpu_second_pillarnet import BAR, dev, load  # noqa: E402

DEV = "cuda:0"
DYN_BAR = 5e-5                                                                  # tests/test_gpu_lidar.py::test_dynamic_pfn_vs_oracle
OURS = dict(vfe=lidar.__all__, backbone_3d=B3.backbones_3d_all, map_to_bev=lidar.map_to_bev_all, backbone_2d=B2.backbones_2d_all)
NAMES = P.load_json("names")
CONFIGS = P.load_json("configs")


def cpu(x):
    return x.detach().cpu().numpy()


def sparse_errors(st, g, stages):
    """{stage: relative error} of our sparse tensors against the fixture; shapes and sorted active sets must be equal."""
    return {k: P.rel(*P.held_sparse(g, k, cpu(st[k].features), cpu(st[k].indices), st[k].spatial_shape, multiset=k == "merged")) for k in stages}


# --------------------------------------------------------------------------------------------------------------------------------
# the five backbones against fixture a
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.BACKBONES))
def test_hip_backbone_against_the_reference_class_at_every_stage(name):
    k, g = P.backbone_case(name), P.load(name)
    m = load(B3.backbones_3d_all[k["cls"]](BC.Cfg(k["cfg"]), k["cin"], list(k["grid"])), k["sd"])
    m.precision = "bf16x3"
    key = "pillar" if k["cls"] in C.PILLAR else "voxel"
    bd = {f"{key}_features": dev(k["feat"]), f"{key}_coords": dev(k["idx"], np.int32), "batch_size": k["batch"]}
    before = set(bd)
    with torch.no_grad():
        bd = m(bd)
    errs = sparse_errors(P.sparse_stages(bd, k["cls"]), g, P.stage_names(k["cls"]))
    if key == "pillar":
        for s in ("x_conv4", "x_conv5"):
            errs[s] = P.rel(*P.held_dense(g, s, cpu(bd["multi_scale_2d_features"][s])))
    assert P.returned_names(before, bd) == NAMES["returns"][name]
    if name == P.HEIGHT_COMPRESSION_OF:
        hc = lidar.map_to_bev_all["HeightCompression"](BC.Cfg(NUM_BEV_FEATURES=256))
        after = set(bd)
        errs["spatial_features"] = P.rel(*P.held_dense(g, "spatial_features", cpu(hc(bd)["spatial_features"])))
        assert P.returned_names(after, bd) == NAMES["returns"]["HeightCompression"]
    print(f"{name} bf16x3 against the reference class: " + ", ".join(f"{s} {e:.2e}" for s, e in errs.items()))
    assert max(errs.values()) <= BAR, errs


# --------------------------------------------------------------------------------------------------------------------------------
# the dynamic VFEs
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.DYNAMIC))
def test_hip_dynamic_vfe_against_the_reference_class(name):
    cls, cfg, args, kind, seed = P.dynamic_setup(name)
    g = P.load("dyn_" + name)
    m = lidar.__all__[cls](model_cfg=BC.Cfg(cfg), **args)
    m = (load(m, P.seeded_state(m, seed)) if seed is not None else m).to(DEV).eval()
    bd = dict(points=dev(P.dynamic_points()), batch_size=P.DYN_POINTS[0])
    before = set(bd)
    bd = m(bd)
    coords = cpu(bd["pillar_coords" if kind == "simple2d" else "voxel_coords"])
    assert coords.dtype == np.int32 and np.array_equal(coords, g["coords"]), "coordinates differ"
    assert P.returned_names(before, bd) == NAMES["returns"]["dyn_" + name]
    err, mag = P.held(g, "features", cpu(bd["voxel_features" if kind == "mean" else "pillar_features"]))
    print(f"{name} against the reference class (fp32): {err:.3e} absolute (max|ref| {mag:.3f})")
    assert err <= DYN_BAR, (name, err)


# --------------------------------------------------------------------------------------------------------------------------------
# the config chains against fixture c
# --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def config_batch(name):
    return P.config_input(CONFIGS[name])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_hip_config_chain_against_the_reference_classes(name):
    """VFE -> BACKBONE_3D -> MAP_TO_BEV -> BACKBONE_2D as the config names them, through our registries with the reference's
    batch_dict keys, from the input the fixture was made from (checksum first)."""
    s, g = CONFIGS[name], P.load("cfg_" + name)
    inp = config_batch(name)
    if s["VFE"]["NAME"] in P.HARD_VFES:
        assert inp["checksum"] == int(g["checksum"]) and len(inp["voxel_coords"]) == int(g["n_voxels"])
        # counts and coordinates as float32: that is how the reference's load_data_to_gpu hands them over
        bd = dict(voxels=dev(inp["voxels"]), voxel_num_points=dev(inp["voxel_num_points"]), voxel_coords=dev(inp["voxel_coords"]),
                  batch_size=inp["batch_size"])
    else:
        bd = dict(points=dev(inp["points"]), batch_size=inp["batch_size"])
    before = set(bd)
    with torch.no_grad():
        for stage, m in P.build_chain(s, OURS):
            m = (load(m, P.seeded_state(m, P.CFG_SEED[stage])) if len(m.state_dict()) else m.to(DEV).eval())
            if hasattr(m, "precision"):
                m.precision = "bf16x3"
            bd = m(bd)
            if stage == "vfe" and "vfe.coords" in g:
                coords = cpu(bd["pillar_coords" if "pillar_coords" in bd else "voxel_coords"])
                assert np.array_equal(coords, g["vfe.coords"]), "the dynamic VFE's coordinates differ"
            if stage == "backbone_3d":
                cls = s["BACKBONE_3D"]["NAME"]
                st = P.sparse_stages(bd, cls)
                for k in P.stage_names(cls):
                    idx = cpu(st[k].indices)
                    o = P.ascending(idx, cpu(st[k].features) if k == "merged" else None)
                    assert st[k].spatial_shape == g[k + ".shape"].tolist() and np.array_equal(idx[o], g[k + ".idx"]), f"{k}: active set differs"
    assert P.returned_names(before, bd)["keys"] == NAMES["returns"]["cfg_" + name]["keys"]
    if "spatial_features_2d" in bd:
        err, mag = P.held_dense(g, "spatial_features_2d", cpu(bd["spatial_features_2d"]))
    else:
        e = bd["encoded_spconv_tensor"]
        err, mag = P.held_sparse(g, "out", cpu(e.features), cpu(e.indices), e.spatial_shape)
    print(f"{name} chain against the reference classes: err {P.rel(err, mag):.3e} (max|ref| {mag:.3f})")
    assert mag > 1e-2 and P.rel(err, mag) <= BAR
