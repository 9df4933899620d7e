"""CPU checks of tests/lidar_feature_cases.py, which tests/test_gpu_lidar_feature_kernels.py holds the HIP kernels to.

1. The fp64 restatements agree with oracle/lidar_oracle.py (torch fp32, pinned to the reference's goldens by tests/test_oracle_lidar.py) on the
   oracle's own configurations, within the derived bound plus the fp32 rounding of the oracle's output: this pins layout and conventions
   (feature order per flag combination, (b, z, y, x), the z of f_center per kind).
2. For every GPU case, the fp32 emulation in the kernel's documented operation order stays within 1 x the bound of its fp64 value, so
   the GPU assertion (2 x bound) is never looser than the arithmetic explains."""
import numpy as np
import pytest
import torch

import cases
import lidar_feature_cases as LF
from lidar_vision_vqa_amd import synth
from oracle import lidar_oracle as LO
from test_oracle_lidar import pillar_sd

RNG = list(synth.PC_RANGE_NUSC)
U = LF.U


def geometry(vs):
    """(vsize, offset) as the oracle's fp32 tensors see them: python floats rounded to fp32 where they meet a tensor."""
    off = [vs[k] / 2 + RNG[k] for k in range(3)]
    return np.asarray(vs, np.float32), np.asarray(off, np.float32)


def folded(sd, n_layers):
    """Eval BatchNorm (eps 1e-3) folded in fp64 -> layers [(w, scale, shift)] and, per layer, the widening of the affine term for a
    subject that evaluates (y - mean) / sqrt(var + eps) * gamma + beta in fp32: six roundings on |acc scale| + |mean scale| + |beta|."""
    layers, affine = [], []
    for i in range(n_layers):
        p = f"pfn_layers.{i}."
        g = {k: sd[p + k].double().numpy() for k in ("linear.weight", "norm.weight", "norm.bias", "norm.running_mean", "norm.running_var")}
        scale = g["norm.weight"] / np.sqrt(g["norm.running_var"] + 1e-3)
        layers.append((g["linear.weight"], scale, g["norm.bias"] - g["norm.running_mean"] * scale))
        affine.append((6.0, np.abs(g["norm.running_mean"] * scale) + np.abs(g["norm.bias"])))
    return layers, affine


def hold(name, got, ref, bound, slack=0.0):
    err = np.abs(np.asarray(got, np.float64) - ref)
    lim = bound + slack
    ratio = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: max err {float(err.max()) if err.size else 0.0:.3e}  max err/bound {ratio:.3f}")
    assert (err <= lim).all(), (name, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------
# 1. against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def hard_batch(c, t, vs):
    scenes = []
    for s in range(2):
        pts = synth.scene_points(c["dist"], c["n"], c["seed"] + 100 * s)
        pts = pts[LO.mask_points_by_range(pts, RNG)]
        vox, co, num = LO.VoxelGenerator(vs, RNG, 4, t, c["max_voxels"]).generate(pts)
        scenes.append(dict(voxels=vox, voxel_coords=co, voxel_num_points=num))
    return LO.collate_batch(scenes)


@pytest.mark.parametrize("name", list(cases.PILLAR_CASES))
@pytest.mark.parametrize("with_distance,use_absolute_xyz", [(False, True), (True, True), (False, False), (True, False)])
def test_pillar_vfe_restatement_vs_oracle(name, with_distance, use_absolute_xyz):
    c = cases.PILLAR_CASES[name]
    b = hard_batch(c, c["T"], synth.VOXEL_PILLAR)
    flags = (1 if use_absolute_xyz else 0) | (2 if with_distance else 0)
    sd = pillar_sd(c["filters"], c["wseed"], c_in=LF.pfn_cin(4, flags))
    o = LO.pillar_vfe(b["voxels"], b["voxel_num_points"], b["voxel_coords"], sd, synth.VOXEL_PILLAR, RNG, c["filters"],
                      with_distance=with_distance, use_absolute_xyz=use_absolute_xyz).numpy()
    layers, affine = folded(sd, len(c["filters"]))
    vs, off = geometry(synth.VOXEL_PILLAR)
    ref, bound = LF.pillar_vfe(b["voxels"], b["voxel_num_points"], b["voxel_coords"], layers, flags, vs, off, affine=affine)
    assert (b["voxel_num_points"] < c["T"]).any() and ref.shape == o.shape
    hold(f"pillar_vfe {name} flags={flags}", o, ref, bound, U * np.abs(ref))


@pytest.mark.parametrize("kind,filters,vs", [("pillar", [64], synth.VOXEL_PILLAR), ("pillar", [64, 64], synth.VOXEL_PILLAR),
                                             ("voxel", [64, 64], synth.VOXEL_01), ("simple2d", [32], synth.VOXEL_PILLAR)])
@pytest.mark.parametrize("with_distance,use_absolute_xyz", [(False, True), (True, False)])
def test_dynamic_pfn_restatement_vs_oracle(kind, filters, vs, with_distance, use_absolute_xyz):
    k = {"pillar": 0, "voxel": 1, "simple2d": 2}[kind]
    flags = (1 if use_absolute_xyz else 0) | (2 if with_distance else 0)
    per = [synth.scene_points("C", 3000, 120 + s) for s in range(2)]
    bpts = np.concatenate([np.pad(p, ((0, 0), (1, 0)), constant_values=s) for s, p in enumerate(per)]).astype(np.float32)
    grid = LO.grid_size(RNG, vs)
    sd = pillar_sd(filters, 300 + len(filters), c_in=LF.dyn_cin(5, k, flags))
    o = LO.dynamic_pfn_vfe(bpts, RNG, vs, grid, sd, filters, kind, with_distance=with_distance, use_absolute_xyz=use_absolute_xyz)
    pts, inv, m = bpts[o["keep"]], o["unq_inv"], len(o["unq_key"])
    pmean = LO.scatter_mean(torch.from_numpy(pts[:, 1:4].copy()), torch.from_numpy(inv), m).numpy()
    layers, affine = folded(sd, len(filters))
    v, off = geometry(vs)
    ref, bound = LF.dynamic_pfn(pts, inv, o["coords"], pmean, k, layers, flags, m, v, off, affine=affine)
    hold(f"dynamic_pfn {kind} {filters} flags={flags}", o["features"].numpy(), ref, bound, U * np.abs(ref))


def test_mean_scatter_mean_and_scatter_restatements_vs_oracle():
    c = cases.MEAN_CASES["mean_C8k"]
    pts = synth.scene_points(c["dist"], c["n"], c["seed"])
    pts = pts[LO.mask_points_by_range(pts, RNG)]
    vox, co, num = LO.VoxelGenerator(synth.VOXEL_01, RNG, 4, c["T"], c["max_voxels"]).generate(pts)
    ref = LF.mean_vfe(vox, num)
    bound = (c["T"] + 1) * U * np.abs(vox.astype(np.float64)).sum(axis=1) / np.maximum(num, 1)[:, None]
    hold("mean_vfe", LO.mean_vfe(vox, num), ref, bound)
    hold("mean_vfe fp32 sequence", LF.mean_vfe_f32(vox, num), ref, bound)
    # scatter_mean: DynamicMeanVFE's use (points[:, 1:], dynamic_mean_vfe.py:64)
    bpts = np.pad(pts, ((0, 0), (1, 0)))
    dv = LO.dynamic_mean_vfe(bpts, RNG, synth.VOXEL_01, LO.grid_size(RNG, synth.VOXEL_01))
    kept, inv, m = bpts[dv["keep"]], dv["unq_inv"].astype(np.int32), len(dv["unq_key"])
    ref, bound = LF.scatter_mean(kept, 1, 4, inv, dv["unq_cnt"], m)
    hold("scatter_mean", dv["voxel_features"].numpy(), ref, bound, U * np.abs(ref))
    # PointPillarScatter: a copy, equal element for element
    co4 = np.pad(co[:500, [0, 1, 2]], ((0, 0), (1, 0))).astype(np.int32)
    co4[:, 1] = 0
    co4 = np.unique(co4 // np.array([1, 1, 2, 2]), axis=0).astype(np.int32)          # distinct cells of the 512 x 512 pillar grid
    co4[::2, 0] = 1
    feat = synth.randn((len(co4), 3), 5)
    assert np.array_equal(LO.pointpillar_scatter(feat, co4, 512, 512).numpy(), LF.pillar_scatter(feat, co4, len(co4), 2, 512, 512))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the fp32 emulations of the GPU cases stay within 1 x bound
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_bound_holds_fp32_pillar_single_layer(fast):
    worst = 0.0
    for args in LF.pillar_single_layer_cases():
        k = LF.pillar_case(*args)
        m = k["m"]
        got = LF.pillar_vfe_f32(k["voxels"][:m], k["num"][:m], k["coords"][:m], k["layers"], k["flags"], fast)
        err = np.abs(got.astype(np.float64) - k["ref"])
        assert (err <= k["bound"]).all(), (args, float((err / k["bound"]).max()))
        worst = max(worst, float((err / k["bound"]).max()))
    print(f"pillar_vfe fp32 emulation ({'butterfly' if fast else 'sequential'} mean): largest err/bound {worst:.3f}")


@pytest.mark.parametrize("args", LF.pillar_generic_cases(), ids=lambda a: f"T{a[1]}c{a[2]}_{'x'.join(map(str, a[3]))}_f{a[4]}")
def test_bound_holds_fp32_pillar_generic(args):
    k = LF.pillar_case(*args)
    m = k["m"]
    assert LF.pillar_lds_bytes(k["t"], k["c"], k["couts"], k["flags"]) is not None
    got = LF.pillar_vfe_f32(k["voxels"][:m], k["num"][:m], k["coords"][:m], k["layers"], k["flags"], False)
    hold(f"pillar_vfe fp32 {args[:5]}", got, k["ref"], k["bound"])


def test_pillar_generic_cases_cover_every_launch_shape():
    """The generic list reaches 4-, 2- and 1-wave workgroups, a request above 64 KB, and both kernels at exactly 160 KB."""
    shapes = [LF.pillar_lds_bytes(a[1], a[2], a[3], a[4]) + (a[1] <= 32,) for a in LF.pillar_generic_cases()]
    assert {s[0] for s in shapes} == {1, 2, 4}
    assert any(s[1] > 64 * 1024 for s in shapes) and any(s[1] == 160 * 1024 and not s[2] for s in shapes)
    assert LF.pillar_lds_bytes(64, 4, (64, 64), 1) is not None and LF.pillar_lds_bytes(32, 4, (256,), 1) is not None
    assert LF.pillar_lds_bytes(41, 4, (256, 256), 1) is None and LF.pillar_lds_bytes(64, 4, (161, 32), 1) is None


@pytest.mark.parametrize("args", LF.dynamic_cases(), ids=lambda a: f"n{a[0]}c{a[1]}k{a[2]}f{a[3]}_{'x'.join(map(str, a[4]))}")
def test_bound_holds_fp32_dynamic_pfn(args):
    k = LF.dynamic_case(*args)
    got = LF.dynamic_pfn_f32(k["pts"], k["inv"], k["pcoord"], k["pmean"], k["kind"], k["layers"], k["flags"], k["m_cap"])
    hold(f"dynamic_pfn fp32 {args[:5]}", got, k["ref"], k["bound"])
    assert (got[k["empty"]] == 0).all()


def test_bound_holds_fp32_scatter_mean():
    for args in LF.scatter_cases():
        k = LF.scatter_case(*args)
        got = LF.scatter_mean_f32(k["pts"], k["col0"], k["nc"], k["inv"], k["cnt"], k["m_cap"])
        hold(f"scatter_mean fp32 {args[:4]}", got, k["ref"], k["bound"])


@pytest.mark.parametrize("c,h,w", LF.DWCONV_SHAPES)
def test_bound_holds_fp32_dwconv(c, h, w):
    k = LF.dwconv_case(c, h, w, 9700 + c)
    for key, bias in (("bias", k["bias"]), ("nobias", None)):
        y, a = k["ref"][key]
        for lo in (False, True):
            hold(f"dwconv fp32 {c}x{h}x{w} {key} lo={lo}", LF.dwconv3x3_gelu_f32(k["bev"], k["w9"], bias, lo), y, LF.dwconv_bound(y, a, lo))


def test_copy_and_bridge_case_builders_hold_their_properties():
    """The builders assert their own point; building every one here keeps a silently degenerate case from reaching the GPU run."""
    for ny, nx in LF.COPY_GRIDS:
        for d in (1, 2, 5):
            rows, live = LF.grid_rows(2, d, ny, nx, 9800 + d)
            assert live < len(rows) or ny * nx * d * 2 == 1
    for c, h, w in LF.DWCONV_SHAPES:
        k = LF.bridge_case(c, h, w, 9900 + c)
        assert k["live"] < k["cap"]
    big = LF.bridge_case(136, 9, 130, 9900 + 136)
    assert LF.block_census(big["idx"][2], 0, 1) == (0, 1, 0, 0) and LF.block_census(big["idx"][2], 0, 2) == (0, 0, 0, 0)
    assert LF.block_census(big["idx"][3], 0, 1) == (0, 0, 1, 0) and LF.block_census(big["idx"][3], 0, 0) == (0, 0, 0, 0)
