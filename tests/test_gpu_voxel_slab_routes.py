"""The over-cap slab routes of csrc/voxel_binned.hip, reached on purpose and held to the CPU oracles bit for bit.

The slab-binned kernels rank every set of integer cells of the LiDAR stack -- the dynamic voxeliser, the hard voxeliser with voxel_path 1,
the rule builder of the sparse convolutions and the BEV merge -- and a slab that is locally dense takes other code: counters in global
memory with fences (k_dyn_slab_write above DYN_VCAP voxels), global stand-ins for the per-voxel state and the bucket array (k_hard_slab
above HARD_VCAP voxels / HARD_PCAP points).  tests/voxel_slab_cases.py builds inputs with one such slab; every test here first asserts,
from lvq_voxel_slab_plan (the library's own choose_cfg and constants) and the oracle's keys, that the slab is in the class the case
names -- a case that misses its route FAILS -- and then compares exactly: integers, or floats through their uint32 views.  There is
no tolerance in this file: where floats are summed (the BEV merge, the mean VFE, the convolution) the inputs are chosen so that every
sum is exact in fp32 in any order.  DESIGN.md ("Slab classes") lists what each case put into its slab."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sparse_conv_cases as SC  # noqa: E402
import voxel_slab_cases as VS  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import backbone3d as B3  # noqa: E402
from lidar_vision_vqa_amd import bev  # noqa: E402
from oracle import lidar_oracle as LO  # noqa: E402
from test_gpu_sparse_conv import run_conv  # noqa: E402
from test_gpu_sparse_conv_rules import KINDS, check  # noqa: E402

DEV = "cuda:0"
T = 10
DYN_PATHS = [pytest.param(0, id="binned"), pytest.param(2, id="bitmap")]
HARD_PATHS = [pytest.param(1, id="binned"), pytest.param(0, id="hashed"), pytest.param(2, id="legacy")]
# cases that sit ON a cap or one past it: (which count, which of the plan's caps, distance)
BOUNDARY = {"p_4096": ("vox", 0, 0), "p_4097": ("vox", 0, 1), "v_4096": ("vox", 0, 0), "v_4097": ("vox", 0, 1),
            "h_np_8192": ("pts", 2, 0), "h_np_8193": ("pts", 2, 1), "h_np_256": ("pts", 3, 0), "h_np_257": ("pts", 3, 1)}


def L():
    from lidar_vision_vqa_amd import lidar
    return lidar


class Cfg(dict):
    __getattr__ = dict.__getitem__


def plan(keyspace, n, hard):
    """(logslab, nslabs, [DYN_VCAP, HARD_VCAP, HARD_PCAP, SMALL_PCAP]) from the library: the choose_cfg and the constants the launches use."""
    ls, ns, caps = ctypes.c_int(0), ctypes.c_int(0), (ctypes.c_int * 4)()
    F.check(F.lib().lvq_voxel_slab_plan(keyspace, n, int(hard), ctypes.byref(ls), ctypes.byref(ns), caps), "lvq_voxel_slab_plan")
    return ls.value, ns.value, list(caps)


@functools.lru_cache(maxsize=None)
def dyn_oracle(name):
    c = VS.cloud(name)
    return c, LO.dynamic_voxelize(c["batched"], c["range"], c["vsize"], c["grid"], c["ndim"])


def assert_route(name, hard):
    """The slab that holds the case's dense block is in the class voxel_slab_cases.EXPECTED names, by the library's plan and caps."""
    c, o = dyn_oracle(name)
    ls, ns, caps = plan(c["keyspace"], c["n"], hard)
    vox, pts = VS.slab_stats(o["unq_key"], o["unq_cnt"], ls, ns)
    s = int(VS.cell_keys(c["cells"][:1], c["grid"], c["ndim"])[0] >> ls)
    want = VS.EXPECTED[name]
    got = VS.hard_class(vox[s], pts[s], caps[1], caps[2], caps[3]) if hard else VS.dyn_class(vox[s], caps[0])
    print(f"{name}: logslab {ls}, {ns} slabs; slab {s}: {vox[s]} voxels, {pts[s]} points -> {got}; "
          f"largest slab {vox.max()} voxels / {pts.max()} points")
    assert got == want[5 if hard else 4], (name, got, int(vox[s]), int(pts[s]), ls)
    if name in BOUNDARY and (hard or BOUNDARY[name][0] == "vox"):
        which, cap, d = BOUNDARY[name]
        cap = (1 if hard else 0) if which == "vox" else cap                   # HARD_VCAP / DYN_VCAP
        assert (vox if which == "vox" else pts)[s] == caps[cap] + d
    return s, ls, ns


def dev(a):
    return torch.tensor(a, device=DEV)            # (a copy: the builders' arrays are shared and read-only)


# ---------------------------------------------------------------------------------------------------------------------------------
# dynamic voxeliser
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voxel_path", DYN_PATHS)
@pytest.mark.parametrize("name", VS.DYN_NAMES)
def test_dynamic_dense_slab_vs_oracle(name, voxel_path, tune):
    """unq_key, unq_cnt, unq_inv, coords, pt_coords and both counts; the two-level bitmap (voxel_path 2) is held to the same oracle, so the
    two agree bit for bit.  p_* / v_*: pillar and 3-D grid; *_4096 / *_4097: the last slab with LDS counters and the first without;
    *_slab0 / *_last_partial / *_mid_slab0_empty: where the slab lies (block 0 of k_dyn_slab_write publishes M although its slab is
    empty); *_mixed: 1 .. 40 points per voxel, so the global counters add; *_scene1: the block in the second scene."""
    c, o = dyn_oracle(name)
    s, ls, ns = assert_route(name, hard=False)
    if name.endswith("_last_partial"):
        assert s == ns - 1 and c["keyspace"] % (1 << ls) != 0
    if name.endswith("_slab0_empty"):
        assert s > 0 and int((o["unq_key"] >> ls == 0).sum()) == 0
    tune(voxel_path=voxel_path)
    dv = L()._dynamic_voxelize(dev(c["batched"]), c["bs"], c["range"], c["vsize"], c["grid"], c["ndim"])
    m, nvalid = dv["counts"].cpu().tolist()
    assert m == len(o["unq_key"]) and nvalid == int(o["keep"].sum()) == c["n"]
    assert np.array_equal(dv["unq_key"][:m].cpu().numpy(), o["unq_key"])
    assert np.array_equal(dv["unq_cnt"][:m].cpu().numpy().astype(np.int64), o["unq_cnt"])
    inv = dv["inv"].cpu().numpy()
    assert np.array_equal(inv >= 0, o["keep"])
    assert np.array_equal(inv[o["keep"]].astype(np.int64), o["unq_inv"])
    assert np.array_equal(dv["coords"][:m].cpu().numpy(), LO._decode_coords(o["unq_key"], c["grid"], c["ndim"]))
    assert np.array_equal(dv["pt_coords"].cpu().numpy()[o["keep"]][:, :c["ndim"]], o["coords"][:, :c["ndim"]])


@pytest.mark.parametrize("name", ["v_mid_slab0_empty", "v_mixed"])
def test_dynamic_mean_vfe_on_the_dense_sheet(name):
    """The consumer of unq_inv / unq_cnt: DynamicMeanVFE (dynamic_mean_vfe.py:53-72) on the sheet clouds.  The points lie on a 2^-10 m
    lattice (voxel_slab_cases), so a voxel's sum of up to 40 points is exact in fp32 in any order and the mean is one correctly rounded
    division on either side: the features are compared through their bits."""
    c, _ = dyn_oracle(name)
    assert_route(name, hard=False)
    o = LO.dynamic_mean_vfe(c["batched"], c["range"], c["vsize"], c["grid"])
    m = L().__all__["DynMeanVFE"](model_cfg=Cfg(), num_point_features=4, voxel_size=list(c["vsize"]), grid_size=c["grid"],
                                  point_cloud_range=c["range"])
    bd = m(dict(points=dev(c["batched"]), batch_size=c["bs"]))
    assert np.array_equal(bd["voxel_coords"].cpu().numpy(), o["voxel_coords"])
    got, want = bd["voxel_features"].cpu().numpy(), o["voxel_features"].numpy()
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# hard voxeliser
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _generator(grid_name, mv):
    pcr, vs, _, _ = VS.GRIDS[grid_name]
    return LO.VoxelGenerator(vs, pcr, 4, T, mv)


@functools.lru_cache(maxsize=None)
def hard_oracle(name, mv):
    c = VS.cloud(name)
    return [_generator(c["grid_name"], mv).generate(sc) for sc in c["scenes"]]


def hard_vs_oracle(name, mv):
    c = VS.cloud(name)
    lid = L()
    gen = lid.VoxelGeneratorWrapper(c["vsize"], c["range"], 4, T, mv)
    assert gen.grid.tolist() == c["grid"]
    bd = lid.voxelize_batch(gen, [dev(sc) for sc in c["scenes"]])
    svo = bd["scene_voxel_off"].cpu().numpy()
    co, num, vox = bd["voxel_coords"].cpu().numpy(), bd["voxel_num_points"].cpu().numpy(), bd["voxels"].cpu().numpy()
    want = hard_oracle(name, mv)
    assert svo.tolist() == np.concatenate(([0], np.cumsum([len(on) for _, _, on in want]))).tolist()
    for s, (ov, oc, on) in enumerate(want):
        a, b = svo[s], svo[s + 1]
        assert np.array_equal(co[a:b, 1:], oc) and (co[a:b, 0] == s).all(), s
        assert np.array_equal(num[a:b], on), s
        assert np.array_equal(vox[a:b].view(np.uint32), ov.view(np.uint32)), s
    return want


@pytest.mark.parametrize("voxel_path", HARD_PATHS)
@pytest.mark.parametrize("name", VS.HARD_NAMES)
def test_hard_dense_slab_vs_oracle(name, voxel_path, tune):
    """Voxels (bits), coords, num_points and scene_voxel_off at T = 10 on all three implementations; voxel_path 1 is the one that runs
    k_hard_slab.  The four (vfit, pfit) classes (h_ordinary, h_vfit_pover, h_vover_pfit, h_vover_pover; the last two on the 3-D grid
    as well, and in the second scene of a batch) and both sides of 4096 voxels, 8192 points and 256 points (k_hard_slab_small's last
    slab and k_hard_slab's first)."""
    assert_route(name, hard=True)
    tune(voxel_path=voxel_path)
    hard_vs_oracle(name, 60000)


@pytest.mark.parametrize("voxel_path", HARD_PATHS)
def test_hard_max_voxels_cuts_inside_the_dense_slab(voxel_path, tune):
    """max_voxels = 3000 of 5420 voxels, 5120 of them in the over-cap slab: voxels ranked by the global stand-ins are dropped by
    `rank >= max_voxels` in the placement pass, and the kept ones keep their first-appearance order."""
    name, mv = "h_vover_pfit", 3000
    s, ls, _ = assert_route(name, hard=True)
    tune(voxel_path=voxel_path)
    (ov, oc, on), = hard_vs_oracle(name, mv)
    c = VS.cloud(name)
    kept = VS.cell_keys(np.concatenate([np.zeros((len(oc), 1), np.int64), oc[:, ::-1]], axis=1), c["grid"], 3) >> ls == s
    assert len(on) == mv and 0 < int(kept.sum()) < 5120 and not kept.all()


# ---------------------------------------------------------------------------------------------------------------------------------
# rule builder, one convolution on its table, BEV merge
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rule_sites(name):
    """The cells that lvq_voxelize_dynamic ranks for the case (output sites; a submanifold layer ranks its inputs) and their grid."""
    kind, shape, batch = VS.RULE_EXPECTED[name][:3]
    idx, _, _ = VS.rule_cells(name)
    if kind == "merge":
        return np.unique(idx[:, [0, 2, 3]], axis=0), shape[1:]
    if kind == "subm":
        return idx, shape
    stride, padding, _ = KINDS[kind]
    return SC.rules_memo(idx, shape, batch, (3,) * len(shape), stride, padding, False)[0], SC.out_shape(shape, 3, stride, padding, False)


def assert_rule_route(name):
    kind, shape, batch, kcand = VS.RULE_EXPECTED[name][:4]
    idx, _, _ = VS.rule_cells(name)
    sites, oshape = rule_sites(name)
    ls, ns, caps = plan(batch * int(np.prod(oshape)), len(idx) * kcand, False)
    vox, _ = VS.slab_stats(VS.index_keys(sites, oshape), np.ones(len(sites)), ls, ns)
    print(f"{name}: {len(idx) * kcand} candidates, logslab {ls}, {ns} slabs; densest slab {vox.max()} cells of {len(sites)}")
    assert vox.max() > caps[0], (name, int(vox.max()), ls)


@pytest.mark.parametrize("voxel_path", DYN_PATHS)
@pytest.mark.parametrize("name", ["r_subm2d", "r_strided2d", "r_subm3d"])
def test_rules_dense_slab(name, voxel_path, tune):
    """check() of tests/test_gpu_sparse_conv_rules.py (count, output order, the whole table, nothing written behind it) on cell sets
    whose ranked cells put more than DYN_VCAP into one slab: a dense strip under a submanifold 3 x 3, a lattice of odd cells under
    kernel 3 / stride 2 / padding 1 (1024 x 1024 input, 5120 output sites in one slab), a dense sheet under a submanifold 3 x 3 x 3."""
    assert_rule_route(name)
    idx, shape, batch = VS.rule_cells(name)
    tune(voxel_path=voxel_path)
    n_out = check(np.array(idx), shape, batch, VS.RULE_EXPECTED[name][0])
    assert n_out == len(rule_sites(name)[0])


def test_conv_on_a_table_from_an_over_cap_slab():
    """One lvq_sparse_conv layer (16 -> 16, plain bf16) on the strided table as the library built it, against conv_from_table on the
    restated table.  Features in -8 .. 8 and weights in -2 .. 2 are whole numbers: every product and every partial sum is exact in
    bf16 x bf16 -> fp32, so the comparison is an equality."""
    name = "r_strided2d"
    assert_rule_route(name)
    idx, shape, batch = VS.rule_cells(name)
    want_idx, want_nbr = SC.rules_memo(idx, shape, batch, (3, 3), 2, 1, False)
    oi, nbr, _, oshape = B3.sparse_conv_rules(dev(idx), shape, batch, 3, 2, 1, False)
    assert oshape == [512, 512] and np.array_equal(oi.cpu().numpy(), want_idx)
    rng = np.random.default_rng(16)
    feat = rng.integers(-8, 9, size=(len(idx), 16)).astype(np.float32)
    w = rng.integers(-2, 3, size=(16, 3, 3, 16)).astype(np.float32)
    out = run_conv(feat, nbr.cpu().numpy(), w, "bf16")[:len(want_idx)]
    ref = SC.conv_from_table(feat, want_nbr, w)
    assert float(np.abs(ref).max()) > 50 and np.array_equal(out.astype(np.float64), ref)


@pytest.mark.parametrize("voxel_path", DYN_PATHS)
def test_bev_merge_dense_slab(voxel_path, tune):
    """lvq_sparse_bev_merge (bev_out of the VoxelNeXt backbone) whose merged (b, y, x) cells put 5120 into one slab, a third of them
    from two rows; whole-number features, so the row sums are exact and compared as equal."""
    name = "r_merge"
    assert_rule_route(name)
    idx, shape, batch = VS.rule_cells(name)
    feat = np.random.default_rng(17).integers(-8, 9, size=(len(idx), 16)).astype(np.float32)
    want_f, want_idx, want_shape = SC.bev_merge(feat.astype(np.float64), np.asarray(idx, np.int64), shape)
    tune(voxel_path=voxel_path)
    y = bev.bev_out(bev.SparseTensor(dev(feat), dev(idx), shape, batch))
    assert y.spatial_shape == want_shape and y.batch_size == batch
    assert np.array_equal(y.indices.cpu().numpy(), want_idx)
    assert np.array_equal(y.features.cpu().numpy().astype(np.float64), want_f)
