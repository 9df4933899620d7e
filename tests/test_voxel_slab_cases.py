"""CPU check of tests/voxel_slab_cases.py: every named case lands in the slab class its GPU test names.

The table (voxel_slab_cases.EXPECTED / RULE_EXPECTED) was written by hand from the geometry of each case; the classes are formed here
from the restated constants 4096 / 8192 / 256 and the restated choose_cfg, on the keys the CPU oracle gives the points.  A case that
silently becomes ordinary -- a cloud resized, a block moved across a slab edge, choose_cfg changed -- fails here, without a GPU.
(The GPU tests make the same assertion from lvq_voxel_slab_plan; test_restated_plan_is_the_library's holds the two together.)"""
import ctypes
import os

import numpy as np
import pytest

import sparse_conv_cases as SC
import voxel_slab_cases as VS
from oracle import lidar_oracle as LO


def oracle_slabs(name):
    c = VS.cloud(name)
    o = LO.dynamic_voxelize(c["batched"], c["range"], c["vsize"], c["grid"], c["ndim"])
    assert o["keep"].all(), "a point fell outside its grid"
    return c, o, VS.slab_stats(o["unq_key"], o["unq_cnt"], c["logslab"], c["nslabs"])


@pytest.mark.parametrize("name", list(VS.CLOUDS))
def test_cloud_lands_in_its_class(name):
    c, o, (vox, pts) = oracle_slabs(name)
    logslab, slab, nvox, npts, dclass, hclass = VS.EXPECTED[name]
    assert 5000 <= c["n"] <= 70000 and len(c["batched"]) == c["n"]
    # the oracle's cells are the cells the points were built for, with the multiplicities asked for
    order = np.argsort(VS.cell_keys(c["cells"], c["grid"], c["ndim"]))
    assert np.array_equal(o["unq_key"], VS.cell_keys(c["cells"], c["grid"], c["ndim"])[order])
    assert np.array_equal(o["unq_cnt"], c["mult"][order])
    assert (c["logslab"], c["dense_slab"]) == (logslab, slab)
    assert VS.choose_cfg(c["keyspace"], c["n"], hard=True) == (c["logslab"], c["nslabs"])       # one plan for both voxelisers
    assert vox[slab] == nvox and (npts is None or pts[slab] == npts)
    assert VS.dyn_class(vox[slab]) == dclass and VS.hard_class(vox[slab], pts[slab]) == hclass
    print(f"{name}: logslab {logslab}, {c['nslabs']} slabs, n {c['n']}; slab {slab}: {vox[slab]} voxels, {pts[slab]} points")
    # the dense slab is the only one of its kind: every other slab is ordinary for both voxelisers
    others = np.arange(c["nslabs"]) != slab
    assert vox[others].max() < VS.DYN_VCAP // 2 and pts[others].max() < VS.HARD_PCAP // 2
    if VS.CLOUDS[name]["empty0"]:
        assert pts[0] == 0 and slab != 0


def test_the_table_covers_what_the_issue_names():
    """Dynamic: below, at and above 4096; hard: all four (vfit, pfit) classes, both sides of 256 and 8192 points and of 4096 voxels;
    the dense slab first, last (partial) and in the middle behind an empty slab 0; a second scene; multiplicities 1 and 1 .. 40."""
    E = VS.EXPECTED
    dyn = {n: E[n] for n in VS.DYN_NAMES}
    assert {2048, 4096, 4097, 5120} <= {e[2] for e in dyn.values()}
    assert {e[4] for e in dyn.values()} == {"lds", "global"}
    hard = {n: E[n] for n in VS.HARD_NAMES}
    assert {e[5] for e in hard.values()} == {"small", "vfit_pfit", "vfit_pover", "vover_pfit", "vover_pover"}
    assert {(e[2], e[3]) for e in hard.values()} >= {(4096, 4096), (4097, 4097), (4096, 8192), (4096, 8193), (128, 256), (128, 257)}
    for g in ("p", "v"):
        assert E[g + "_slab0"][1] == 0 and E[g + "_mid_slab0_empty"][1] > 0 and VS.CLOUDS[g + "_mid_slab0_empty"]["empty0"]
        c = VS.cloud(g + "_last_partial")
        assert c["dense_slab"] == c["nslabs"] - 1 and c["keyspace"] % (1 << c["logslab"]) != 0
        assert VS.CLOUDS[g + "_scene1"]["bs"] == 2 and VS.CLOUDS[g + "_scene1"]["block"][0] == 1
        m = VS.cloud(g + "_mixed")["mult"]
        assert m.min() == 1 and m.max() == 40 and (m[:5120] > 1).sum() > 500
    assert all(VS.CLOUDS[n]["mult"] == ("const", 1) for n in VS.DYN_NAMES if not n.endswith("_mixed"))


def test_guard_scenes_are_over_cap_on_both_grids():
    scenes = VS.guard_scenes()
    bpts = np.concatenate([np.pad(p, ((0, 0), (1, 0)), constant_values=s) for s, p in enumerate(scenes)]).astype(np.float32)
    for gname in ("pillar", "voxel"):
        pcr, vs, grid, ndim = VS.GRIDS[gname]
        o = LO.dynamic_voxelize(bpts, pcr, vs, grid, ndim)
        logslab, nslabs = VS.choose_cfg(VS.keyspace(gname, 2), len(bpts))
        vox, pts = VS.slab_stats(o["unq_key"], o["unq_cnt"], logslab, nslabs)
        assert vox.max() == 5120 > VS.DYN_VCAP and (vox > VS.DYN_VCAP).sum() == 1, (gname, vox.max())
        # hard, three dimensions always (nz = 1 on the pillar grid: the same keys)
        assert VS.hard_class(vox.max(), pts[vox.argmax()]).startswith("vover")


@pytest.mark.parametrize("name", list(VS.RULE_EXPECTED))
def test_rule_cells_land_in_their_class(name):
    kind, shape, batch, kcand, logslab, dslab, nvox = VS.RULE_EXPECTED[name]
    idx, shape2, batch2 = VS.rule_cells(name)
    assert (shape2, batch2) == (shape, batch) and len(np.unique(idx, axis=0)) == len(idx)
    n = len(idx) * kcand
    assert 5000 <= n <= 70000
    if kind == "merge":
        oshape = shape[1:]
        sites = np.unique(idx[:, [0, 2, 3]], axis=0)
        assert len(sites) < len(idx)                                             # rows do merge
    elif kind == "subm":
        oshape, sites = shape, idx
    else:
        oshape = SC.out_shape(shape, 3, 2, 1, False)
        sites, _ = SC.rules(idx, shape, batch, (3,) * len(shape), 2, 1, False)
    plan = VS.choose_cfg(batch * int(np.prod(oshape)), n)
    keys = VS.index_keys(sites, oshape)
    vox, _ = VS.slab_stats(keys, np.ones(len(keys)), *plan)
    print(f"{name}: n {n}, logslab {plan[0]}, {plan[1]} slabs; slab {dslab}: {vox[dslab]} cells of {len(sites)}")
    assert plan[0] == logslab and vox[dslab] == nvox > VS.DYN_VCAP and vox.argmax() == dslab
    assert np.sort(vox)[-2] < VS.DYN_VCAP // 2


def test_restated_plan_is_the_librarys():
    """voxel_slab_cases.choose_cfg and the four constants against lvq_voxel_slab_plan (host only) on the shapes of every case and a sweep."""
    from lidar_vision_vqa_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = _ffi.lib()
    shapes = [(VS.cloud(n)["keyspace"], VS.cloud(n)["n"]) for n in VS.CLOUDS]
    rng = np.random.default_rng(0)
    shapes += [(int(k), int(n)) for k, n in zip(2 ** rng.uniform(0, 31, 300), 2 ** rng.uniform(0, 24, 300))]
    shapes += [(1 << 30, 1), ((1 << 30) + 1, 10 ** 6), ((1 << 31) - 1, 5000), (1, 0), (1 << 27, 1), ((8192 << 17) + 1, 1)]
    for ks, n in shapes:
        for hard in (0, 1):
            ls, ns, caps = ctypes.c_int(-1), ctypes.c_int(-1), (ctypes.c_int * 4)()
            rc = L.lvq_voxel_slab_plan(ks, n, hard, ctypes.byref(ls), ctypes.byref(ns), caps)
            want = VS.choose_cfg(ks, n, bool(hard))
            if want is None:
                assert rc == -5 and ls.value == -1, (ks, n, hard)
            else:
                assert rc == 0 and (ls.value, ns.value) == want, (ks, n, hard)
                assert list(caps) == [VS.DYN_VCAP, VS.HARD_VCAP, VS.HARD_PCAP, VS.SMALL_PCAP]
