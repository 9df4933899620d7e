"""Inputs that reach the over-cap slab routes of csrc/voxel_binned.hip (numpy only; importable without a GPU).

The slab-binned kernels cut the linear key space into slabs of 2^logslab keys and size them from the MEAN density (choose_cfg:
n / 384 + 1 slabs), so a cloud that is sparse overall and dense in one place gets large slabs, one of which holds the dense place.
One workgroup ranks a slab, and it branches on what the slab holds:

  k_dyn_slab_write   voxels <= DYN_VCAP (4096): per-voxel counters in LDS ("lds"); more: counters in unq_cnt itself ("global")
  k_hard_slab_small  points <= SMALL_PCAP (256): the brute-force kernel ("small")
  k_hard_slab        more points: vfit = voxels <= HARD_VCAP (4096), pfit = points <= HARD_PCAP (8192); whichever fails moves its arrays
                     to global stand-ins ("vfit_pfit", "vfit_pover", "vover_pfit", "vover_pover")

The clouds are built from lists of CELLS, not from random draws: a dense block of cells, scattered cells elsewhere (never in the block's
slab, so the block's slab holds exactly the block), and a multiplicity per cell.  Points sit strictly inside their cells at multiples of
2^-10 m (intensities at multiples of 2^-8), so sums of up to 40 points of a cell are exact in fp32 in any order and a mean over them can
be compared bit for bit.  The rule-builder cell sets follow the same scheme with index rows (b, (z,) y, x).

choose_cfg and the four caps are RESTATED here for the CPU table of tests/test_voxel_slab_cases.py; the GPU tests take both from the
library (lvq_voxel_slab_plan) instead.
"""
import functools

import numpy as np

DYN_VCAP = 4096
HARD_VCAP = 4096
HARD_PCAP = 8192
SMALL_PCAP = 256
MAX_SLABS = 8192

NUSC = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
R54 = (-54.0, -54.0, -5.0, 54.0, 54.0, 3.0)
GRIDS = {
    # name: (point_cloud_range, voxel_size, grid (nx, ny, nz), ndim of the dynamic key)
    "pillar": (NUSC, (0.2, 0.2, 8.0), (512, 512, 1), 2),
    "pillar540": (R54, (0.2, 0.2, 8.0), (540, 540, 1), 2),          # 291 600 keys: the last slab is partial
    "voxel": (NUSC, (0.1, 0.1, 0.2), (1024, 1024, 40), 3),
    "voxel1440": (R54, (0.075, 0.075, 0.2), (1440, 1440, 40), 3),   # 82 944 000 keys: the last slab is partial
}


def choose_cfg(keyspace, n, hard=False):
    """(logslab, nslabs) of voxel_binned.hip's choose_cfg, or None where the binned path does not take the shape."""
    max_ls = 17 if hard else 18
    if keyspace <= 0 or keyspace > (MAX_SLABS << max_ls) or keyspace >= 2 ** 31:
        return None
    want = min(n // 384 + 1, MAX_SLABS)
    ls = 10
    while ls < 17 and ((keyspace + (1 << ls) - 1) >> ls) > want:
        ls += 1
    while ((keyspace + (1 << ls) - 1) >> ls) > MAX_SLABS:
        if ls >= max_ls:
            return None
        ls += 1
    return ls, (keyspace + (1 << ls) - 1) >> ls


def slab_stats(unq_key, unq_cnt, logslab, nslabs):
    """(voxels per slab, points per slab) from the unique keys and their counts."""
    s = np.asarray(unq_key, np.int64) >> logslab
    return (np.bincount(s, minlength=nslabs).astype(np.int64),
            np.bincount(s, weights=np.asarray(unq_cnt, np.float64), minlength=nslabs).astype(np.int64))


def dyn_class(nvox, vcap=DYN_VCAP):
    return "lds" if nvox <= vcap else "global"


def hard_class(nvox, npts, vcap=HARD_VCAP, pcap=HARD_PCAP, small=SMALL_PCAP):
    if npts == 0:
        return "empty"
    if npts <= small:
        return "small"
    return ("vfit" if nvox <= vcap else "vover") + "_" + ("pfit" if npts <= pcap else "pover")


def cell_keys(cells, grid, ndim):
    """Linear keys ((b nx + cx) ny + cy) nz + cz of rows (b, cx, cy, cz); ndim 2 leaves z out."""
    c = np.asarray(cells, np.int64)
    key = (c[:, 0] * grid[0] + c[:, 1]) * grid[1] + c[:, 2]
    return key * grid[2] + c[:, 3] if ndim == 3 else key


def keyspace(grid_name, bs, ndim=None):
    _, _, g, nd = GRIDS[grid_name]
    return bs * g[0] * g[1] * (g[2] if (ndim or nd) == 3 else 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# point clouds
# ---------------------------------------------------------------------------------------------------------------------------------
# name: grid, scenes, dense block (b, cx range, cy range, cz range), extra dense cells, scattered cells, multiplicity of the dense cells,
#       keep slab 0 empty.  Multiplicities: ("const", k) | ("const_plus", k, j): k everywhere, k + 1 in j cells | ("mixed",): 85 % ones, the
#       rest 2 .. 40 with both ends present.  Scattered cells hold one point each.
def _case(grid, bs, block, extra=(), scatter=300, mult=("const", 1), empty0=False):
    return dict(grid=grid, bs=bs, block=block, extra=tuple(extra), scatter=scatter, mult=mult, empty0=empty0)


COLS = lambda b, c0, c1: (b, (c0, c1), (0, 512), (0, 1))                      # full columns of the pillar grid: 512 cells each
SHEET = lambda b, cx, nz: (b, (cx, cx + 1), (0, 1024), (0, nz))                # a 1024 x nz sheet of the 3-D grids
CLOUDS = {
    # ---- dynamic voxeliser: voxels of the densest slab below, at and above DYN_VCAP; where the slab lies; what the counters add ----
    "p_below": _case("pillar", 1, COLS(0, 64, 68), scatter=3000),
    "p_4096": _case("pillar", 1, COLS(0, 64, 72), scatter=1000),
    "p_4097": _case("pillar", 1, COLS(0, 64, 72), extra=[(0, 72, 0, 0)], scatter=1000),
    "p_slab0": _case("pillar", 1, COLS(0, 0, 10)),
    "p_mid_slab0_empty": _case("pillar", 1, COLS(0, 200, 210), empty0=True),
    "p_last_partial": _case("pillar540", 1, (0, (530, 540), (0, 540), (0, 1))),
    "p_mixed": _case("pillar", 1, COLS(0, 32, 42), mult=("mixed",)),
    "p_scene1": _case("pillar", 2, COLS(1, 130, 140)),
    "v_4096": _case("voxel", 1, SHEET(0, 512, 4), scatter=1000),
    "v_4097": _case("voxel", 1, SHEET(0, 512, 4), extra=[(0, 512, 0, 4)], scatter=1000),
    "v_slab0": _case("voxel", 1, SHEET(0, 0, 5)),
    "v_mid_slab0_empty": _case("voxel", 1, SHEET(0, 512, 5), empty0=True),
    "v_last_partial": _case("voxel1440", 1, SHEET(0, 1439, 5)),
    "v_mixed": _case("voxel", 1, SHEET(0, 512, 5), mult=("mixed",)),
    "v_scene1": _case("voxel", 2, SHEET(1, 512, 5)),
    # ---- hard voxeliser: the four (vfit, pfit) classes and both sides of 4096 voxels, 8192 points, 256 points ----
    "h_ordinary": _case("pillar", 1, COLS(0, 64, 68), scatter=3000),
    "h_vover_pfit": _case("pillar", 1, COLS(0, 64, 74), mult=("const_plus", 1, 80)),
    "h_vover_pover": _case("pillar", 1, COLS(0, 64, 74), mult=("const_plus", 2, 60)),
    "h_vfit_pover": _case("pillar", 1, (0, (64, 65), (0, 100), (0, 1)), mult=("const", 90)),
    "h_np_8192": _case("pillar", 1, COLS(0, 64, 72), mult=("const", 2)),
    "h_np_8193": _case("pillar", 1, COLS(0, 64, 72), mult=("const_plus", 2, 1)),
    "h_np_256": _case("pillar", 1, (0, (64, 65), (0, 128), (0, 1)), scatter=5000, mult=("const", 2)),
    "h_np_257": _case("pillar", 1, (0, (64, 65), (0, 128), (0, 1)), scatter=5000, mult=("const_plus", 2, 1)),
    "h_v_vover_pfit": _case("voxel", 1, SHEET(0, 512, 5), mult=("const_plus", 1, 80)),
    "h_v_vover_pover": _case("voxel", 1, SHEET(0, 512, 5), mult=("const_plus", 2, 60)),
    "h_scene1": _case("pillar", 2, COLS(1, 128, 138), mult=("const_plus", 2, 60)),
}
DYN_NAMES = [k for k in CLOUDS if k[0] in "pv"]
# the hard tests also run the 4096 / 4097 pair of the dynamic list (one point per voxel: nvox == np)
HARD_NAMES = ["h_ordinary", "h_vover_pfit", "h_vover_pover", "h_vfit_pover", "p_4096", "p_4097", "h_np_8192", "h_np_8193", "h_np_256",
              "h_np_257", "h_v_vover_pfit", "h_v_vover_pover", "h_scene1"]

# name: (logslab, slab of the dense block, its voxels, its points, dynamic class, hard class) -- written by hand from the geometry above
# (tests/test_voxel_slab_cases.py holds the builders to it; "p_mixed" / "v_mixed" give their point counts as None: seeded draws)
EXPECTED = {
    "p_below": (15, 1, 2048, 2048, "lds", "vfit_pfit"),
    "p_4096": (15, 1, 4096, 4096, "lds", "vfit_pfit"),
    "p_4097": (15, 1, 4097, 4097, "global", "vover_pfit"),
    "p_slab0": (15, 0, 5120, 5120, "global", "vover_pfit"),
    "p_mid_slab0_empty": (15, 3, 5120, 5120, "global", "vover_pfit"),
    "p_last_partial": (15, 8, 5400, 5400, "global", "vover_pfit"),
    "p_mixed": (13, 2, 5120, None, "global", "vover_pover"),
    "p_scene1": (16, 5, 5120, 5120, "global", "vover_pfit"),
    "v_4096": (17, 160, 4096, 4096, "lds", "vfit_pfit"),
    "v_4097": (17, 160, 4097, 4097, "global", "vover_pfit"),
    "v_slab0": (17, 0, 5120, 5120, "global", "vover_pfit"),
    "v_mid_slab0_empty": (17, 160, 5120, 5120, "global", "vover_pfit"),
    "v_last_partial": (17, 632, 5120, 5120, "global", "vover_pfit"),
    "v_mixed": (17, 160, 5120, None, "global", "vover_pover"),
    "v_scene1": (17, 480, 5120, 5120, "global", "vover_pfit"),
    "h_ordinary": (15, 1, 2048, 2048, "lds", "vfit_pfit"),
    "h_vover_pfit": (15, 1, 5120, 5200, "global", "vover_pfit"),
    "h_vover_pover": (14, 2, 5120, 10300, "global", "vover_pover"),
    "h_vfit_pover": (14, 2, 100, 9000, "lds", "vfit_pover"),
    "h_np_8192": (14, 2, 4096, 8192, "lds", "vfit_pfit"),
    "h_np_8193": (14, 2, 4096, 8193, "lds", "vfit_pover"),
    "h_np_256": (15, 1, 128, 256, "lds", "small"),
    "h_np_257": (15, 1, 128, 257, "lds", "vfit_pfit"),
    "h_v_vover_pfit": (17, 160, 5120, 5200, "global", "vover_pfit"),
    "h_v_vover_pover": (17, 160, 5120, 10300, "global", "vover_pover"),
    "h_scene1": (15, 10, 5120, 10300, "global", "vover_pover"),
}


def _mults(spec, k, rng):
    if spec[0] == "const":
        return np.full(k, spec[1], np.int64)
    if spec[0] == "const_plus":
        m = np.full(k, spec[1], np.int64)
        m[rng.permutation(k)[:spec[2]]] += 1
        return m
    assert spec[0] == "mixed"
    m = np.where(rng.random(k) < 0.85, 1, rng.integers(2, 41, size=k))
    m[rng.permutation(k)[:2]] = (1, 40)
    return m.astype(np.int64)


@functools.lru_cache(maxsize=None)
def cloud(name):
    """dict(scenes = [N_s, 4] fp32 per scene (x, y, z, intensity; shuffled), batched = [N, 5] with the scene in column 0 (shuffled as a
    whole), cells [K, 4] (b, cx, cy, cz), mult [K], grid name, range, vsize, grid, ndim, bs, logslab, nslabs, dense_slab).  The arrays
    are shared between tests: do not write to them."""
    spec = CLOUDS[name]
    pcr, vs, grid, ndim = GRIDS[spec["grid"]]
    bs = spec["bs"]
    rng = np.random.default_rng(sum(map(ord, name)))
    b, (x0, x1), (y0, y1), (z0, z1) = spec["block"]
    bx, by, bz = np.meshgrid(np.arange(x0, x1), np.arange(y0, y1), np.arange(z0, z1), indexing="ij")
    dense = np.stack([np.full(bx.size, b), bx.ravel(), by.ravel(), bz.ravel()], axis=1).astype(np.int64)
    if spec["extra"]:
        dense = np.concatenate([dense, np.asarray(spec["extra"], np.int64)])
    mult = _mults(spec["mult"], len(dense), rng)
    n = int(mult.sum()) + spec["scatter"]
    ks = keyspace(spec["grid"], bs)
    logslab, nslabs = choose_cfg(ks, n)
    dslabs = np.unique(cell_keys(dense, grid, ndim) >> logslab)
    assert len(dslabs) == 1, (name, "the dense block straddles slabs", dslabs)
    # scattered cells: distinct keys outside the dense slab (and outside slab 0 where that is to stay empty)
    cand = rng.permutation(ks)[:4 * spec["scatter"] + 64] if ks < (1 << 22) else np.unique(rng.integers(0, ks, size=4 * spec["scatter"] + 64))
    cand = rng.permutation(cand)
    keep = (cand >> logslab) != dslabs[0]
    if spec["empty0"]:
        keep &= (cand >> logslab) != 0
    sk = cand[keep][:spec["scatter"]].astype(np.int64)
    assert len(sk) == spec["scatter"]
    nz = grid[2] if ndim == 3 else 1
    sc = np.stack([sk // (nz * grid[1] * grid[0]), sk // (nz * grid[1]) % grid[0], sk // nz % grid[1], sk % nz], axis=1)
    cells = np.concatenate([dense, sc])
    mult = np.concatenate([mult, np.ones(len(sc), np.int64)])
    # points: a seeded position strictly inside the cell (the middle half of every axis), snapped to 2^-10 m
    pc = np.repeat(cells, mult, axis=0)
    u = rng.uniform(0.25, 0.75, size=(len(pc), 3))
    xyz = np.asarray(pcr[:3]) + (pc[:, 1:4] + u) * np.asarray(vs)
    xyz = np.round(xyz * 1024.0) / 1024.0
    inten = rng.integers(0, 256, size=(len(pc), 1)) / 256.0
    pts = np.concatenate([pc[:, :1].astype(np.float64), xyz, inten], axis=1).astype(np.float32)
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    scenes = [np.ascontiguousarray(pts[pts[:, 0] == s, 1:]) for s in range(bs)]
    for a in [pts] + scenes:
        a.setflags(write=False)
    return dict(name=name, scenes=scenes, batched=pts, cells=cells, mult=mult, grid_name=spec["grid"], range=list(pcr), vsize=tuple(vs),
                grid=list(grid), ndim=ndim, bs=bs, n=n, keyspace=ks, logslab=logslab, nslabs=nslabs, dense_slab=int(dslabs[0]))


def guard_scenes():
    """Two scenes for the guard-band tests of tests/test_gpu_voxel_refcfg.py, which run every case on the pillar grid AND on the 0.1 m
    grid: ten full pillar columns (5120 voxels in one slab of the pillar grid) and a 1024 x 5 sheet (5120 in one slab of the 3-D grid)."""
    return [cloud("p_slab0")["scenes"][0].copy(), cloud("v_mid_slab0_empty")["scenes"][0].copy()]


# ---------------------------------------------------------------------------------------------------------------------------------
# cell sets for the rule builder and the BEV merge: index rows (b, (z,) y, x), keys ((b D + z) H + y) W + x on the OUTPUT grid
# ---------------------------------------------------------------------------------------------------------------------------------
def index_keys(idx, shape):
    idx = np.asarray(idx, np.int64)
    key = idx[:, 0]
    for a, d in enumerate(shape):
        key = key * d + idx[:, 1 + a]
    return key


def _scattered_rows(rng, shape, batch, count, logslab, avoid):
    ks = batch * int(np.prod(shape))
    cand = rng.permutation(np.unique(rng.integers(0, ks, size=4 * count + 64)))
    cand = cand[~np.isin(cand >> logslab, avoid)][:count]
    assert len(cand) == count
    cols = []
    for d in shape[::-1]:
        cols.append(cand % d)
        cand = cand // d
    return np.stack([cand] + cols[::-1], axis=1)


# name: (kind, spatial shape, batch, candidates per input row, logslab of the ranked key space, its dense slab, voxels there)
RULE_EXPECTED = {
    "r_subm2d": ("subm", [512, 512], 1, 1, 15, 1, 5120),              # rows 64 .. 73 of the grid, every column
    "r_strided2d": ("strided", [1024, 1024], 1, 4, 13, 1, 5120),      # output grid 512 x 512; output rows 16 .. 25, every column
    "r_subm3d": ("subm", [41, 1024, 1024], 1, 1, 17, 40, 5120),       # the sheet z = 5, y = 0 .. 4, every x
    "r_merge": ("merge", [4, 512, 512], 2, 1, 15, 9, 5120),           # (b, y, x) cells of scene 1, rows 64 .. 73; z folds away
}


@functools.lru_cache(maxsize=None)
def rule_cells(name):
    """(index rows int32 in a shuffled order, spatial shape, batch).  "r_strided2d" places its dense inputs at ODD (y, x), two apart:
    under kernel 3, stride 2, padding 1 each reaches 2 x 2 output sites and neighbours share them, so 9 x 511 inputs give 10 x 512
    sites -- about as many sites as inputs, where a solid block gives a quarter."""
    kind, shape, batch, kcand, logslab, dslab, _ = RULE_EXPECTED[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "r_subm2d":
        y, x = np.meshgrid(np.arange(64, 74), np.arange(512), indexing="ij")
        dense = np.stack([np.zeros(y.size, np.int64), y.ravel(), x.ravel()], axis=1)
        rows = np.concatenate([dense, _scattered_rows(rng, shape, batch, 300, logslab, [dslab])])
    elif name == "r_strided2d":
        y, x = np.meshgrid(2 * np.arange(16, 25) + 1, 2 * np.arange(511) + 1, indexing="ij")
        dense = np.stack([np.zeros(y.size, np.int64), y.ravel(), x.ravel()], axis=1)
        # scattered inputs: cells of the OUTPUT grid outside the dense slab and its neighbours, doubled (even coordinates: one site each)
        sc = _scattered_rows(rng, [512, 512], batch, 100, logslab, [dslab - 1, dslab, dslab + 1])
        sc[:, 1:] *= 2
        rows = np.concatenate([dense, sc])
    elif name == "r_subm3d":
        y, x = np.meshgrid(np.arange(5), np.arange(1024), indexing="ij")
        dense = np.stack([np.zeros(y.size, np.int64), np.full(y.size, 5), y.ravel(), x.ravel()], axis=1)
        rows = np.concatenate([dense, _scattered_rows(rng, shape, batch, 300, logslab, [dslab])])
    else:
        assert name == "r_merge"
        # every cell of the strip at z = 0 or 1, a third of them at z = 2 as well (rows that merge), scattered rows elsewhere
        y, x = np.meshgrid(np.arange(64, 74), np.arange(512), indexing="ij")
        z = rng.integers(0, 2, size=y.size)
        dense = np.stack([np.ones(y.size, np.int64), z, y.ravel(), x.ravel()], axis=1)
        twice = dense[rng.random(len(dense)) < 1.0 / 3.0].copy()
        twice[:, 1] = 2
        sc = _scattered_rows(rng, shape[1:], batch, 300, logslab, [dslab])
        sc = np.concatenate([sc[:, :1], rng.integers(0, shape[0], size=(len(sc), 1)), sc[:, 1:]], axis=1)
        rows = np.concatenate([dense, twice, sc])
    rows = np.ascontiguousarray(rows[rng.permutation(len(rows))].astype(np.int32))
    rows.setflags(write=False)
    return rows, list(shape), batch
