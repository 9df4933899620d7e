"""Scenes and operands of tests/test_gpu_bev_tile_kernels.py, host side only (numpy): the GPU file runs them, tests/test_oracle_bev_tiles.py
checks on the CPU that the tie rule of oracle/bev_tiles_oracle.py leaves the tight bound in force on (almost) every row of every case.

Scenes (sizes from the dispatch arithmetic of csrc/bev_tiles.hip; grid = 2 x min(CUs, cap_tiles) for the K|V kernels):
  S1   B = 1, 24 x 24: 9 tiles -> grid 18, not a multiple of 16: the branch without the XCD partition.  The four image corners, a pillar on
       an interior tile corner (8, 8) that dirties cells of four tiles, the full left edge of tile (1, 2), 12 more; three trailing pillar
       rows beyond n_live that must be ignored.
  S2   B = 3, 40 x 16, scene 1 empty: 30 tiles -> grid 60.  H != W; cell (13, 5) holds a pillar in scenes 0 and 2 with different
       features; the features of scene 2 are scaled by 1e-3 (t ~ GELU(b9), c0 and eps decide rstd).
  S3   B = 2, 16 x 32: 16 tiles -> grid 32, the XCD-partitioned branch with fewer than 8 row groups (empty slices, a partial group).
       Runs with b9 = NULL.
  S3b  B = 2, 32 x 32: 32 tiles -> grid 64, the same branch with two workgroups per slice and column half.
  S4*  the live list of S1 with every cell forced dirty, cut on the host to (live pieces, dirty rows) = (1, 5), (7, 16), (9, 63),
       (15, 64), (9, 65): live pieces % 8 in {1, 7}, rows around the 16- and 64-row groups.  (A pillar set cannot give 5 dirty rows -- a
       union of clipped 3 x 3 windows has 4, 6, 8, 9, ... cells -- so the lists, which are plain inputs of the entry points, are cut.)
       S4z is S1 with n_live = 0: nothing is live, nothing may be written.
  S5   force_all on B scenes of 64 x 64 with B = 2 CUs / 64 + 1: more than 2 x CUs groups, so workgroups run 3 and 2 groups.  The features
       of scene 1 are scaled by 30 (rstd is small)."""
import functools

import numpy as np

from lidar_vision_vqa_amd import synth
from oracle import bev_tiles_oracle as BO

C = 64
EPS = 1e-5
C0 = 0.7
B9_SEED = 23                     # GELU(b9) -- the token of every clean cell -- has no channel near a bf16 midpoint (test_oracle_bev_tiles)
NS = (256, 512, 768, 1024)
MAX_KEYS = 64 * 64


def _cells(B, H, W, fixed, n_random, seed):
    """(scene, y, x) list: `fixed` first, then n_random more distinct cells drawn from `seed` (in scenes that have a fixed cell)."""
    rng = np.random.default_rng(seed)
    scenes = sorted({c[0] for c in fixed})
    have = set(fixed)
    out = list(fixed)
    while len(out) < len(fixed) + n_random:
        c = (scenes[int(rng.integers(len(scenes)))], int(rng.integers(H)), int(rng.integers(W)))
        if c not in have:
            have.add(c)
            out.append(c)
    return out


# The feature seeds below (3001, 3002, 3000, 3002) are chosen on the CPU, from the reference alone, so that no row of S1 .. S4 has three or
# more channels near a bf16 midpoint (tests/test_oracle_bev_tiles.py).
def _scene(name, B, H, W, cells, seed, trailing=0, scale=None, use_b9=True, force_all=False):
    coords = np.array([(s, 0, y, x) for s, y, x in cells], np.int32).reshape(-1, 4)
    feat = synth.randn((len(cells), C), seed)
    for s, f in (scale or {}).items():
        feat[coords[:, 0] == s] *= np.float32(f)
    return dict(name=name, B=B, H=H, W=W, coords=coords, feat=feat, n_live=len(cells) - trailing, use_b9=use_b9, force_all=force_all, cut=None)


@functools.lru_cache(maxsize=None)
def scene(name, cus=256):
    if name == "S1" or name.startswith("S4"):
        fixed = [(0, 0, 0), (0, 0, 23), (0, 23, 0), (0, 23, 23), (0, 8, 8)] + [(0, y, 16) for y in range(8, 16)]
        cells = _cells(1, 24, 24, fixed, 12 + 3, 301)
        sc = _scene(name, 1, 24, 24, cells, 3001, trailing=3)
        if name == "S4z":
            sc["n_live"] = 0
        elif name != "S1":
            sc["force_all"] = True
            sc["cut"] = dict(S4a=(1, 5), S4b=(7, 16), S4c=(9, 63), S4d=(15, 64), S4e=(9, 65))[name]
        return sc
    if name == "S2":
        fixed = [(0, 13, 5), (2, 13, 5), (0, 0, 0), (2, 39, 15), (0, 39, 0), (2, 7, 8)]
        return _scene(name, 3, 40, 16, _cells(3, 40, 16, fixed, 12, 311), 3002, scale={2: 1e-3})
    if name == "S2s0":                                            # scene 0 of S2 on its own
        full = scene("S2")
        keep = full["coords"][:, 0] == 0
        sc = dict(full, name=name, B=1, coords=full["coords"][keep].copy(), feat=full["feat"][keep].copy(), n_live=int(keep.sum()))
        return sc
    if name == "S2f":                                             # S2 with every cell forced dirty
        return dict(scene("S2"), name=name, force_all=True)
    if name == "S2e":                                             # one empty 40 x 16 scene, every cell forced dirty: the per-model table
        return _scene(name, 1, 40, 16, [], 313, force_all=True)
    if name == "S3":
        return _scene(name, 2, 16, 32, _cells(2, 16, 32, [(0, 3, 3), (1, 15, 31)], 18, 321), 3000, use_b9=False)
    if name == "S3b":
        return _scene(name, 2, 32, 32, _cells(2, 32, 32, [(0, 3, 3), (1, 31, 0)], 22, 331), 3002)
    if name == "S5":
        B = 2 * cus // 64 + 1
        fixed = [(s, 5 + 6 * s % 50, 9 + 11 * s % 50) for s in range(B)]
        return _scene(name, B, 64, 64, _cells(B, 64, 64, fixed, 4 * B, 341), 342, scale={1: 30.0}, force_all=True)
    if name == "S5e":                                             # the table of S5: one empty 64 x 64 scene
        return _scene(name, 1, 64, 64, [], 343, force_all=True)
    raise KeyError(name)


def cut_lists(codes, pdirty, pieces, rows):
    """The first `pieces` live pieces with their masks trimmed (highest bits first, from the last piece backwards) to `rows` dirty rows."""
    codes = list(codes[:pieces])
    cnt = [bin(m).count("1") for _, m in pdirty[:pieces]]
    assert pieces <= rows <= sum(cnt), (pieces, rows, sum(cnt))
    i = pieces - 1
    while sum(cnt) > rows:
        if cnt[i] > 1:
            cnt[i] -= 1
        else:
            i -= 1
    out, nd = [], 0
    for (_, m), c in zip(pdirty[:pieces], cnt):
        bits = [j for j in range(8) if (m >> j) & 1][:c]
        out.append((nd, sum(1 << j for j in bits)))
        nd += c
    return codes, out, (pieces, 8 * pieces, rows)


@functools.lru_cache(maxsize=None)
def prepared(name, cus=256):
    """A scene with everything the references need: occupancy, index map, bookkeeping lists, the compact rows and their fp64 conv tokens."""
    sc = dict(scene(name, cus))
    B, H, W = sc["B"], sc["H"], sc["W"]
    nl = sc["n_live"]
    co = sc["coords"][:nl]
    occ = np.zeros((B, H, W), bool)
    occ[co[:, 0], co[:, 2], co[:, 3]] = True
    idx = np.full((B, H, W), -1, np.int32)
    idx[co[:, 0], co[:, 2], co[:, 3]] = np.arange(nl, dtype=np.int32)
    codes, pdirty, row_src, counts = BO.bookkeeping(occ, 0, force_all=sc["force_all"])
    if sc["cut"]:
        codes, pdirty, counts = cut_lists(codes, pdirty, *sc["cut"])
        row_src = None
    w9, b9 = conv_weights()
    t, mag = BO.conv_tokens(sc["feat"][:nl], co, B, H, W, w9, b9 if sc["use_b9"] else None)
    rows = BO.rows_of(codes, pdirty, B, H, W)
    sc.update(occ=occ, idx=idx, codes=codes, pdirty=pdirty, row_src=row_src, counts=counts, rows=rows, t=t, mag=mag,
              t_rows=t[rows["s"], rows["y"], rows["x"]], mag_rows=mag[rows["s"], rows["y"], rows["x"]],
              dirty=BO.dirty_cells(occ)[rows["s"], rows["y"], rows["x"]])
    return sc


@functools.lru_cache(maxsize=None)
def conv_weights():
    return synth.randn((C, 9), 22, 0.3), synth.randn((C,), B9_SEED)


@functools.lru_cache(maxsize=4)
def kv_operands(n):
    """fp32 operands of lvq_bev_tile_kv, drawn directly: M, R ~ N(0, 1/64); m0, r0, T ~ N(0, 1); c0 = 0.7, eps = 1e-5, d_ln = n."""
    return dict(M=synth.randn((2 * n, C), 400 + n, 0.125), m0=synth.randn((2 * n,), 401 + n), R=synth.randn((C, C), 402 + n, 0.125),
                r0=synth.randn((C,), 403 + n), T=synth.randn((MAX_KEYS, 2 * n), 404 + n))


@functools.lru_cache(maxsize=4)
def token_operands(n):
    """fp32 operands of lvq_bev_tile_tokens: Wp ~ 0.15 N(0, 1); bias, beta, PE ~ N(0, 1); gamma ~ 1 + N(0, 1)."""
    return dict(Wp=synth.randn((n, C), 500 + n, 0.15), bias=synth.randn((n,), 501 + n), gamma=1.0 + synth.randn((n,), 502 + n),
                beta=synth.randn((n,), 503 + n), PE=synth.randn((MAX_KEYS, n), 504 + n))


ROUTE_SCENES = ("S1", "S2", "S3", "S3b", "S4a", "S4b", "S4c", "S4d", "S4e", "S4z")
ALL_SCENES = ROUTE_SCENES + ("S2s0", "S2f", "S2e", "S5", "S5e")
