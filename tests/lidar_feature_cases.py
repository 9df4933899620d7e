"""fp64 restatements, first-order fp32 error bounds, fp32 emulations in the kernels' operation order, and seeded case builders for the fp32
feature kernels between the voxeliser and the key stream (csrc/vfe.hip, csrc/elementwise.hip: dwconv family, csrc/bev_bridge.hip:
lvq_sparse_to_dense).  numpy only: tests/test_lidar_feature_restatements.py runs all of it on the CPU, tests/test_gpu_lidar_feature_kernels.py
holds the kernels to it.

Bounds (u = 2^-24; every arithmetic assertion on the GPU is 2 x bound per element, the fp32 emulation must stay within 1 x bound):
  PFN input features   cluster (T + 1) u sum_j |x_j| / n + u |f|   (T-term fp32 sum and a divide, then one subtraction)
                       centre  2 u (|cell * vs| + |off|) + u |f|    distance 3 u |f|    raw columns 0
  PFN layer, channel o (sum_k |w_ok| df_k + (cin + 1) u sum_k |w_ok| |f_k|) |scale_o| + 2 u (|acc_o scale_o| + |shift_o|)
                       carried through relu and max (1-Lipschitz) into the next layer's [x, x_max]
  scatter_mean         (n_v + 1) u sum |x| / n_v
  dwconv + GELU        a = 11 u (|bias| + sum |tap * w|);  1.13 a + 2 u |y|, + 2^-8 |y| (hi alone) or 2^-16 |y| (hi + lo):
                       bf16 keeps 8 significant bits, so round-to-nearest is off by up to 2^-8 |y|, and lo = bf16(y - hi) by 2^-8 of that
                       (a first draft had 2^-9 / 2^-17; the fp32 emulation reaches 1.99 x that at hi alone)

Reference file:line citations are those of include/lvq.h (relative to the reference's src/lidar-encoder/pcdet/models unless a path says otherwise)."""
import functools
import math

import numpy as np

U = 2.0 ** -24
F32, F64 = np.float32, np.float64

# 0.2 m pillars over +-51.2 m (cbgs_pp_multihead.yaml), 16 z cells of 0.5 m so that the per-cell z centre of kind 1 / coords[:, 1] is exercised
VS = np.array([0.2, 0.2, 0.5], F32)
LO = np.array([-51.2, -51.2, -5.0], F32)
OFF = (VS / F32(2) + LO).astype(F32)                       # offset = vsize / 2 + range_lo, formed in fp32 by the caller (include/lvq.h)
GRID = (512, 512, 16)


def f32(a):
    return np.asarray(a, F32)


def fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in fp64, the sum is rounded to fp64 and then to fp32."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------
# MeanVFE  (backbones_3d/vfe/mean_vfe.py:25-29)
# ------------------------------------------------------------------------------------------------------------------------------
def mean_vfe(voxels, num):
    """mean_vfe.py:25-29 in fp64: sum over ALL T slots / clamp(num_points, 1)."""
    return np.asarray(voxels, F64).sum(axis=1) / np.maximum(np.asarray(num, F64), 1.0)[:, None]


def mean_vfe_f32(voxels, num):
    """k_mean_vfe's fp32 sequence: s = 0; s += slot j for j = 0..T-1; one divide by max(n, 1).  The kernel is bit-identical to this."""
    v = f32(voxels)
    s = np.zeros((v.shape[0], v.shape[2]), F32)
    for j in range(v.shape[1]):
        s = (s + v[:, j, :]).astype(F32)
    return (s / np.maximum(num, 1).astype(F32)[:, None]).astype(F32)


def mean_case(m, t, c, seed, extra=9):
    """[m + extra, t, c] slots of which the first m rows are live; every slot (padding included) holds a value, as the sum runs over all
    T slots; num_points includes 0 (the clamp) when there is room."""
    rng = np.random.default_rng(seed)
    cap = m + extra
    vox = (rng.standard_normal((cap, t, c)) * 20.0).astype(F32)
    num = rng.integers(1, t + 1, cap).astype(np.int32)
    if m >= 3:
        num[1] = 0
    return dict(voxels=vox, num=num, m=m, cap=cap, t=t, c=c)


# ------------------------------------------------------------------------------------------------------------------------------
# PillarVFE + PFNLayer  (backbones_3d/vfe/pillar_vfe.py:8-49, 94-123)
# ------------------------------------------------------------------------------------------------------------------------------
def pfn_cin(c, flags):
    return (c if flags & 1 else c - 3) + 6 + (1 if flags & 2 else 0)


def pillar_features(voxels, num, coords, flags, vs=VS, off=OFF):
    """pillar_vfe.py:94-120 in fp64: [voxel_features | features[..., 3:]], f_cluster (mean over all T slots / num_points), f_center
    (coords (b, z, y, x): x from column 3, y from 2, z from 1), the optional norm, then the padding mask on the INPUTS.
    Returns (f [M, T, cin], df)."""
    v = np.asarray(voxels, F64)
    n = np.asarray(num, F64)
    m, t, c = v.shape
    vs, off = np.asarray(vs, F64), np.asarray(off, F64)
    xyz = v[:, :, :3]
    mean = xyz.sum(axis=1, keepdims=True) / n[:, None, None]
    cl = xyz - mean
    d_cl = (t + 1) * U * np.abs(xyz).sum(axis=1, keepdims=True) / n[:, None, None] + U * np.abs(cl)
    cell = np.asarray(coords, F64)[:, [3, 2, 1]]
    ctr = cell * vs + off
    ce = xyz - ctr[:, None, :]
    d_ce = 2 * U * (np.abs(cell * vs) + np.abs(off))[:, None, :] + U * np.abs(ce)
    base = v if flags & 1 else v[:, :, 3:]
    parts, dparts = [base, cl, ce], [np.zeros_like(base), d_cl, d_ce]
    if flags & 2:
        dist = np.sqrt((xyz * xyz).sum(axis=2, keepdims=True))
        parts.append(dist)
        dparts.append(3 * U * dist)
    f, df = np.concatenate(parts, axis=2), np.concatenate(dparts, axis=2)
    mask = (np.arange(t)[None, :] < np.asarray(num)[:, None])[:, :, None]
    return f * mask, df * mask


def pillar_features_f32(voxels, num, coords, flags, fast, vs=VS, off=OFF):
    """The kernels' fp32 sequence.  Generic (k_pillar_vfe): sequential sum over j = 0..T-1; fast (k_pillar_vfe1): xor butterfly over 32
    lanes (slots >= T hold zero).  Centre = cell * vs (rounded) + off (rounded); distance = sqrt((x x + y y) + z z)."""
    v = f32(voxels)
    m, t, c = v.shape
    vs, off = f32(vs), f32(off)
    xyz = v[:, :, :3]
    if fast:
        s = np.zeros((m, 32, 3), F32)
        s[:, :t] = xyz
        lane = np.arange(32)
        for o in (1, 2, 4, 8, 16):
            s = (s + s[:, lane ^ o]).astype(F32)
        s = s[:, 0]
    else:
        s = np.zeros((m, 3), F32)
        for j in range(t):
            s = (s + xyz[:, j]).astype(F32)
    mean = (s / np.asarray(num).astype(F32)[:, None]).astype(F32)
    cl = (xyz - mean[:, None, :]).astype(F32)
    cell = np.asarray(coords)[:, [3, 2, 1]].astype(F32)
    ctr = ((cell * vs).astype(F32) + off).astype(F32)
    ce = (xyz - ctr[:, None, :]).astype(F32)
    parts = [v if flags & 1 else v[:, :, 3:], cl, ce]
    if flags & 2:
        sq = (xyz * xyz).astype(F32)
        parts.append(np.sqrt(((sq[..., 0] + sq[..., 1]).astype(F32) + sq[..., 2]).astype(F32)).astype(F32)[..., None])
    f = np.concatenate(parts, axis=2).astype(F32)
    mask = (np.arange(t)[None, :] < np.asarray(num)[:, None])[:, :, None]
    return np.where(mask, f, F32(0))


def pfn_layer(f, df, w, scale, shift, affine_u=2.0, affine_extra=0.0):
    """One linear + folded BatchNorm + ReLU (pillar_vfe.py:28-44 / dynamic_pillar_vfe.py:35-43) on rows f [..., cin] in fp64 with the
    layer bound of the module docstring.  affine_u / affine_extra widen the affine term for a subject that evaluates the BatchNorm
    unfolded (the torch oracle)."""
    w, scale, shift = np.asarray(w, F64), np.asarray(scale, F64), np.asarray(shift, F64)
    cin = w.shape[1]
    acc = f @ w.T
    y = acc * scale + shift
    aw = np.abs(w).T
    dy = (df @ aw + (cin + 1) * U * (np.abs(f) @ aw)) * np.abs(scale) + affine_u * U * (np.abs(acc * scale) + np.abs(shift) + affine_extra)
    return np.maximum(y, 0.0), dy


def pfn_layer_f32(f, w, scale, shift):
    """acc = 0; acc = fmaf(f_k, w_k, acc) for k ascending; y = max(acc * scale (rounded) + shift, 0): -ffp-contract=off."""
    f, w = f32(f), f32(w)
    acc = np.zeros(f.shape[:-1] + (w.shape[0],), F32)
    for k in range(w.shape[1]):
        acc = fma32(f[..., k, None], w[:, k], acc)
    y = ((acc * f32(scale)).astype(F32) + f32(shift)).astype(F32)
    return np.maximum(y, F32(0))


def pillar_vfe(voxels, num, coords, layers, flags, vs=VS, off=OFF, affine=None):
    """PillarVFE.forward (pillar_vfe.py:94-123) in fp64 -> (pillar_features [M, cout_last], bound).  layers: [(w, scale, shift)].
    Every one of the T slots takes part in the max-pool of every layer: a padded slot contributes relu(shift) (the mask is on the
    inputs, pillar_vfe.py:117-120), and non-final layers hand [x, x_max] on (pillar_vfe.py:46-49)."""
    f, df = pillar_features(voxels, num, coords, flags, vs, off)
    for l, (w, sc, sh) in enumerate(layers):
        kw = {} if affine is None else dict(affine_u=affine[l][0], affine_extra=affine[l][1])
        y, dy = pfn_layer(f, df, w, sc, sh, **kw)
        mx, dmx = y.max(axis=1, keepdims=True), dy.max(axis=1, keepdims=True)
        if l == len(layers) - 1:
            return mx[:, 0], dmx[:, 0]
        f = np.concatenate([y, np.broadcast_to(mx, y.shape)], axis=2)
        df = np.concatenate([dy, np.broadcast_to(dmx, dy.shape)], axis=2)


def pillar_vfe_f32(voxels, num, coords, layers, flags, fast, vs=VS, off=OFF):
    f = pillar_features_f32(voxels, num, coords, flags, fast, vs, off)
    for l, (w, sc, sh) in enumerate(layers):
        y = pfn_layer_f32(f, w, sc, sh)
        mx = y.max(axis=1, keepdims=True)
        if l == len(layers) - 1:
            return mx[:, 0]
        f = np.concatenate([y, np.broadcast_to(mx, y.shape)], axis=2)


def pfn_params(cin, couts, seed, norm=True):
    """[(w, scale, shift)] with cin_l = 2 cout_{l-1}.  norm=False is the USE_NORM=False form: scale 1, shift = linear bias of both signs."""
    rng = np.random.default_rng(seed)
    layers = []
    for co in couts:
        w = (rng.standard_normal((co, cin)) / np.sqrt(cin)).astype(F32)
        scale = (0.5 + rng.random(co)).astype(F32) if norm else np.ones(co, F32)
        shift = (0.5 * rng.standard_normal(co)).astype(F32)
        layers.append((w, scale, shift))
        cin = 2 * co
    return layers


def cell_points(rng, cells_xyz, c):
    """One fp32 point [x, y, z, intensity, extra...] inside each of the given (cx, cy, cz) cells."""
    cells = np.asarray(cells_xyz, F64)
    xyz = LO.astype(F64) + (cells + rng.random(cells.shape)) * VS.astype(F64)
    rest = rng.random(cells.shape[:-1] + (c - 3,))
    return np.concatenate([xyz, rest], axis=-1).astype(F32)


@functools.lru_cache(maxsize=None)
def pillar_case(m, t, c, couts, flags, seed, norm=True, extra=13):
    """m live pillars in a buffer of m + extra (the rows behind the live count hold ordinary pillars: if the kernel ran them, the output
    pattern would go).  num_points cycles through {1, 2, T - 1, T}; row 0 sits at cell (0, 0), row 1 at the last cell.  Holds the fp64
    value and bound of the live rows, and asserts what the case exists for."""
    rng = np.random.default_rng(seed)
    cap = m + extra
    num = np.array([max(1, min(t, (1, 2, t - 1, t)[i % 4])) for i in range(cap)], np.int32)
    cells = np.stack([rng.integers(0, GRID[0], cap), rng.integers(0, GRID[1], cap), rng.integers(0, GRID[2], cap)], axis=1)
    cells[0, :2] = 0
    if cap > 1:
        cells[1, :2] = (GRID[0] - 1, GRID[1] - 1)
    coords = np.stack([rng.integers(0, 2, cap), cells[:, 2], cells[:, 1], cells[:, 0]], axis=1).astype(np.int32)
    vox = cell_points(rng, np.repeat(cells[:, None, :], t, axis=1), c)
    vox[np.arange(t)[None, :] >= num[:, None]] = 0.0             # the voxeliser leaves padding slots zero
    layers = pfn_params(pfn_cin(c, flags), couts, seed + 1, norm)
    # channel 0 of the first layer reads the (non-negative) intensity alone, with a negative weight and a positive shift: every live
    # slot lies below relu(shift), so the pad value is this channel's maximum wherever there is padding and must stay out where there is none
    layers[0][0][0, :] = 0.0
    layers[0][0][0, 3 if flags & 1 else 0] = -0.7
    layers[0][2][0] = 0.3
    ref, bound = pillar_vfe(vox[:m], num[:m], coords[:m], layers, flags)
    case = dict(voxels=vox, num=num, coords=coords, m=m, cap=cap, t=t, c=c, layers=layers, flags=flags, ref=ref, bound=bound,
                couts=tuple(couts))
    check_pillar_case(case)
    return case


def check_pillar_case(case):
    """(a) some (pillar, channel) attains its maximum on a padded slot; (b) some pillar has num_points == T and a channel where the pad
    value relu(shift) WOULD win by more than the bar if it were let in.  (Single-layer cases; (a) needs a pillar with padding, (b) one
    without: m >= 4 guarantees both when T >= 2.)"""
    m, t, num = case["m"], case["t"], case["num"][:case["m"]]
    assert (case["ref"] >= 0).all() and np.isfinite(case["bound"]).all()
    if len(case["layers"]) != 1 or m < 4:
        return
    f, df = pillar_features(case["voxels"][:m], num, case["coords"][:m], case["flags"])
    y, dy = pfn_layer(f, df, *case["layers"][0])
    live = np.arange(t)[None, :, None] < num[:, None, None]
    live_max = np.where(live, y, -np.inf).max(axis=1)
    pad = np.maximum(np.asarray(case["layers"][0][2], F64), 0.0)[None, :]
    margin = 4 * case["bound"]
    if t >= 2:
        assert ((num < t)[:, None] & (pad > live_max + margin)).any(), "no maximum comes from a padded slot"
    full = num == t
    assert full.any(), "no pillar with num_points == T"
    assert (full[:, None] & (pad > live_max + margin)).any(), "letting the pad value into a full pillar would go unseen"


# ------------------------------------------------------------------------------------------------------------------------------
# scatter_mean  (torch_scatter.scatter_mean as used in dynamic_mean_vfe.py:64, dynamic_pillar_vfe.py:105)
# ------------------------------------------------------------------------------------------------------------------------------
def scatter_mean(pts, col0, nc, inv, cnt, m_cap):
    """Segment sum of pts[:, col0:col0+nc] over unq_inv (rows with -1 dropped) / clamp(count, 1), fp64 -> (mean [m_cap, nc], bound)."""
    x = np.asarray(pts, F64)[:, col0:col0 + nc]
    keep = np.asarray(inv) >= 0
    s, a = np.zeros((m_cap, nc)), np.zeros((m_cap, nc))
    np.add.at(s, np.asarray(inv)[keep], x[keep])
    np.add.at(a, np.asarray(inv)[keep], np.abs(x[keep]))
    n = np.maximum(np.asarray(cnt, F64), 1.0)[:, None]
    return s / n, (n + 1) * U * a / n


def scatter_mean_f32(pts, col0, nc, inv, cnt, m_cap):
    """fp32 additions in input order (the atomics' order is free; the bound is order-free too), one divide."""
    x = f32(pts)[:, col0:col0 + nc]
    s = np.zeros((m_cap, nc), F32)
    for i in np.flatnonzero(np.asarray(inv) >= 0):
        s[inv[i]] = (s[inv[i]] + x[i]).astype(F32)
    return (s / np.maximum(cnt, 1).astype(F32)[:, None]).astype(F32)


@functools.lru_cache(maxsize=None)
def scatter_case(n, c, col0, nc, seed):
    """n points over about n / 6 voxels; one voxel holds 200 of them when there are that many; every seventh point is dropped (-1); the
    last two voxels of m_cap receive nothing (count 0 -> 0)."""
    rng = np.random.default_rng(seed)
    nv = max(1, n // 6)
    m_cap = nv + 2
    inv = rng.integers(0, nv, n).astype(np.int32)
    if n > 1:
        inv[::7] = -1
    if n >= 250:
        inv[rng.permutation(np.flatnonzero(inv >= 0))[:200]] = nv // 2
    pts = (rng.standard_normal((n, c)) * 30.0).astype(F32)
    cnt = np.bincount(inv[inv >= 0], minlength=m_cap).astype(np.int32)
    ref, bound = scatter_mean(pts, col0, nc, inv, cnt, m_cap)
    if n >= 250:
        assert cnt.max() >= 200
    if n > 1:
        assert (inv == -1).any()
    assert (cnt[-2:] == 0).all() and (ref[-2:] == 0).all()
    return dict(pts=pts, inv=inv, cnt=cnt, m_cap=m_cap, n=n, c=c, col0=col0, nc=nc, ref=ref, bound=bound)


# ------------------------------------------------------------------------------------------------------------------------------
# dynamic PFN  (dynamic_pillar_vfe.py:105-127, 210-227; dynamic_voxel_vfe.py:73-92; PFNLayerV2 dynamic_pillar_vfe.py:35-46)
# ------------------------------------------------------------------------------------------------------------------------------
def dyn_cin(c, kind, flags):
    return (c - 1 if flags & 1 else c - 4) + (3 if kind == 2 else 6) + (1 if flags & 2 else 0)


def _dyn_parts(pts, inv, pcoord, pmean, kind, flags, vs, off, dt):
    p = np.asarray(pts, dt)
    xyz = p[:, 1:4]
    cell = np.asarray(pcoord).astype(dt)
    vs, off = np.asarray(vs, dt), np.asarray(off, dt)
    ctr = ((cell * vs).astype(dt) + off).astype(dt)
    if kind != 1:
        ctr[:, 2] = off[2]                                      # pillar / simple2d: z - z_offset (dynamic_pillar_vfe.py:113, 217)
    ce = (xyz - ctr).astype(dt)
    base = p[:, 1:] if flags & 1 else p[:, 4:]
    cl = None
    if kind != 2:
        cl = (xyz - np.asarray(pmean, dt)[np.maximum(np.asarray(inv), 0)]).astype(dt)
    return p, xyz, cell, ce, base, cl


def dynamic_features(pts, inv, pcoord, pmean, kind, flags, vs=VS, off=OFF):
    """kind 0 / 1: [points[:, 1:] | points[:, 4:], f_cluster, f_center] (dynamic_pillar_vfe.py:105-123, dynamic_voxel_vfe.py:73-88);
    kind 2: [f_center, points[:, 1:] | points[:, 4:]] (dynamic_pillar_vfe.py:210-219); optional norm last.  points_mean is an INPUT
    (fp32), so f_cluster is one subtraction.  Rows with unq_inv == -1 are zero.  fp64 -> (f [n, cin], df)."""
    p, xyz, cell, ce, base, cl = _dyn_parts(pts, inv, pcoord, pmean, kind, flags, vs, off, F64)
    vs64, off64 = np.asarray(vs, F64), np.asarray(off, F64)
    d_ce = 2 * U * (np.abs(cell * vs64) + np.abs(off64)) + U * np.abs(ce)
    if kind == 2:
        parts, dparts = [ce, base], [d_ce, np.zeros_like(base)]
    else:
        parts, dparts = [base, cl, ce], [np.zeros_like(base), U * np.abs(cl), d_ce]
    if flags & 2:
        dist = np.sqrt((xyz * xyz).sum(axis=1, keepdims=True))
        parts.append(dist)
        dparts.append(3 * U * dist)
    keep = (np.asarray(inv) >= 0)[:, None]
    return np.concatenate(parts, axis=1) * keep, np.concatenate(dparts, axis=1) * keep


def dynamic_features_f32(pts, inv, pcoord, pmean, kind, flags, vs=VS, off=OFF):
    p, xyz, cell, ce, base, cl = _dyn_parts(pts, inv, pcoord, pmean, kind, flags, vs, off, F32)
    parts = [ce, base] if kind == 2 else [base, cl, ce]
    if flags & 2:
        sq = (xyz * xyz).astype(F32)
        parts.append(np.sqrt(((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)).astype(F32)[:, None])
    return np.where((np.asarray(inv) >= 0)[:, None], np.concatenate(parts, axis=1).astype(F32), F32(0))


def _seg_max(y, inv, m_cap):
    """scatter_max into zeros: the outputs are post-ReLU, so zero-initialised rows equal the maximum and empty rows stay zero."""
    out = np.zeros((m_cap, y.shape[1]), y.dtype)
    keep = np.asarray(inv) >= 0
    np.maximum.at(out, np.asarray(inv)[keep], y[keep])
    return out


def dynamic_pfn(pts, inv, pcoord, pmean, kind, layers, flags, m_cap, vs=VS, off=OFF, affine=None):
    """One or two PFNLayerV2 (dynamic_pillar_vfe.py:35-46: linear, BatchNorm, ReLU, scatter_max; non-final layers hand
    [x, x_max[unq_inv]] on), fp64 -> (features [m_cap, cout_last], bound).  Voxels without a point are zero."""
    f, df = dynamic_features(pts, inv, pcoord, pmean, kind, flags, vs, off)
    iv = np.maximum(np.asarray(inv), 0)
    for l, (w, sc, sh) in enumerate(layers):
        kw = {} if affine is None else dict(affine_u=affine[l][0], affine_extra=affine[l][1])
        y, dy = pfn_layer(f, df, w, sc, sh, **kw)
        mx, dmx = _seg_max(y, inv, m_cap), _seg_max(dy, inv, m_cap)
        if l == len(layers) - 1:
            return mx, dmx
        f, df = np.concatenate([y, mx[iv]], axis=1), np.concatenate([dy, dmx[iv]], axis=1)


def dynamic_pfn_f32(pts, inv, pcoord, pmean, kind, layers, flags, m_cap, vs=VS, off=OFF):
    f = dynamic_features_f32(pts, inv, pcoord, pmean, kind, flags, vs, off)
    iv = np.maximum(np.asarray(inv), 0)
    for l, (w, sc, sh) in enumerate(layers):
        y = pfn_layer_f32(f, w, sc, sh)
        mx = _seg_max(y, inv, m_cap)
        if l == len(layers) - 1:
            return mx
        f = np.concatenate([y, mx[iv]], axis=1)


@functools.lru_cache(maxsize=None)
def dynamic_case(n, c, kind, flags, couts, seed, norm=True):
    """n points [batch, x, y, z, extra...] over about n / 4 voxels, labelled in any order (the kernel does not need sorted ranks).
    Strip 1 (points 64..127) is dropped whole and strip 2 (128..191) keeps its last point only, where n reaches that far; the last
    three voxels of m_cap receive no point.  points_mean is the fp64 mean of the live points rounded to fp32."""
    rng = np.random.default_rng(seed)
    nv = max(1, n // 4)
    m_cap = nv + 3
    cells = np.stack([rng.integers(0, GRID[0], nv), rng.integers(0, GRID[1], nv), rng.integers(0, GRID[2], nv)], axis=1)
    cells[0, :2] = 0
    cells[-1, :2] = (GRID[0] - 1, GRID[1] - 1)
    inv = rng.integers(0, nv, n).astype(np.int32)
    pcoord = cells[inv].astype(np.int32)
    pts = np.concatenate([rng.integers(0, 2, (n, 1)).astype(F32), cell_points(rng, pcoord, c - 1)], axis=1)
    if n > 4:
        inv[3::11] = -1
    if n >= 128:
        inv[64:128] = -1
    if n >= 192:
        inv[128:191] = -1
        inv[191] = nv - 1
        pcoord[191] = cells[nv - 1]
        pts[191, 1:] = cell_points(rng, cells[nv - 1], c - 1)
    live = inv >= 0
    s = np.zeros((m_cap, 3))
    np.add.at(s, inv[live], pts[live, 1:4].astype(F64))
    cnt = np.bincount(inv[live], minlength=m_cap)
    pmean = (s / np.maximum(cnt, 1)[:, None]).astype(F32)
    layers = pfn_params(dyn_cin(c, kind, flags), couts, seed + 1, norm)
    ref, bound = dynamic_pfn(pts, inv, pcoord, pmean, kind, layers, flags, m_cap)
    if n >= 128:
        assert (inv[64:128] == -1).all(), "strip 1 is not wholly dropped"
    if n >= 192:
        assert (inv[128:191] == -1).all() and inv[191] >= 0, "strip 2: the last point must be the only live one"
    assert (cnt[-3:] == 0).all() and (ref[-3:] == 0).all() and live.any()
    assert float(ref.max()) > 0
    return dict(pts=pts, inv=inv, pcoord=pcoord, pmean=pmean, kind=kind, flags=flags, layers=layers, m_cap=m_cap, n=n, c=c,
                couts=tuple(couts), ref=ref, bound=bound, empty=cnt == 0)


# ------------------------------------------------------------------------------------------------------------------------------
# copies: PointPillarScatter, its index-map form, SparseConvTensor.dense()
# ------------------------------------------------------------------------------------------------------------------------------
def _in_range(coords, batch, ny, nx):
    co = np.asarray(coords)
    return (co[:, 0] >= 0) & (co[:, 0] < batch) & (co[:, 2] >= 0) & (co[:, 2] < ny) & (co[:, 3] >= 0) & (co[:, 3] < nx)


def pillar_scatter(feat, coords, m, batch, ny, nx):
    """pointpillar_scatter.py:14-37: canvas[b, :, y, x] = feat[row] for the first m rows (b, z, y, x), nz == 1; rows outside the grid or
    the batch are skipped (the reference never produces one).  Same dtype as feat: a copy."""
    canvas = np.zeros((batch, feat.shape[1], ny, nx), feat.dtype)
    ok = _in_range(coords[:m], batch, ny, nx)
    for r in np.flatnonzero(ok):
        b, _, y, x = coords[r]
        canvas[b, :, y, x] = feat[r]
    return canvas


def pillar_index_map(coords, m, batch, ny, nx):
    """pointpillar_scatter.py:14-37 as an index map: idx[b, y, x] = pillar row or -1."""
    idx = np.full((batch, ny, nx), -1, np.int32)
    ok = _in_range(coords[:m], batch, ny, nx)
    for r in np.flatnonzero(ok):
        idx[coords[r, 0], coords[r, 2], coords[r, 3]] = r
    return idx


def sparse_to_dense(feats, indices, m, batch, d, h, w):
    """map_to_bev/height_compression.py:10-26: dense() [N, C, D, H, W] viewed as [N, C * D, H, W]: out[b, ch * d + z, y, x] = feats[r, ch].
    indices [*, 4] = (b, z, y, x) or [*, 3] = (b, y, x) with d == 1; rows outside the grid are skipped."""
    c = feats.shape[1]
    out = np.zeros((batch, c, d, h, w), feats.dtype)
    for r in range(m):
        row = indices[r]
        b, z, y, x = (row[0], row[1], row[2], row[3]) if len(row) == 4 else (row[0], 0, row[1], row[2])
        if 0 <= b < batch and 0 <= z < d and 0 <= y < h and 0 <= x < w:
            out[b, :, z, y, x] = feats[r]
    return out.reshape(batch, c * d, h, w)


@functools.lru_cache(maxsize=None)
def grid_rows(batch, d, ny, nx, seed, want=40):
    """Distinct cells (b, z, y, x) of the grid in a shuffled order.  The first `live` rows are the input: in-range rows with one row
    per coordinate just outside its range (batch included) mixed in.  The rows behind `live` point at FREE cells of the grid where
    the grid has any, so running them would show.  Returns (rows [cap, 4] int32, live)."""
    rng = np.random.default_rng(seed)
    total = batch * d * ny * nx
    k = min(total, want)
    cells = rng.permutation(total)[:k]
    rows = np.stack([cells // (d * ny * nx), cells // (ny * nx) % d, cells // nx % ny, cells % nx], axis=1)
    n_dead = max(1, k // 3) if k > 1 else 0
    good, dead = rows[:k - n_dead], rows[k - n_dead:]
    bad = np.array([[-1, 0, 0, 0], [batch, 0, 0, 0], [0, -1, 0, 0], [0, d, 0, 0], [0, 0, -1, 0], [0, 0, ny, 0], [0, 0, 0, -1], [0, 0, 0, nx]])
    if d == 1:
        bad = bad[[0, 1, 4, 5, 6, 7]]                           # the pillar entry points do not read z
    head = np.concatenate([good, bad])[rng.permutation(len(good) + len(bad))]
    out = np.concatenate([head, dead]).astype(np.int32)
    live = len(head)
    inside = (out[:live, 0] >= 0) & (out[:live, 0] < batch) & (out[:live, 1] >= 0) & (out[:live, 1] < d) & (out[:live, 2] >= 0) & \
             (out[:live, 2] < ny) & (out[:live, 3] >= 0) & (out[:live, 3] < nx)
    assert inside.sum() == len(good) >= 1 and (~inside).sum() == len(bad)
    assert total == 1 or len(dead) >= 1, "no row behind the live count"
    return out, live


# ------------------------------------------------------------------------------------------------------------------------------
# depthwise 3 x 3 + exact GELU -> token-major bf16  (fusion/vat_lidar.py:82-85, 212-221)
# ------------------------------------------------------------------------------------------------------------------------------
_erf = np.vectorize(math.erf, otypes=[F64])


def dwconv3x3_gelu(bev, w9, bias):
    """Conv2d(C, C, 3, padding=1, groups=C) + GELU(erf) on [B, C, H, W], flattened to tokens [B, H * W, C] (vat_lidar.py:82-85, 212-221),
    fp64 -> (tokens, a) with a = 11 u (|bias| + sum |tap * w|): the bound of the pre-activation."""
    x = np.asarray(bev, F64)
    b, c, h, w = x.shape
    w9 = np.asarray(w9, F64).reshape(c, 3, 3)
    bs = np.zeros(c) if bias is None else np.asarray(bias, F64)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    acc = np.broadcast_to(bs[None, :, None, None], x.shape).copy()
    mag = np.abs(acc)
    for rr in range(3):
        for k in range(3):
            t = xp[:, :, rr:rr + h, k:k + w] * w9[None, :, rr, k, None, None]
            acc += t
            mag += np.abs(t)
    y = 0.5 * acc * (1.0 + _erf(acc / math.sqrt(2.0)))
    tok = lambda a: a.transpose(0, 2, 3, 1).reshape(b, h * w, c)
    return tok(y), tok(11 * U * mag)


def dwconv_bound(y, a, lo):
    return 1.13 * a + 2 * U * np.abs(y) + (2.0 ** -16 if lo else 2.0 ** -8) * np.abs(y)


def bf16_round(a):
    """fp32 -> bf16 round-to-nearest-even, returned as fp32."""
    u = f32(a).view(np.uint32)
    u = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return u.view(F32)


def bf16_bits_to_f32(bits):
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


def dwconv3x3_gelu_f32(bev, w9, bias, lo):
    """k_dwconv3x3_gelu's sequence: acc = bias; acc = fmaf(tap, w, acc) over rows then columns; 0.5 x (1 + erf(x * 0.70710678f)) in fp32
    (erf itself from the fp64 library, rounded); hi = bf16(y), lo = bf16(y - hi).  Returns hi (+ lo) as fp32 tokens."""
    x = f32(bev)
    b, c, h, w = x.shape
    w9 = f32(w9).reshape(c, 3, 3)
    bs = np.zeros(c, F32) if bias is None else f32(bias)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    acc = np.broadcast_to(bs[None, :, None, None], x.shape).astype(F32)
    for rr in range(3):
        for k in range(3):
            acc = fma32(xp[:, :, rr:rr + h, k:k + w], w9[None, :, rr, k, None, None], acc)
    e = _erf((acc * F32(0.70710678118654752440)).astype(F32).astype(F64)).astype(F32)
    y = (((F32(0.5) * acc).astype(F32)) * (F32(1) + e).astype(F32)).astype(F32)
    hi = bf16_round(y)
    out = hi if not lo else (hi.astype(F64) + bf16_round((y - hi).astype(F32)).astype(F64))
    return np.asarray(out).transpose(0, 2, 3, 1).reshape(b, h * w, c)


@functools.lru_cache(maxsize=None)
def dwconv_case(c, h, w, seed, batch=2):
    rng = np.random.default_rng(seed)
    bev = rng.standard_normal((batch, c, h, w)).astype(F32)
    w9 = (0.3 * rng.standard_normal((c, 9))).astype(F32)
    bias = (0.2 * rng.standard_normal(c)).astype(F32)
    out = {}
    for key, bs in (("bias", bias), ("nobias", None)):
        y, a = dwconv3x3_gelu(bev, w9, bs)
        out[key] = (y, a)
    return dict(bev=bev, w9=w9, bias=bias, ref=out, c=c, h=h, w=w, batch=batch)


DW_PX, DW_RY = 64, 4                                          # pixels x rows of one workgroup of the two dwconv kernels


def block_census(idx, by, bx):
    """Live cells of workgroup (by, bx)'s 6 x 66 neighbourhood in one scene's index map: (inside the block, in halo column x0 - 1,
    in halo row y0 + 4, elsewhere in the halo)."""
    h, w = idx.shape
    y0, x0 = by * DW_RY, bx * DW_PX
    n_in = n_col = n_row = n_other = 0
    for y in range(max(y0 - 1, 0), min(y0 + DW_RY + 1, h)):
        for x in range(max(x0 - 1, 0), min(x0 + DW_PX + 1, w)):
            if idx[y, x] < 0:
                continue
            if y0 <= y < y0 + DW_RY and x0 <= x < x0 + DW_PX:
                n_in += 1
            elif x == x0 - 1 and y0 <= y < y0 + DW_RY:
                n_col += 1
            elif y == y0 + DW_RY and x0 <= x < x0 + DW_PX:
                n_row += 1
            else:
                n_other += 1
    return n_in, n_col, n_row, n_other


@functools.lru_cache(maxsize=None)
def bridge_case(c, h, w, seed, extra=11):
    """Pillars for lvq_pillar_dwconv3x3_gelu on a [5, c, h, w] batch: scene 0 holds the four image corners and a few random cells,
    scene 1 is empty, scene 2 holds ONE pillar in column 63 (the halo column x0 - 1 of the workgroup at x0 = 64), scene 3 ONE pillar in
    row 4 (the halo row y0 + 4 of the workgroups at y0 = 0), scene 4 random cells.  Rows behind the live count sit on free cells of
    scene 1.  Where the image is large enough the build asserts: a workgroup whose only live cell is in its halo column, one whose
    only live cell is in its halo row, and beside each a workgroup whose whole neighbourhood is empty."""
    rng = np.random.default_rng(seed)
    batch = 5
    rows = {(0, 0, 0), (0, 0, w - 1), (0, h - 1, 0), (0, h - 1, w - 1)}
    for b in (0, 4):
        for _ in range(6):
            rows.add((b, int(rng.integers(0, h)), int(rng.integers(0, w))))
    if w > DW_PX:
        rows.add((2, min(1, h - 1), DW_PX - 1))
    if h > DW_RY:
        rows.add((3, DW_RY, min(w - 1, 100)))
    rows = np.array(sorted(rows))[:, [0, 0, 1, 2]]
    rows[:, 1] = 0
    rows = rows[rng.permutation(len(rows))]
    live = len(rows)
    dead = np.array([[1, 0, int(rng.integers(0, h)), int(rng.integers(0, w))] for _ in range(extra)])
    coords = np.concatenate([rows, dead]).astype(np.int32)
    feat = rng.standard_normal((len(coords), c)).astype(F32)
    w9 = (0.3 * rng.standard_normal((c, 9))).astype(F32)
    bias = (0.2 * rng.standard_normal(c)).astype(F32)
    idx = pillar_index_map(coords, live, batch, h, w)
    assert (idx[1] < 0).all() and all(idx[0, y, x] >= 0 for y in (0, h - 1) for x in (0, w - 1))
    nby, nbx = -(-h // DW_RY), -(-w // DW_PX)
    if w > DW_PX:
        assert block_census(idx[2], 0, 1) == (0, 1, 0, 0), "scene 2: the workgroup at x0 = 64 must see its halo column only"
        if nbx > 2:
            assert block_census(idx[2], 0, 2) == (0, 0, 0, 0), "scene 2: no empty workgroup beside it"
    if h > DW_RY:
        assert block_census(idx[3], 0, min(w - 1, 100) // DW_PX) == (0, 0, 1, 0), "scene 3: a workgroup at y0 = 0 must see its halo row only"
        if min(w - 1, 100) > DW_PX:
            assert block_census(idx[3], 0, 0) == (0, 0, 0, 0), "scene 3: no empty workgroup beside it"
    return dict(feat=feat, coords=coords, live=live, cap=len(coords), w9=w9, bias=bias, batch=batch, c=c, h=h, w=w, idx=idx,
                nby=nby, nbx=nbx)


# ------------------------------------------------------------------------------------------------------------------------------
# the case lists both test files walk
# ------------------------------------------------------------------------------------------------------------------------------
FLAGS = (0, 1, 2, 3)                                          # bit0 USE_ABSLOTE_XYZ, bit1 WITH_DISTANCE: cin 7 / 10 / 8 / 11 at c = 4
FAST_T = (1, 7, 8, 9, 20, 31, 32)
FAST_COUT = (8, 48, 64)
FAST_M = (1, 7, 8, 9, 31, 32, 33, 257)


def pillar_single_layer_cases():
    """(m, t, c, couts, flags, seed, norm): every case the fast kernel takes (c = 4, one layer, T <= 32, cout <= 64).  The generic
    kernel runs the same list under tune(pillar_vfe_generic=1)."""
    out = []
    for ti, t in enumerate(FAST_T):
        for ci, cout in enumerate(FAST_COUT):
            for flags in FLAGS:
                out.append((33, t, 4, (cout,), flags, 7000 + 100 * ti + 10 * ci + flags, True))
    for mi, m in enumerate(FAST_M):
        out.append((m, 20, 4, (64,), 1 + 2 * (mi & 1), 7900 + mi, True))
    for flags in FLAGS:
        out.append((33, 20, 4, (64,), flags, 7950 + flags, False))     # USE_NORM=False: scale 1, shift of both signs
    return out


def pillar_generic_cases():
    """Shapes only k_pillar_vfe<32> / <64> take: c = 5, T in {33, 64}, cout > 64, stacks of 2..4 layers, the > 64 KB LDS request, the
    2- and 1-wave workgroups, and the largest accepted shapes (T * cmax == 20480 floats per plane pair is 160 KB)."""
    out = [(33, 20, 5, (64,), 1, 8000, True), (33, 20, 5, (64,), 2, 8001, True), (33, 20, 5, (48,), 3, 8002, False),
           (9, 33, 4, (64,), 1, 8003, True), (9, 64, 4, (64,), 3, 8004, True), (9, 64, 4, (48,), 0, 8005, False),
           (9, 20, 4, (65,), 1, 8006, True), (9, 20, 4, (128,), 3, 8007, True), (9, 32, 4, (256,), 1, 8008, True),
           (9, 20, 4, (32, 64), 1, 8009, True), (9, 64, 4, (64, 64), 1, 8010, True), (9, 20, 4, (16, 16, 32), 3, 8011, True),
           (9, 20, 5, (16, 16, 16, 32), 1, 8012, True), (9, 32, 4, (64, 64), 0, 8013, False),
           (6, 32, 4, (256, 256), 1, 8014, True),            # <32>: cmax 512, one wave per workgroup, 128 KB
           (6, 40, 4, (256, 256), 1, 8015, True),            # <64>: T * cmax = 20480 exactly, 160 KB
           (6, 64, 4, (160, 256), 3, 8016, True)]            # <64>: T = 64 at its widest, cmax 320, 160 KB
    return out


def pillar_lds_bytes(t, c, couts, flags):
    """(waves per workgroup, dynamic LDS bytes) of the generic kernel for a shape, as include/lvq.h states the rule; None if refused."""
    cin, cmax = pfn_cin(c, flags), c
    for l, co in enumerate(couts):
        cmax = max(cmax, cin, co if l == len(couts) - 1 else 2 * co)
        cin = 2 * co
    per_wave = 2 * t * cmax * 4
    for wpb in (4, 2, 1):
        if per_wave * wpb <= 160 * 1024:
            return wpb, per_wave * wpb
    return None


DYN_N = (1, 63, 64, 65, 300)


def dynamic_cases():
    """(n, c, kind, flags, couts, seed, norm)."""
    out = []
    for kind in (0, 1, 2):
        for flags in FLAGS:
            out.append((300, 4 + (kind + flags) % 3, kind, flags, (64,), 9000 + 10 * kind + flags, True))
    for i, n in enumerate(DYN_N):
        out.append((n, 4, i % 3, 1, (64,), 9100 + i, True))
        out.append((n, 5, (i + 1) % 3, 3, (64, 64), 9110 + i, True))
    out += [(300, 4, 0, 1, (32,), 9200, True), (300, 4, 1, 1, (96,), 9201, True), (65, 4, 2, 1, (96,), 9202, False),
            (300, 4, 0, 1, (192, 192), 9203, True), (300, 4, 1, 3, (256, 256), 9204, True), (65, 6, 0, 0, (64, 64), 9205, False),
            (65, 11, 0, 1, (64,), 9206, True)]                # c = 11 with absolute xyz: 16 augmented features, the most the kernel takes
    return out


SCATTER_N = (1, 255, 256, 257)
SCATTER_COLS = ((5, 1, 3), (5, 1, 4), (4, 0, 4), (6, 5, 1))


def scatter_cases():
    return [(n, c, col0, nc, 9500 + 10 * i + j) for i, n in enumerate(SCATTER_N) for j, (c, col0, nc) in enumerate(SCATTER_COLS)]


DWCONV_SHAPES = ((8, 1, 1), (40, 3, 63), (64, 4, 64), (72, 5, 65), (136, 9, 130))
COPY_GRIDS = ((1, 1), (4, 64), (5, 65), (9, 300))
COPY_CH = (1, 31, 32, 33, 70)
