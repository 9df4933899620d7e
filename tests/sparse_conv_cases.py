"""Host side (numpy / torch CPU, fp64) of the sparse-convolution tests: two independent restatements of include/lvq.h's "Sparse
convolution backbone" semantics, the backbone chain on either of them, and the coordinate sets of the GPU tests.

  sparse_conv   fp64 numpy over a coordinate dictionary, the header's formulas verbatim: the output set, the neighbour table
                nbr [n_out, K] (-1 = absent) and out[q] = sum over ascending offsets of W[:, o, :] . in[row]
  dense_conv    fp64 torch conv3d / conv2d (cross-correlation, weight.permute(0, 4, 1, 2, 3)) on the densified tensor; the active set
                comes from a ones-kernel convolution of the occupancy mask
  backbone      VoxelResBackBone8xVoxelNeXt (spconv_backbone_voxelnext.py:166-225) as a chain of either restatement, BatchNorm folded
                in fp64, with every stage's tensor kept for per-stage error reports

tests/test_sparse_conv_restatements.py holds the two against each other on the CPU; the GPU files compare the kernels with `sparse_conv`.
"""
import functools
import itertools

import numpy as np
import torch

from lidar_vision_vqa_amd import synth

CIN = (4, 5, 16, 32, 64, 128)
COUT = (16, 32, 64, 128)


def _t(v, nd):
    return tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v),) * nd


def out_shape(shape, kernel, stride, padding, subm):
    nd = len(shape)
    k, s, p = _t(kernel, nd), _t(stride, nd), _t(padding, nd)
    return list(shape) if subm else [(d + 2 * pp - kk) // ss + 1 for d, kk, ss, pp in zip(shape, k, s, p)]


# --------------------------------------------------------------------------------------------------------------------------------
# sparse restatement
# --------------------------------------------------------------------------------------------------------------------------------
def rules(idx, shape, batch, kernel, stride, padding, subm):
    """(out_idx [n_out, 1 + nd], nbr [n_out, K]).  subm: out_idx is idx (same order); else ascending (b, z, y, x)."""
    idx = np.asarray(idx, np.int64).reshape(-1, len(shape) + 1)
    nd = len(shape)
    k, s, p = _t(kernel, nd), _t(stride, nd), _t(padding, nd)
    if subm:
        s, p = (1,) * nd, tuple(kk // 2 for kk in k)
    oshape = out_shape(shape, k, s, p, subm)
    offs = list(itertools.product(*[range(kk) for kk in k]))                    # ascending o = (oz * ky + oy) * kx + ox
    row_of = {}
    for i, r in enumerate(idx):
        if 0 <= r[0] < batch and all(0 <= r[1 + a] < shape[a] for a in range(nd)):
            row_of[tuple(r)] = i
    if subm:
        outs = [tuple(r) for r in idx]
    else:
        sites = set()
        for (b, *c) in row_of:
            for o in offs:
                num = [c[a] + p[a] - o[a] for a in range(nd)]
                if all(n % s[a] == 0 and 0 <= n // s[a] < oshape[a] for a, n in enumerate(num)):
                    sites.add((b, *[n // s[a] for a, n in enumerate(num)]))
        outs = sorted(sites)
    nbr = np.full((len(outs), len(offs)), -1, np.int64)
    for r, (b, *q) in enumerate(outs):
        if subm and (b, *q) not in row_of:
            continue                                                            # a row outside the grid takes no part
        for j, o in enumerate(offs):
            c = tuple(q[a] * s[a] - p[a] + o[a] for a in range(nd))
            if all(0 <= c[a] < shape[a] for a in range(nd)):
                nbr[r, j] = row_of.get((b, *c), -1)
    return np.asarray(outs, np.int64).reshape(-1, nd + 1), nbr


def conv_from_table(feat, nbr, weight):
    """acc [n_out, C_out] fp64: offsets in ascending order.  weight [C_out, *kernel, C_in]."""
    w = np.asarray(weight, np.float64)
    w = w.reshape(w.shape[0], -1, w.shape[-1])
    f = np.asarray(feat, np.float64)
    acc = np.zeros((nbr.shape[0], w.shape[0]))
    for o in range(nbr.shape[1]):
        have = nbr[:, o] >= 0
        if have.any():
            acc[have] += f[nbr[have, o]] @ w[:, o, :].T
    return acc


def epilogue(acc, bias=None, scale=None, shift=None, residual=None, relu=False):
    y = np.asarray(acc, np.float64)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if scale is not None:
        y = y * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return np.maximum(y, 0.0) if relu else y


_RULES_MEMO = {}


def rules_memo(idx, shape, batch, kernel, stride, padding, subm):
    """rules() remembered per (index set, geometry): the layers of a backbone stage share their table, as indice_key says."""
    idx = np.ascontiguousarray(idx, np.int64)
    key = (idx.tobytes(), tuple(shape), batch, _t(kernel, len(shape)), _t(stride, len(shape)), _t(padding, len(shape)), bool(subm))
    if key not in _RULES_MEMO:
        if len(_RULES_MEMO) > 64:
            _RULES_MEMO.clear()
        _RULES_MEMO[key] = rules(idx, shape, batch, kernel, stride, padding, subm)
    return _RULES_MEMO[key]


def sparse_conv(feat, idx, shape, batch, weight, stride=1, padding=0, subm=False):
    kernel = tuple(np.asarray(weight).shape[1:-1])
    oi, nbr = rules_memo(idx, shape, batch, kernel, stride, padding, subm)
    return oi, conv_from_table(feat, nbr, weight)


# --------------------------------------------------------------------------------------------------------------------------------
# dense restatement
# --------------------------------------------------------------------------------------------------------------------------------
def dense_conv(feat, idx, shape, batch, weight, stride=1, padding=0, subm=False):
    idx = np.asarray(idx, np.int64)
    nd = len(shape)
    w = torch.as_tensor(np.asarray(weight, np.float64))
    k = tuple(w.shape[1:-1])
    s, p = _t(stride, nd), _t(padding, nd)
    if subm:
        s, p = (1,) * nd, tuple(kk // 2 for kk in k)
    c_in = w.shape[-1]
    x = torch.zeros((batch, c_in, *shape), dtype=torch.float64)
    occ = torch.zeros((batch, 1, *shape), dtype=torch.float64)
    cols = tuple(torch.as_tensor(idx[:, a]) for a in range(nd + 1))
    f = torch.as_tensor(np.asarray(feat, np.float64))
    if nd == 3:
        x[cols[0], :, cols[1], cols[2], cols[3]] = f
        occ[cols[0], 0, cols[1], cols[2], cols[3]] = 1.0
        conv, wd = torch.nn.functional.conv3d, w.permute(0, 4, 1, 2, 3)
    else:
        x[cols[0], :, cols[1], cols[2]] = f
        occ[cols[0], 0, cols[1], cols[2]] = 1.0
        conv, wd = torch.nn.functional.conv2d, w.permute(0, 3, 1, 2)
    y = conv(x, wd.contiguous(), stride=s, padding=p)
    if subm:
        oi = idx
    else:
        act = conv(occ, torch.ones((1, 1, *k), dtype=torch.float64), stride=s, padding=p)[:, 0] > 0.5
        oi = torch.nonzero(act).numpy()                                         # ascending (b, z, y, x)
    sel = tuple(torch.as_tensor(oi[:, a]) for a in range(nd + 1))
    vals = y[sel[0], :, sel[1], sel[2], sel[3]] if nd == 3 else y[sel[0], :, sel[1], sel[2]]
    return oi.reshape(-1, nd + 1), vals.numpy().reshape(len(oi), -1)


# --------------------------------------------------------------------------------------------------------------------------------
# the backbone chain on either restatement
# --------------------------------------------------------------------------------------------------------------------------------
def bn_fold(sd, prefix, eps):
    g = lambda k: np.asarray(sd[prefix + k], np.float64)
    scale = g("weight") / np.sqrt(g("running_var") + eps)
    return scale, g("bias") - g("running_mean") * scale


def bev_merge(feat, idx, shape):
    """bev_out: unique (b, y, x) ascending, rows summed."""
    byx = idx[:, [0, 2, 3]]
    uniq, inv = np.unique(byx, axis=0, return_inverse=True)
    out = np.zeros((len(uniq), feat.shape[1]))
    np.add.at(out, inv.reshape(-1), feat)
    return out, uniq, list(shape[1:])


def backbone(sd, feats, coords, grid_size, batch, conv=sparse_conv):
    """{stage: (features fp64, indices, spatial_shape)} for conv_input, x_conv1..6, merged, bev, conv_out, out."""
    sd = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in sd.items()}
    shape = [grid_size[2] + 1, grid_size[1], grid_size[0]]
    f, idx = np.asarray(feats, np.float64), np.asarray(coords, np.int64)

    def post_act(f, idx, shape, prefix, stride, padding, subm, eps=1e-3, bias=None):
        oi, acc = conv(f, idx, shape, batch, sd[prefix + "0.weight"], stride, padding, subm)
        sc, sh = bn_fold(sd, prefix + "1.", eps)
        return epilogue(acc, bias, sc, sh, None, True), oi, out_shape(shape, 3, stride, padding, subm)

    def block(f, idx, shape, prefix):
        _, a = conv(f, idx, shape, batch, sd[prefix + "conv1.weight"], 1, 1, True)
        h = epilogue(a, sd[prefix + "conv1.bias"], *bn_fold(sd, prefix + "bn1.", 1e-3), None, True)
        _, a = conv(h, idx, shape, batch, sd[prefix + "conv2.weight"], 1, 1, True)
        return epilogue(a, sd[prefix + "conv2.bias"], *bn_fold(sd, prefix + "bn2.", 1e-3), f, True)

    st = {}
    f, idx, shape = post_act(f, idx, shape, "conv_input.", 1, 1, True)
    st["conv_input"] = (f, idx, shape)
    for b in ("conv1.0.", "conv1.1."):
        f = block(f, idx, shape, b)
    st["x_conv1"] = (f, idx, shape)
    for n in (2, 3, 4, 5, 6):
        f, idx, shape = post_act(f, idx, shape, f"conv{n}.0.", 2, 1, False)
        for b in (f"conv{n}.1.", f"conv{n}.2."):
            f = block(f, idx, shape, b)
        st[f"x_conv{n}"] = (f, idx, shape)
    f4, i4, s4 = st["x_conv4"]
    f5, i5, _ = st["x_conv5"]
    f6, i6, _ = st["x_conv6"]
    i5, i6 = i5.copy(), i6.copy()
    i5[:, 1:] *= 2
    i6[:, 1:] *= 4
    fm, im = np.concatenate([f4, f5, f6]), np.concatenate([i4, i5, i6])
    st["merged"] = (fm, im, s4)
    f, idx, shape = bev_merge(fm, im, s4)
    st["bev"] = (f, idx, shape)
    f, idx, shape = post_act(f, idx, shape, "conv_out.", 1, 1, False)
    st["conv_out"] = (f, idx, shape)
    f, idx, shape = post_act(f, idx, shape, "shared_conv.", 1, 1, True, eps=1e-5, bias=sd["shared_conv.0.bias"])
    st["out"] = (f, idx, shape)
    return st


def densify(f, idx, shape, batch):
    out = np.zeros((batch, f.shape[1], *shape))
    if len(shape) == 3:
        out[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = f
    else:
        out[idx[:, 0], :, idx[:, 1], idx[:, 2]] = f
    return out


def expected_state_dict_shapes(input_channels, channels=(16, 32, 64, 128, 128), out_channel=128):
    """Keys and shapes of the reference's `backbone_3d.*` checkpoint entries (spconv 2.x weight layout [C_out, *kernel, C_in])."""
    sh = {}

    def bn(p, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            sh[p + k] = (c,)
        sh[p + "num_batches_tracked"] = ()

    def block(p, c):
        for n in ("1", "2"):
            sh[f"{p}conv{n}.weight"] = (c, 3, 3, 3, c)
            sh[f"{p}conv{n}.bias"] = (c,)
            bn(f"{p}bn{n}.", c)

    sh["conv_input.0.weight"] = (channels[0], 3, 3, 3, input_channels)
    bn("conv_input.1.", channels[0])
    block("conv1.0.", channels[0])
    block("conv1.1.", channels[0])
    cin = channels[0]
    for n, c in zip((2, 3, 4, 5, 6), (channels[1], channels[2], channels[3], channels[4], channels[4])):
        sh[f"conv{n}.0.0.weight"] = (c, 3, 3, 3, cin)
        bn(f"conv{n}.0.1.", c)
        block(f"conv{n}.1.", c)
        block(f"conv{n}.2.", c)
        cin = c
    sh["conv_out.0.weight"] = (out_channel, 3, 3, channels[3])
    bn("conv_out.1.", out_channel)
    sh["shared_conv.0.weight"] = (out_channel, 3, 3, out_channel)
    sh["shared_conv.0.bias"] = (out_channel,)
    bn("shared_conv.1.", out_channel)
    return sh


@functools.lru_cache(maxsize=None)
def backbone_state(input_channels, seed):
    return synth.seeded_state_dict(expected_state_dict_shapes(input_channels).items(), seed)


# --------------------------------------------------------------------------------------------------------------------------------
# coordinate sets
# --------------------------------------------------------------------------------------------------------------------------------
def _distinct(rows):
    seen, out = set(), []
    for r in rows:
        if tuple(r) not in seen:
            seen.add(tuple(r))
            out.append(tuple(int(v) for v in r))
    return out


@functools.lru_cache(maxsize=None)
def coords(name):
    """(indices int32 [N, 1 + nd] in a shuffled order, spatial_shape, batch).
      g3a / g3b   batch 2 on [9, 24, 32] / [6, 5, 7]: random cells (the CPU comparison of the two restatements; g2a / g2b their 2-D twins)
      edge3 / edge2   batch 4 with scene 2 EMPTY: every corner, one cell on every edge and face, the pair (last cell of scene 0, first
                  cell of scene 1) and (last of 1, first of 3 -- across the empty scene), a full 3 x 3 x 3 block (every offset occurs), an
                  isolated cell (only its centre), random cells
      n0 / n1     no row, one row
      bb_small / bb_mid   the backbone grids: grid_size (32, 24, 8) batch 2, (88, 72, 16) batch 3 with scene 1 empty"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("g3a", "g3b", "g2a", "g2b"):
        shape = {"g3a": [9, 24, 32], "g3b": [6, 5, 7], "g2a": [24, 32], "g2b": [5, 7]}[name]
        n = {"g3a": 500, "g3b": 90, "g2a": 200, "g2b": 20}[name]
        rows = [(rng.integers(2), *[rng.integers(d) for d in shape]) for _ in range(3 * n)]
        rows = _distinct(rows)[:n]
        return np.asarray(rows, np.int32), shape, 2
    if name in ("edge3", "edge2"):
        shape = [7, 10, 12] if name == "edge3" else [10, 12]
        nd = len(shape)
        rows = []
        for b in (0, 1, 3):
            for corner in itertools.product(*[(0, d - 1) for d in shape]):
                rows.append((b, *corner))
        for fixed in itertools.product(*[(0, None, -1)] * nd):                  # faces and edges: some axes pinned to a side, the rest inside
            if all(v is None for v in fixed):
                continue
            rows.append((0, *[(d // 2 if v is None else (0 if v == 0 else d - 1)) for v, d in zip(fixed, shape)]))
        rows += [(1, *block) for block in itertools.product(*[(3, 4, 5)] * nd)]  # a full block: its centre has every offset
        rows.append((3, *[d // 2 for d in shape]))                              # isolated: only its centre (scene 3 holds corners only besides)
        rows += [(int(rng.choice((0, 1))), *[int(rng.integers(d)) for d in shape]) for _ in range(60)]
        rows = _distinct(rows)
        rows = [rows[i] for i in rng.permutation(len(rows))]
        return np.asarray(rows, np.int32), shape, 4
    if name == "n0":
        return np.zeros((0, 4), np.int32), [7, 10, 12], 2
    if name == "n1":
        return np.asarray([(1, 6, 9, 11)], np.int32), [7, 10, 12], 2
    if name in ("bb_small", "bb_mid"):
        grid, batch, n, scenes = ((32, 24, 8), 2, 260, (0, 1)) if name == "bb_small" else ((88, 72, 16), 3, 900, (0, 2))
        shape = [grid[2] + 1, grid[1], grid[0]]
        # clustered cells (a sparse CNN on isolated voxels exercises nothing) below z = nz (the voxeliser never fills the extra plane)
        centres = [(int(rng.choice(scenes)), *[int(rng.integers(d)) for d in (grid[2], grid[1], grid[0])]) for _ in range(n // 12)]
        rows = []
        for b, z, y, x in centres:
            for _ in range(16):
                c = (z + int(rng.integers(-1, 2)), y + int(rng.integers(-2, 3)), x + int(rng.integers(-2, 3)))
                if all(0 <= v < d for v, d in zip(c, (grid[2], grid[1], grid[0]))):
                    rows.append((b, *c))
        rows += [(scenes[0], 0, 0, 0), (scenes[-1], grid[2] - 1, grid[1] - 1, grid[0] - 1)]
        rows = _distinct(rows)[:n]
        return np.asarray(rows, np.int32), shape, batch
    raise KeyError(name)


def check_edge_case(name, kernel=3):
    """The properties the rule tests rely on, asserted where the case is built: every offset occurs, some row has only its centre."""
    idx, shape, batch = coords(name)
    _, nbr = rules(idx, shape, batch, (kernel,) * len(shape), 1, 1, True)
    assert (nbr >= 0).any(axis=0).all(), "an offset never occurs"
    centre = nbr.shape[1] // 2
    only = (nbr >= 0).sum(axis=1) == 1
    assert (only & (nbr[:, centre] >= 0)).any(), "no row with only its centre"
    assert 2 not in set(idx[:, 0].tolist()) and {0, 1, 3} <= set(idx[:, 0].tolist())
    last = tuple(d - 1 for d in shape)
    have = {tuple(r) for r in idx.tolist()}
    assert (0, *last) in have and (1, *([0] * len(shape))) in have and (1, *last) in have and (3, *([0] * len(shape))) in have
    return True
