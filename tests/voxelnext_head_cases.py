"""Host side (numpy, fp64) of the VoxelNeXtHead tests: the cases, and restatements written from the module structure
(pcdet/models/dense_heads/voxelnext_head.py:13-559, centernet_utils.py:243-354), not from the kernels.

  cases        CASES, B = 2, a few hundred rows in all, 128 channels:
                 nusc   the six nuScenes tasks, ten classes, vel, stride 8, KERNEL_SIZE_HEAD 1, USE_BIAS_BEFORE_NORM True; a 16 x 16 grid with
                        170 + 130 rows (the 64-row tiles have a ragged tail and one tile spans both scenes); K = 32
                 k3     one task, three classes, no vel, stride 4, KERNEL_SIZE_HEAD absent (the class default, 3), USE_BIAS_BEFORE_NORM
                        absent; a 16 x 24 grid with rows on all four edges and in the corners; the last rows of scene 0 and the first rows of
                        scene 1 occupy the same cells (a neighbour must not cross scenes); K = 96: the NMS mask has two words
                 nc1    num_conv = 1 everywhere, one task, two classes, KERNEL_SIZE_HEAD 1, stride 4; K = 32
               Weights come from synth.seeded_array per state_dict key, as in center_head_cases.state.
  head_rows    the branch convs as a dictionary lookup over (b, y, x): SubMConv2d k x k (+ bias), BatchNorm1d folded with eps 1e-5, ReLU,
               SubMConv2d 1 x 1 + bias, fp64
  decode_ref   centernet_utils.py:243-354 with the CORRECTED class: per scene the min(K, n_cls * n_b) largest fp32 scores of the [n_cls, n_b]
               matrix of the scene's rows (stored order), descending, ties towards the lower flat index; class = the matrix row (the reference
               computes ind // K, which is the matrix row only when n_b >= K); gathers through the rows' own (y, x)
  head_final   voxelnext_head.py:418-488: per task decode, per scene NMS, concatenation in head order, labels + 1

inter_area / iou_matrix / greedy_nms / decode_margins / Cfg / the class lists are center_head_cases' (imported, not copied).  The xseeds
were chosen by tools/make_voxelnext_head_golden.py --search so that every margin condition holds
(tests/test_voxelnext_head_restatements.py asserts them on the CPU).
"""
import functools

import numpy as np

from lidar_vision_vqa_amd import synth

import center_head_cases as CC
from center_head_cases import BRANCH_WIDTH, NUSC_CLASSES, NUSC_HEADS, Cfg, decode_margins, greedy_nms, inter_area, iou_matrix, scores32  # noqa: F401

C = 128
BN_EPS = 1e-5                                    # nn.BatchNorm1d's default: voxelnext_head.py:26 passes none


def head_cfg(heads, vel, stride, k, num_conv=2, kernel_size=None, bias_before_norm=None, limit=(-6.0, -10.0, -10.0, 6.0, 10.0, 10.0),
             pre=1000, post=83, nms_thresh=CC.NMS_THRESH, score_thresh=CC.SCORE_THRESH, **extra):
    """kernel_size None leaves KERNEL_SIZE_HEAD out (the class default, 3); bias_before_norm None leaves USE_BIAS_BEFORE_NORM out (False)."""
    names = ["center", "center_z", "dim", "rot"] + (["vel"] if vel else [])
    post_cfg = Cfg(SCORE_THRESH=score_thresh, POST_CENTER_LIMIT_RANGE=list(limit), MAX_OBJ_PER_SAMPLE=k,
                   NMS_CONFIG=Cfg(NMS_TYPE="nms_gpu", NMS_THRESH=nms_thresh, NMS_PRE_MAXSIZE=pre, NMS_POST_MAXSIZE=post))
    cfg = Cfg(CLASS_NAMES_EACH_HEAD=[list(h) for h in heads], SHARED_CONV_CHANNEL=C, NUM_HM_CONV=num_conv,
              SEPARATE_HEAD_CFG=Cfg(HEAD_ORDER=names, HEAD_DICT=Cfg({n: Cfg(out_channels=BRANCH_WIDTH[n], num_conv=num_conv) for n in names})),
              TARGET_ASSIGNER_CONFIG=Cfg(FEATURE_MAP_STRIDE=stride), POST_PROCESSING=post_cfg, **extra)
    if kernel_size is not None:
        cfg["KERNEL_SIZE_HEAD"] = kernel_size
    if bias_before_norm is not None:
        cfg["USE_BIAS_BEFORE_NORM"] = bias_before_norm
    return cfg


# name -> what the constructor and a forward need.  Cells are 0.8 m (stride * voxel), boxes about 0.55 m (the dim branch's bias); the limit
# range cuts the outer 0.4 m in x.  rows: active rows per scene; seam: how many cells the end of scene 0 shares with the start of scene 1.
CASES = {
    "nusc": dict(heads=NUSC_HEADS, vel=True, stride=8, k=32, class_names=NUSC_CLASSES, grid=(16, 16), rows=(170, 130), seam=0,
                 voxel_size=[0.1, 0.1, 0.2], point_cloud_range=[-6.4, -6.4, -5.0, 6.4, 6.4, 3.0], grid_size=[128, 128, 40],
                 wseed=81, xseed=42, hm_scale=2.5, hm_bias=-2.0, cfg=dict(kernel_size=1, bias_before_norm=True)),
    "k3": dict(heads=[["Car", "Pedestrian", "Cyclist"]], vel=False, stride=4, k=96, class_names=["Car", "Pedestrian", "Cyclist"], grid=(16, 24),
               rows=(230, 220), seam=12, voxel_size=[0.2, 0.2, 0.2], point_cloud_range=[-9.6, -6.4, -5.0, 9.6, 6.4, 3.0], grid_size=[96, 64, 40],
               wseed=82, xseed=14, hm_scale=2.5, hm_bias=-2.0, cfg=dict(limit=(-9.2, -10.0, -10.0, 9.2, 10.0, 10.0))),
    "nc1": dict(heads=[["Car", "Pedestrian"]], vel=False, stride=4, k=32, class_names=["Car", "Pedestrian"], grid=(16, 16), rows=(150, 120), seam=0,
                voxel_size=[0.2, 0.2, 0.2], point_cloud_range=[-6.4, -6.4, -5.0, 6.4, 6.4, 3.0], grid_size=[64, 64, 40],
                wseed=83, xseed=2, hm_scale=2.5, hm_bias=-2.0, cfg=dict(kernel_size=1, num_conv=1)),
}


def case_cfg(name, **kw):
    c = CASES[name]
    return head_cfg(c["heads"], c["vel"], c["stride"], c["k"], **dict(c.get("cfg", {}), **kw))


def kernel_size(cfg):
    return int(cfg.get("KERNEL_SIZE_HEAD", 3))


def golden_name(name):
    return f"voxelnext_head_{name}.npz"


def branch_names(cfg):
    return list(cfg.SEPARATE_HEAD_CFG.HEAD_DICT) + ["hm"]


def scene_cells(h, w, n, rng, first=()):
    """n distinct cells of an h x w grid in a seeded order: `first`, then the four corners and one cell of every edge, then the rest."""
    must = [tuple(c) for c in first]
    for c in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1)]:
        if c not in must:
            must.append(c)
    rest = [(y, x) for y in range(h) for x in range(w) if (y, x) not in must]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    cells = (must + rest)[:n]
    head, tail = cells[:len(first)], cells[len(first):]
    return head + [tail[i] for i in rng.permutation(len(tail))]


def case_indices(name):
    """[N, 3] int32 (b, y, x): scene 0's rows, then scene 1's, each in a seeded (not sorted) order; the last `seam` rows of scene 0 and the
    first `seam` rows of scene 1 are the same cells."""
    c = CASES[name]
    h, w = c["grid"]
    rng = np.random.default_rng([c["wseed"], 7])
    s0 = scene_cells(h, w, c["rows"][0], rng)
    seam = s0[len(s0) - c["seam"]:] if c["seam"] else []
    s1 = scene_cells(h, w, c["rows"][1], rng, first=seam)
    return np.array([(0, y, x) for y, x in s0] + [(1, y, x) for y, x in s1], np.int32)


def case_input(name, xseed=None):
    """(features [N, 128] fp32, indices [N, 3] int32)"""
    c = CASES[name]
    idx = case_indices(name)
    return synth.randn((len(idx), C), c["xseed"] if xseed is None else xseed), idx


# --------------------------------------------------------------------------------------------------------------------------------
# structure and state
# --------------------------------------------------------------------------------------------------------------------------------
def state_shapes(cfg):
    """[(key, shape)] in the reference's registration order (voxelnext_head.py:18-40, 92-105).  Weights are spconv 2.x's [C_out, *kernel, C_in]."""
    bias, ks = cfg.get("USE_BIAS_BEFORE_NORM", False), kernel_size(cfg)
    out = []
    for i, heads in enumerate(cfg.CLASS_NAMES_EACH_HEAD):
        for name in branch_names(cfg):
            width = len(heads) if name == "hm" else cfg.SEPARATE_HEAD_CFG.HEAD_DICT[name]["out_channels"]
            num_conv = cfg.NUM_HM_CONV if name == "hm" else cfg.SEPARATE_HEAD_CFG.HEAD_DICT[name]["num_conv"]
            p = f"heads_list.{i}.{name}"
            for k in range(num_conv - 1):
                out += [(f"{p}.{k}.0.weight", (C, ks, ks, C))] + ([(f"{p}.{k}.0.bias", (C,))] if bias else []) + CC._bn_keys(f"{p}.{k}.1", C)
            out += [(f"{p}.{num_conv - 1}.weight", (width, 1, 1, C)), (f"{p}.{num_conv - 1}.bias", (width,))]
    return out


def state(cfg, seed, hm_scale=1.0, hm_bias=-2.19):
    """A seeded state_dict, with center_head_cases.state's rescaling: convs in front of a ReLU N(0, 2 / fan_in); hm: zero-mean filters *
    hm_scale, bias hm_bias; dim: weight * DIM_SCALE, bias DIM_BIAS."""
    out = {}
    for k, s in state_shapes(cfg):
        a = synth.seeded_array(k, tuple(s), seed)
        last = k.count(".") == 4                                              # heads_list.i.name.k.weight / .bias
        if len(s) == 4 and not last:
            a = (a * np.sqrt(2.0)).astype(np.float32)
        if last and ".hm." in k:
            a = ((a - a.mean(axis=(1, 2, 3), keepdims=True)) * hm_scale).astype(np.float32) if len(s) == 4 else np.full(s, hm_bias, np.float32)
        if last and ".dim." in k:
            a = (a * CC.DIM_SCALE).astype(np.float32) if len(s) == 4 else np.full(s, CC.DIM_BIAS, np.float32)
        out[k] = a
    return out


@functools.lru_cache(maxsize=None)
def case_state(name):
    c = CASES[name]
    return state(case_cfg(name), c["wseed"], c["hm_scale"], c["hm_bias"])


# --------------------------------------------------------------------------------------------------------------------------------
# the branch convs, fp64, as a dictionary lookup
# --------------------------------------------------------------------------------------------------------------------------------
def neighbour_table(indices, ks):
    """[N, ks * ks] row numbers (offset-major (dy, dx) ascending), -1 where the cell (b, y + dy, x + dx) holds no row."""
    site = {(int(b), int(y), int(x)): i for i, (b, y, x) in enumerate(indices)}
    r = ks // 2
    return np.array([[site.get((int(b), int(y) + dy, int(x) + dx), -1) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
                     for b, y, x in indices], np.int64).reshape(len(indices), ks * ks)


def _subm(x, nb, w, b):
    """x [N, C_in] fp64, nb [N, K], w [C_out, kh, kw, C_in] -> [N, C_out]"""
    w = np.asarray(w, np.float64).reshape(w.shape[0], -1, w.shape[-1])
    out = np.zeros((x.shape[0], w.shape[0]))
    for o in range(nb.shape[1]):
        g = np.where((nb[:, o] >= 0)[:, None], x[np.maximum(nb[:, o], 0)], 0.0)
        out += g @ w[:, o].T
    return out if b is None else out + np.asarray(b, np.float64)


def head_rows(cfg, sd, feats, indices, eps=BN_EPS):
    """features [N, 128], indices [N, 3] -> one dict {branch: fp64 [N, width]} per task."""
    x = np.asarray(feats, np.float64)
    ks = kernel_size(cfg)
    nb, own = neighbour_table(indices, ks), np.arange(len(indices)).reshape(-1, 1)
    out = []
    for i in range(len(cfg.CLASS_NAMES_EACH_HEAD)):
        task = {}
        for name in branch_names(cfg):
            num_conv = cfg.NUM_HM_CONV if name == "hm" else cfg.SEPARATE_HEAD_CFG.HEAD_DICT[name]["num_conv"]
            y, p = x, f"heads_list.{i}.{name}"
            for k in range(num_conv - 1):
                y = _subm(y, nb, sd[f"{p}.{k}.0.weight"], sd.get(f"{p}.{k}.0.bias"))
                q = f"{p}.{k}.1"
                scale = np.asarray(sd[q + ".weight"], np.float64) / np.sqrt(np.asarray(sd[q + ".running_var"], np.float64) + eps)
                y = np.maximum((y - np.asarray(sd[q + ".running_mean"], np.float64)) * scale + np.asarray(sd[q + ".bias"], np.float64), 0.0)
            task[name] = _subm(y, own, sd[f"{p}.{num_conv - 1}.weight"], sd[f"{p}.{num_conv - 1}.bias"])
        out.append(task)
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# top-K + decode over rows
# --------------------------------------------------------------------------------------------------------------------------------
def decode_ref(task, indices, batch, k, stride, voxel_xy, range_xy, limit, thresh, class_ids, extra=8):
    """One task's rows {branch: [N, c]} (fp32 values) -> per scene a dict with center_head_cases.decode_ref's fields; `flat` is
    class * N + stored row (the kernel's tie order), `rows` the stored rows of the survivors."""
    indices = np.asarray(indices)
    n = len(indices)
    hm = np.asarray(task["hm"]).reshape(n, -1)
    out = []
    for s in range(batch):
        rows = np.nonzero(indices[:, 0] == s)[0]
        n_b = len(rows)
        sc = scores32(hm[rows].T).reshape(-1)                                   # [n_cls, n_b], class-major
        with np.errstate(invalid="ignore"):
            order = np.lexsort((np.arange(sc.size), -np.where(np.isnan(sc), np.inf, sc.astype(np.float64))))
        top = order[:k]
        cls = top // max(n_b, 1)
        r = rows[top % max(n_b, 1)] if n_b else np.zeros(0, np.int64)

        def g(name):
            return np.asarray(task[name], np.float64).reshape(n, -1)[r]

        center, z, dim, rot = g("center"), g("center_z"), np.exp(g("dim")), g("rot")
        x = (indices[r, 2] + center[:, 0]) * stride * voxel_xy[0] + range_xy[0]
        y = (indices[r, 1] + center[:, 1]) * stride * voxel_xy[1] + range_xy[1]
        parts = [x[:, None], y[:, None], z, dim, np.arctan2(rot[:, 1], rot[:, 0])[:, None]] + ([g("vel")] if "vel" in task else [])
        boxes = np.concatenate(parts, axis=1)
        lim = np.asarray(limit, np.float64)
        mask = (boxes[:, :3] >= lim[:3]).all(1) & (boxes[:, :3] <= lim[3:]).all(1)
        if thresh is not None:
            with np.errstate(invalid="ignore"):
                mask &= sc[top] > np.float32(thresh)
        out.append(dict(boxes=boxes[mask], scores=sc[top][mask], labels=np.asarray(class_ids)[cls][mask], flat=(cls * n + r)[mask], rows=r[mask],
                        cand_scores=sc[order[:min(k + extra, sc.size)]], cand_boxes=boxes, n_b=n_b))
    return out


def head_final(cfg, class_names, rows, indices, batch, stride, voxel_size, point_cloud_range):
    """rows: one {branch: [N, c]} per task (fp32 values).  Returns (pre: [task][scene] decode_ref dicts, final: [scene] dicts of
    pred_boxes / pred_scores / pred_labels (1-based), smallest |iou - NMS_THRESH| met, candidates NMS removed)."""
    post = cfg.POST_PROCESSING
    nms = post.NMS_CONFIG
    pre, near, removed = [], np.inf, 0
    final = [dict(pred_boxes=[], pred_scores=[], pred_labels=[]) for _ in range(batch)]
    for i, heads in enumerate(cfg.CLASS_NAMES_EACH_HEAD):
        ids = [class_names.index(x) for x in heads if x in class_names]
        dec = decode_ref(rows[i], indices, batch, post.MAX_OBJ_PER_SAMPLE, stride, voxel_size[:2], point_cloud_range[:2],
                         post.POST_CENTER_LIMIT_RANGE, post.get("SCORE_THRESH"), ids)
        pre.append(dec)
        for s, d in enumerate(dec):
            keep, m = greedy_nms(d["boxes"], nms.NMS_THRESH, nms.NMS_PRE_MAXSIZE, nms.NMS_POST_MAXSIZE)
            near = min(near, m)
            removed += min(len(d["boxes"]), nms.NMS_PRE_MAXSIZE) - len(keep)
            final[s]["pred_boxes"].append(d["boxes"][keep])
            final[s]["pred_scores"].append(d["scores"][keep])
            final[s]["pred_labels"].append(d["labels"][keep] + 1)
    for f in final:
        for key in f:
            f[key] = np.concatenate(f[key], axis=0)
    return pre, final, near, removed


def f32_rows(rows64):
    return [{n: np.asarray(a, np.float32) for n, a in t.items()} for t in rows64]


def case_eval(name, xseed=None):
    c, cfg = CASES[name], case_cfg(name)
    feats, idx = case_input(name, xseed)
    rows64 = head_rows(cfg, case_state(name), feats, idx)
    pre, final, near, removed = head_final(cfg, c["class_names"], f32_rows(rows64), idx, 2, c["stride"], c["voxel_size"], c["point_cloud_range"])
    return rows64, pre, final, near, removed


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(rows64, pre, final, near, removed) of a case from the restatement alone (computed once, shared; do not write to it)."""
    return case_eval(name)


def limit_drops(cfg, pre):
    """candidates that pass the score threshold and fall to the limit range, over tasks and scenes"""
    post = cfg.POST_PROCESSING
    lim, th, n = np.asarray(post.POST_CENTER_LIMIT_RANGE, np.float64), post.get("SCORE_THRESH"), 0
    for task in pre:
        for d in task:
            k = len(d["cand_boxes"])
            ok = d["cand_scores"][:k] > np.float32(th) if th is not None else np.ones(k, bool)
            c = d["cand_boxes"][:, :3]
            n += int((ok & ~((c >= lim[:3]).all(1) & (c <= lim[3:]).all(1))).sum())
    return n


def module_margins(cfg, pre, near):
    """center_head_cases.module_margins over the row-form decode."""
    return CC.module_margins(cfg, pre, near)


# --------------------------------------------------------------------------------------------------------------------------------
# kernel cases the first suite does not reach (tests/test_gpu_voxelnext_head_edges.py; conditions in tests/test_head_edges_conditions.py)
# --------------------------------------------------------------------------------------------------------------------------------
TASK_C = 16
# widths per branch of every task: at most four branches per task, so lvq_sparse_head launches its four-branch kernel
EDGE_LAYOUTS = {"two": [[4, 1]], "one": [[1]], "three_four": [[2, 1, 3], [2, 1, 3, 2]]}
EDGE_SIZES = [(name, kvol, n) for name in EDGE_LAYOUTS for kvol in (1, 9) for n in (1, 65, 200)]
WIDE_PITCH_LAYOUT = [[2, 1, 3, 2, 3], [2, 1, 3, 2, 2]]                           # five branches, operands pitched for eight
STRUCTURED_OFFSETS = [(0, 4), (4,), (4, 8), tuple(range(9))]                      # rows 0-15, 16-31, 32-47, 48-63 of every 64-row tile


def edge_table(kind, n, rng):
    """[n, 9] int32 neighbour table, the centre (offset 4) always the row itself.  random60: head_case's 60 % fill with out-of-range
    entries; sparse5: a 5 % fill; structured: STRUCTURED_OFFSETS by the row's place in its tile (neighbours drawn from all rows)."""
    if kind == "structured":
        nbr = np.full((n, 9), -1, np.int64)
        for r in range(n):
            for o in STRUCTURED_OFFSETS[(r % 64) // 16]:
                nbr[r, o] = rng.integers(0, n)
    else:
        fill = 0.6 if kind == "random60" else 0.05
        nbr = np.where(rng.random((n, 9)) < fill, rng.integers(0, n, (n, 9)), -1)
        if kind == "random60":
            nbr = nbr.astype(np.int32)
            nbr[:, 4] = np.arange(n)
            bad = rng.random((n, 9)) < 0.08                                      # out-of-range entries read as absent
            bad[:, 4] = False
            nbr[bad] = rng.choice(np.array([n, n + 5, -7, 2 ** 31 - 1], np.int64), int(bad.sum())).astype(np.int32)
    nbr[:, 4] = np.arange(n)
    return nbr.astype(np.int32)


def tile_lacks(nbr, n):
    """Per 64-row tile the offsets no row of it has (the kernel skips them), and per (tile, 16-row block) the offsets it lacks."""
    ok = (nbr >= 0) & (nbr < n)
    tiles = [[o for o in range(9) if not ok[t:t + 64, o].any()] for t in range(0, n, 64)]
    blocks = [[[o for o in range(9) if not ok[t + q:min(t + q + 16, t + 64), o].any()] for q in range(0, 64, 16) if t + q < n]
              for t in range(0, n, 64)]
    return tiles, blocks


def sparse_head_case(rng, widths, n, kvol, bs=None, table="random60"):
    """Operands of one lvq_sparse_head call and its fp64 result [16 T, n], drawn from rng: THE builder of the kernel cases (the first
    suite's head_case and edge_head_case below seed it).  widths: per task the output channels of its branches; bs: the branch pitch of
    the operands (None: the largest branch count; slots behind a task's branches hold values the kernel must not read into its result);
    table: edge_table's kind for k_vol 9."""
    n_tasks = len(widths)
    bs = max(len(w) for w in widths) if bs is None else bs
    feat = rng.standard_normal((n, C)).astype(np.float32)
    nbr = edge_table(table, n, rng) if kvol == 9 else None
    fill = {"random60": 0.6, "sparse5": 0.05, "structured": 0.4}[table]
    w1 = (rng.standard_normal((n_tasks, bs, C, kvol, C)) * np.sqrt(2.0 / (C * max(1.0, fill * kvol)))).astype(np.float32)     # [C_out, K, C_in]
    scale = (1.0 + 0.1 * rng.standard_normal((n_tasks, bs, C))).astype(np.float32)
    shift = (0.1 * rng.standard_normal((n_tasks, bs, C))).astype(np.float32)
    w_last = (rng.standard_normal((n_tasks, TASK_C, C)) / np.sqrt(C)).astype(np.float32)
    bias = rng.standard_normal((n_tasks, TASK_C)).astype(np.float32)
    owner = [sum(([j] * w for j, w in enumerate(ws)), []) for ws in widths]
    owner = [o + [-1] * (TASK_C - len(o)) for o in owner]
    ref = np.zeros((TASK_C * n_tasks, n))
    tbl = np.arange(n).reshape(n, 1) if nbr is None else np.where((nbr >= 0) & (nbr < n), nbr, -1)
    f64 = feat.astype(np.float64)
    for ti, ws in enumerate(widths):
        for j in range(len(ws)):
            mid = np.zeros((n, C))
            for o in range(kvol):
                g = np.where((tbl[:, o] >= 0)[:, None], f64[np.maximum(tbl[:, o], 0)], 0.0)
                mid += g @ w1[ti, j, :, o].astype(np.float64).T
            mid = np.maximum(mid * scale[ti, j] + shift[ti, j], 0.0)
            for c in range(TASK_C):
                if owner[ti][c] == j:
                    ref[TASK_C * ti + c] = mid @ w_last[ti, c].astype(np.float64) + bias[ti, c]
    return dict(feat=feat, nbr=nbr, w1=w1, scale=scale, shift=shift, w_last=w_last, bias=bias, owner=owner, n_br=[len(w) for w in widths],
                bs=bs, ref=ref)


@functools.lru_cache(maxsize=None)
def edge_head_case(layout, n, kvol, bs=None, table="random60", seed=211):
    """sparse_head_case for a key of EDGE_LAYOUTS or "wide_pitch"."""
    widths = WIDE_PITCH_LAYOUT if layout == "wide_pitch" else EDGE_LAYOUTS[layout]
    rng = np.random.default_rng([seed, n, kvol, len(widths), sorted(list(EDGE_LAYOUTS) + ["wide_pitch"]).index(layout)])
    return sparse_head_case(rng, widths, n, kvol, bs, table)


DECODE_NAMES = ("center", "center_z", "dim", "rot", "vel", "hm")


def task_rows(rng, n, n_cls, vel):
    """One task's branch outputs for n rows, in the order hm, center, center_z, dim, rot, vel."""
    task = dict(hm=rng.uniform(-5.0, 1.0, (n, n_cls)).astype(np.float32), center=rng.uniform(0, 1, (n, 2)).astype(np.float32),
                center_z=rng.normal(size=(n, 1)).astype(np.float32), dim=rng.normal(-0.5, 0.3, (n, 3)).astype(np.float32),
                rot=rng.normal(size=(n, 2)).astype(np.float32))
    if vel:
        task["vel"] = rng.normal(size=(n, 2)).astype(np.float32)
    return task


def scene_rows(rng, n_rows, grid, extra=(), interleave=True):
    """[N, 3] int32 (b, y, x): n_rows[s] distinct cells of a grid x grid map per scene, then the rows `extra`, all shuffled together."""
    idx = []
    for s, m in enumerate(n_rows):
        idx += [(s, int(c) // grid, int(c) % grid) for c in rng.permutation(grid * grid)[:m]]
    idx = np.array(idx + list(extra), np.int32).reshape(-1, 3)
    return idx[rng.permutation(len(idx))] if interleave and len(idx) else idx


def head_buffer(tasks):
    """[{branch: [N, c]}] -> (channel-major [16 T, N] fp32 buffer, task_channels): task t's branches from channel 16 t on."""
    n = len(tasks[0]["hm"])
    buf = np.zeros((TASK_C * len(tasks), n), np.float32)
    chans = []
    for t, task in enumerate(tasks):
        row, o = [], TASK_C * t
        for name in DECODE_NAMES:
            if name in task:
                wd = task[name].shape[1]
                buf[o:o + wd] = task[name].T
                row.append(o)
                o += wd
            else:
                row.append(-1)
        chans.append(row)
    return buf, chans


MULTI_N_CLS, MULTI_IDS, MULTI_K, MULTI_ROWS = (1, 2, 3), [[7], [2, 9], [4, 0, 5]], 32, (60, 45, 50)
MULTI_SEED = 343                                # the first from 311 on whose nine (task, scene) groups keep decode_margins' distances


@functools.lru_cache(maxsize=None)
def multi_task_case():
    """Three tasks of 1, 2 and 3 classes with vel (box_dim 9) on one set of rows: three scenes interleaved on an 8 x 8 grid, with rows of
    b = batch and b = -1 among them whose scores would win everywhere.  -> (indices [N, 3], tasks)."""
    rng = np.random.default_rng(MULTI_SEED)
    idx = scene_rows(rng, MULTI_ROWS, 8, [(3, 1, 1), (3, 2, 5), (-1, 3, 3), (3, 6, 6), (-1, 0, 7)])
    tasks = [task_rows(rng, len(idx), c, True) for c in MULTI_N_CLS]
    foreign = (idx[:, 0] < 0) | (idx[:, 0] >= 3)
    for t in tasks:
        t["hm"][foreign] = 9.0
    return idx, tasks


PLATEAU_ROWS, PLATEAU_K, PLATEAU_ABOVE, PLATEAU_EQUAL, PLATEAU_LOGIT = (100, 1300, 100), 64, 23, 700, 0.5


@functools.lru_cache(maxsize=None)
def plateau_case():
    """Scene 1 of 3 has 1300 rows of 2 classes: 23 (row, class) pairs with distinct scores above a plateau of 700 pairs that share one
    score, everything else far below; K = 64 ends inside the plateau.  The 1500 rows of the three scenes are interleaved, so the kernel's
    3000 positions (three per thread) carry the other scenes' zero keys between the plateau's members.  -> (indices, task)."""
    rng = np.random.default_rng(312)
    idx = scene_rows(rng, PLATEAU_ROWS, 40, [])
    n = len(idx)
    task = task_rows(rng, n, 2, False)
    rows1 = np.nonzero(idx[:, 0] == 1)[0]
    task["hm"][rows1] = rng.uniform(-6.0, -3.0, (len(rows1), 2)).astype(np.float32)
    pairs = rng.permutation(2 * len(rows1))
    high, level = pairs[:PLATEAU_ABOVE], pairs[PLATEAU_ABOVE:PLATEAU_ABOVE + PLATEAU_EQUAL]
    task["hm"][rows1[high % len(rows1)], high // len(rows1)] = np.linspace(1.0, 2.1, PLATEAU_ABOVE).astype(np.float32)
    task["hm"][rows1[level % len(rows1)], level // len(rows1)] = PLATEAU_LOGIT
    return idx, task


def plateau_stats(idx, task, scene, k, threads=1024):
    """(above, equal, need, keys per thread, threads whose range holds a plateau key, foreign positions between the first and the last
    plateau member) of the select over the n_cls * N positions class * N + stored row."""
    n = len(idx)
    sc = scores32(np.asarray(task["hm"]).T).reshape(-1)                           # position class * N + row
    mine = np.tile(idx[:, 0] == scene, task["hm"].shape[1])
    kth = np.sort(sc[mine])[::-1][k - 1]
    above, equal = int((sc[mine] > kth).sum()), int((sc[mine] == kth).sum())
    chunk = -(-sc.size // threads)
    level = mine & (sc == kth)
    where = np.nonzero(level)[0]
    owners = len(set((where // chunk).tolist()))
    between = int((~mine[where[0]:where[-1]]).sum())
    return above, equal, k - above, chunk, owners, between
