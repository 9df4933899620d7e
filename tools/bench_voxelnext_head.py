#!/usr/bin/env python3
"""Timing of sparse_head.VoxelNeXtHead.forward at the shape of cbgs_voxel0075_voxelnext: the nuScenes head (six tasks, ten classes, vel,
36 branch pairs) on the 180 x 180 stride-8 BEV grid, B = 4, with KERNEL_SIZE_HEAD 1 (the shipped configs) and 3 (the class default),
next to the same forward composed only of what existed before lvq_sparse_head / lvq_voxel_decode:

  composed route   SubMConv2d.run(bn=, relu=True) per branch for the first convs (36 lvq_sparse_conv launches, each writing [N, 128] fp32),
                   a torch fp32 matmul + bias per branch for the last convs, and the LVQ_HEAD_TORCH_POST sequence of torch ops for the rest
  fused route      one lvq_sparse_head, one lvq_voxel_decode, one lvq_nms_bev, one lvq_center_collect

Rows: 22490 active rows per scene of the 32400 cells (69 %), which is what VoxelResBackBone8xVoxelNeXt's own benchmark finds at its 2-D
stage for one 32768-point scene stretched to +-54 m (profiles/backbone3d.json: `shared_conv.0` rows_out); the occupied cells are a
seeded choice, listed ascending in (b, y, x) as the backbone lists them.  Features are a ReLU'd seeded normal.  Report only.

  forward_ms   host clock around whole forwards (a forward ends in a device-to-host copy); the two routes alternate inside one window,
               `reps` windows after a warm-up: median, smallest, largest
  stages_us    device events around the fused convs, the decode, NMS and collect (ops.EVENTS), and around the composed route's first
               convs, last convs and post-processing, in runs of their own: median over `iters`, with min and max
  bytes        what each route's conv stage moves through HBM, counted from the shapes (not measured)
  frac         the fused kernel's fraction of the HBM peak (8 TB/s) and of the dense bf16 MFMA peak (2.5 PFLOP/s), from the counted bytes /
               executed MFMA flops and the median time

    python tools/bench_voxelnext_head.py [--batch 4] [--size 180] [--rows 22490] [--k 500] [--iters 10] [--reps 5] [--out profiles/voxelnext_head.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lidar_vision_vqa_amd import backbone3d as B3, ops, sparse_head as SH, synth  # noqa: E402

CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
HEADS = [["car"], ["truck", "construction_vehicle"], ["bus", "trailer"], ["barrier"], ["motorcycle", "bicycle"], ["pedestrian", "traffic_cone"]]
HBM_PEAK, MFMA_PEAK = 8.0e12, 2.5e15


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


def config(k, ks):
    names = ["center", "center_z", "dim", "rot", "vel"]
    width = dict(center=2, center_z=1, dim=3, rot=2, vel=2)
    return Cfg(CLASS_NAMES_EACH_HEAD=HEADS, SHARED_CONV_CHANNEL=128, KERNEL_SIZE_HEAD=ks, USE_BIAS_BEFORE_NORM=True, NUM_HM_CONV=2,
               SEPARATE_HEAD_CFG=Cfg(HEAD_ORDER=names, HEAD_DICT=Cfg({n: Cfg(out_channels=width[n], num_conv=2) for n in names})),
               TARGET_ASSIGNER_CONFIG=Cfg(FEATURE_MAP_STRIDE=8),
               POST_PROCESSING=Cfg(SCORE_THRESH=0.1, POST_CENTER_LIMIT_RANGE=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], MAX_OBJ_PER_SAMPLE=k,
                                   NMS_CONFIG=Cfg(NMS_TYPE="nms_gpu", NMS_THRESH=0.2, NMS_PRE_MAXSIZE=1000, NMS_POST_MAXSIZE=83)))


def build(k, ks, dev):
    head = SH.VoxelNeXtHead(config(k, ks), 128, 10, CLASSES, np.array([1440, 1440, 40]), [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], [0.075, 0.075, 0.2])
    synth.load_seeded(head, 93)
    with torch.no_grad():
        for h in head.heads_list:
            h.hm[-1].weight.mul_(6.0)
            h.hm[-1].bias.fill_(-2.19)
            h.dim[-1].bias.fill_(0.5)
    return head.to(dev).eval()


def rows(batch, size, per_scene, dev):
    rng = np.random.default_rng(94)
    idx = []
    for b in range(batch):
        cells = np.sort(rng.permutation(size * size)[:per_scene])
        idx.append(np.stack([np.full(per_scene, b), cells // size, cells % size], axis=1))
    idx = torch.from_numpy(np.concatenate(idx).astype(np.int32)).to(dev)
    g = torch.Generator(device=dev).manual_seed(95)
    return torch.relu(torch.randn((idx.shape[0], 128), device=dev, generator=g)), idx


def tensor(feats, idx, size, batch, mode):
    return B3.SparseConvTensor(feats, idx, [size, size], batch, precision=mode)


def fused(head, feats, idx, size, batch, mode):
    os.environ.pop("LVQ_HEAD_TORCH_POST", None)
    with torch.no_grad():
        return head(dict(encoded_spconv_tensor=tensor(feats, idx, size, batch, mode), batch_size=batch))["final_box_dicts"]


def composed(head, feats, idx, size, batch, mode, ev=None):
    """The forward from SubMConv2d.run per branch, torch matmuls and the torch post-processing.  ev: {stage: [(start, end)]} device events."""
    def mark(tag):
        if ev is None:
            return None
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev.setdefault(tag, []).append((s, e))
        s.record()
        return e

    with torch.no_grad():
        x = tensor(feats, idx, size, batch, mode)
        e = mark("first_convs")
        mids = [{n: getattr(h, n)[0][0].run(x, bn=getattr(h, n)[0][1], relu=True).features for n in h.sep_head_dict} for h in head.heads_list]
        e and e.record()
        e = mark("last_convs")
        pred = []
        for h, m in zip(head.heads_list, mids):
            pred.append({n: m[n] @ getattr(h, n)[1].weight.reshape(-1, 128).t() + getattr(h, n)[1].bias for n in h.sep_head_dict})
        e and e.record()
        head.forward_ret_dict["pred_dicts"] = pred
        e = mark("torch_post")
        out = head._torch_post(batch, idx, head._post_cfg())
        e and e.record()
    return out


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=180)
    ap.add_argument("--rows", type=int, default=22490)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_voxelnext_head.py times the MI355X kernels: no GPU, no number"
    dev = torch.device("cuda:0")
    feats, idx = rows(a.batch, a.size, a.rows, dev)
    n, n_tasks, n_pairs = feats.shape[0], len(HEADS), 36
    res = dict(rows=n, rows_per_scene=a.rows, grid=[a.size, a.size], batch=a.batch, k=a.k, tasks=n_tasks, branch_pairs=n_pairs, iters=a.iters,
               reps=a.reps, rows_from="profiles/backbone3d.json: shared_conv.0 rows_out of one scene")
    for ks in (1, 3):
        head = build(a.k, ks, dev)
        kvol = ks * ks
        for mode in ("bf16x3", "bf16"):
            head.precision = mode
            lists, lists_c = fused(head, feats, idx, a.size, a.batch, mode), composed(head, feats, idx, a.size, a.batch, mode)
            same = all(len(p["pred_labels"]) == len(q["pred_labels"]) and torch.equal(p["pred_labels"], q["pred_labels"]) for p, q in zip(lists, lists_c))
            for _ in range(2):
                fused(head, feats, idx, a.size, a.batch, mode), composed(head, feats, idx, a.size, a.batch, mode)
            torch.cuda.synchronize()
            win = {"fused": [], "composed": []}
            for _ in range(a.reps):
                acc = {"fused": 0.0, "composed": 0.0}
                for _ in range(a.iters):
                    for route, fn in (("fused", fused), ("composed", composed)):      # the two routes alternate inside the window
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn(head, feats, idx, a.size, a.batch, mode)
                        torch.cuda.synchronize()
                        acc[route] += time.perf_counter() - t0
                for route in acc:
                    win[route].append(1e3 * acc[route] / a.iters)
            ops.EVENTS = {}
            try:
                for _ in range(a.iters):
                    fused(head, feats, idx, a.size, a.batch, mode)
                torch.cuda.synchronize()
                stages = {tag: stats([s.elapsed_time(e) * 1e3 for s, e in ev]) for tag, ev in ops.EVENTS.items()}
            finally:
                ops.EVENTS = None
            ev = {}
            for _ in range(a.iters):
                composed(head, feats, idx, a.size, a.batch, mode, ev)
            torch.cuda.synchronize()
            stages_c = {tag: stats([s.elapsed_time(e) * 1e3 for s, e in v]) for tag, v in ev.items()}
            # bytes through HBM of the conv stage, from the shapes: the features are gathered per offset (a row's 512 bytes per present
            # neighbour; kvol 9 at 69 % occupancy reads about 6.5 rows per output row), weights are read once per workgroup from L2
            nb = 1.0 if ks == 1 else 1.0 + 8 * a.rows / (a.size * a.size)
            w_bytes = n_pairs * kvol * 128 * 128 * 2 * (2 if mode == "bf16x3" else 1)
            fused_bytes = n_tasks * n * 512 * nb + 16 * n_tasks * n * 4 + w_bytes
            comp_bytes = n_pairs * (n * 512 * nb + n * 512) + n_pairs * n * 512 + sum(2 + 1 + 3 + 2 + 2 + len(h) for h in HEADS) * n * 4 + w_bytes
            flops = 2.0 * n * 128 * 128 * nb * n_pairs * (3 if mode == "bf16x3" else 1)
            t_f = stages["voxelnext_head_convs"]["median"] * 1e-6
            res[f"ks{ks}_{mode}"] = dict(
                forward_ms={r: stats(w) for r, w in win.items()}, stages_us=dict(fused=stages, composed=stages_c),
                conv_stage_bytes=dict(fused=int(fused_bytes), composed=int(comp_bytes)), mfma_flops_executed=flops,
                fused_frac_hbm_peak=fused_bytes / t_f / HBM_PEAK, fused_frac_mfma_peak=flops / t_f / MFMA_PEAK,
                conv_stage_speedup=(stages_c["first_convs"]["median"] + stages_c["last_convs"]["median"]) / stages["voxelnext_head_convs"]["median"],
                boxes_per_scene=[int(len(p["pred_scores"])) for p in lists], routes_agree_on_labels=bool(same))
            print(f"ks{ks}_{mode}", json.dumps(res[f"ks{ks}_{mode}"]))
    res["launches"] = dict(fused_route=dict(rules="1 (KERNEL_SIZE_HEAD 3 only)", convs=1, decode=1, nms=2, collect=1, device_to_host_copies=1),
                           composed_route=f"{n_pairs} lvq_sparse_conv + {n_pairs} matmuls, 6 rule tables (one per branch name) with KERNEL_SIZE_HEAD 3; per "
                                          f"scene and task a top-k pair, gathers, a mask, one lvq_boxes_iou_bev and one device-to-host copy: {a.batch * n_tasks} host round trips")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
