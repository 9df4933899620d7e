#!/usr/bin/env python3
"""Timing of dense_head.CenterHead.forward at the reference's own shape (cbgs_voxel0075_res3d_centerpoint): B = 4 scenes,
spatial_features_2d [4, 512, 180, 180], six tasks / ten classes with vel, MAX_OBJ_PER_SAMPLE = 500, NMS 0.2 / 1000 / 83, next to the
LVQ_HEAD_TORCH_POST=1 route (the reference's sequence of torch ops on the same maps, NMS through lvq_boxes_iou_bev and a host walk) on
the same device.  Report only: there is no pass / fail time.  The post-processing is latency-bound, so the launch and copy counts stand
next to the times.

  forward_ms   host clock around whole forwards (a forward ends in its device-to-host copy, so the clock sees finished work); the two routes
               alternate inside one window, `reps` windows after a warm-up: median, smallest, largest
  stages_us    device events around the conv stack (lvq_conv2d_to_planes + 13 lvq_conv2d) and around each post-processing call, in a run
               of their own (the events add host work between launches)
  launches     counted from the module's plan, not measured: 1 + 1 + 2 per task conv launches, 1 decode, 2 NMS, 1 collect; 1 copy

  conv_roles   the conv stack's launches by role (shared conv, the tasks' fused first convs, the tasks' block-diagonal last convs) next to
               the post-processing calls, device events around every launch summed per forward, again in a run of their own

Weights are seeded (synth.load_seeded, hm bias -2.19 as the reference initialises it, hm filters scaled up so that all K candidates of
every task pass SCORE_THRESH: the largest NMS problem the configuration allows); the input is a ReLU'd seeded normal map.

    python tools/bench_center_head.py [--batch 4] [--size 180] [--iters 10] [--reps 5] [--out profiles/center_head.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lidar_vision_vqa_amd import backbone2d as B2, dense_head as DH, ops, synth  # noqa: E402

CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
HEADS = [["car"], ["truck", "construction_vehicle"], ["bus", "trailer"], ["barrier"], ["motorcycle", "bicycle"], ["pedestrian", "traffic_cone"]]


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


def config(k):
    names = ["center", "center_z", "dim", "rot", "vel"]
    width = dict(center=2, center_z=1, dim=3, rot=2, vel=2)
    return Cfg(CLASS_NAMES_EACH_HEAD=HEADS, SHARED_CONV_CHANNEL=64, USE_BIAS_BEFORE_NORM=True, NUM_HM_CONV=2,
               SEPARATE_HEAD_CFG=Cfg(HEAD_ORDER=names, HEAD_DICT=Cfg({n: Cfg(out_channels=width[n], num_conv=2) for n in names})),
               TARGET_ASSIGNER_CONFIG=Cfg(FEATURE_MAP_STRIDE=8),
               POST_PROCESSING=Cfg(SCORE_THRESH=0.1, POST_CENTER_LIMIT_RANGE=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], MAX_OBJ_PER_SAMPLE=k,
                                   NMS_CONFIG=Cfg(NMS_TYPE="nms_gpu", NMS_THRESH=0.2, NMS_PRE_MAXSIZE=1000, NMS_POST_MAXSIZE=83)))


def build(k, dev):
    head = DH.CenterHead(config(k), 512, 10, CLASSES, np.array([1440, 1440, 40]), [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], [0.075, 0.075, 0.2],
                         predict_boxes_when_training=False)
    synth.load_seeded(head, 91)
    with torch.no_grad():
        for h in head.heads_list:
            h.hm[-1].weight.mul_(6.0)
            h.hm[-1].bias.fill_(-2.19)
            h.dim[-1].bias.fill_(0.5)
    return head.to(dev).eval()


def forward(head, x, torch_post):
    if torch_post:
        os.environ["LVQ_HEAD_TORCH_POST"] = "1"
    else:
        os.environ.pop("LVQ_HEAD_TORCH_POST", None)
    with torch.no_grad():
        return head(dict(spatial_features_2d=x, batch_size=x.shape[0]))["final_box_dicts"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=180)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_center_head.py times the MI355X kernels: no GPU, no number"
    dev = torch.device("cuda:0")
    head = build(a.k, dev)
    g = torch.Generator(device=dev).manual_seed(92)
    x = torch.relu(torch.randn((a.batch, 512, a.size, a.size), device=dev, generator=g))
    res = dict(shape=[a.batch, 512, a.size, a.size], k=a.k, tasks=len(HEADS), iters=a.iters, reps=a.reps)
    for mode in ("bf16x3", "bf16"):
        head.precision = mode
        lists = forward(head, x, False)
        pre = head.forward_ret_dict["candidate_counts"].clone()         # [B, n_tasks] survivors of the decode, before NMS
        lists_t = forward(head, x, True)
        same = all(torch.equal(p["pred_labels"], q["pred_labels"]) and torch.allclose(p["pred_boxes"], q["pred_boxes"], atol=1e-5) for p, q in zip(lists, lists_t))
        for _ in range(2):
            forward(head, x, False), forward(head, x, True)
        torch.cuda.synchronize()
        win = {False: [], True: []}
        for _ in range(a.reps):
            acc = {False: 0.0, True: 0.0}
            for _ in range(a.iters):
                for route in (False, True):                   # the two routes alternate inside the window
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    forward(head, x, route)
                    torch.cuda.synchronize()
                    acc[route] += time.perf_counter() - t0
            for route in acc:
                win[route].append(1e3 * acc[route] / a.iters)
        # stages: device events, in a run of their own
        os.environ.pop("LVQ_HEAD_TORCH_POST", None)
        ops.EVENTS = {}
        real = head._maps

        def maps(xx, split):
            with ops.region("convs", dev):
                return real(xx, split)

        head._maps = maps
        try:
            for _ in range(a.iters):
                forward(head, x, False)
            torch.cuda.synchronize()
            stages = {tag: float(np.median([s.elapsed_time(e) for s, e in ev])) * 1e3 for tag, ev in ops.EVENTS.items()}
        finally:
            ops.EVENTS = None
            del head._maps
        roles = {id(head._plan()["shared"]): "shared_conv"}
        for t in head._plan()["tasks"]:
            roles[id(t["first"])], roles[id(t["last"])] = "first_convs", "last_convs_block_diagonal"
        run_real, ops.EVENTS = B2._Layer.run, {}

        def run(self, *args, **kw):
            with ops.region(roles[id(self)], dev):
                return run_real(self, *args, **kw)

        B2._Layer.run = run
        try:
            for _ in range(a.iters):
                forward(head, x, False)
            torch.cuda.synchronize()
            conv_roles = {tag: sum(s.elapsed_time(e) for s, e in ev) * 1e3 / a.iters for tag, ev in ops.EVENTS.items()}
        finally:
            B2._Layer.run, ops.EVENTS = run_real, None
        res[mode] = dict(conv_roles_us=conv_roles,
            forward_ms={("torch_post" if r else "kernels"): dict(median=float(np.median(w)), min=float(min(w)), max=float(max(w))) for r, w in win.items()},
            stages_us=stages, candidates_per_group=dict(mean=float(pre.float().mean()), max=int(pre.max())),
            boxes_per_scene=[int(len(p["pred_scores"])) for p in lists], routes_agree=bool(same))
        print(mode, json.dumps(res[mode]))
    n_tasks = len(HEADS)
    res["launches"] = dict(kernels_route=dict(convs=2 + 2 * n_tasks, decode=1, nms=2, collect=1, device_to_host_copies=1),
                           torch_post_route="two torch.topk, about a dozen gathers and one mask per task; per scene and task a compaction, a top-k, "
                                            f"a sort, one lvq_boxes_iou_bev and one device-to-host copy of its mask: {a.batch * n_tasks} host round trips")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
