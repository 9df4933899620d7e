#!/usr/bin/env python3
"""Timing of anchor_head.AnchorHeadSingle.forward + anchor_head.post_processing at the shape of kitti_models/pointpillar.yaml: B = 4 scenes,
spatial_features_2d [4, 384, 248, 216], 3 classes x 2 rotations = 6 anchors per cell (321 408 per scene), direction classifier,
SCORE_THRESH 0.1, NMS 0.01 / 4096 / 500, next to the LVQ_HEAD_TORCH_POST=1 route (the reference's sequence of torch ops on the same dense
outputs, NMS through lvq_boxes_iou_bev and a host walk) on the same device.  Report only: there is no pass / fail time.

  whole_ms     host clock around forward + post_processing (a call ends in its device-to-host copy, so the clock sees finished work); the
               two routes alternate inside one window, `reps` windows after a warm-up: median, smallest, largest
  stages_us    device events around the conv launch (lvq_conv2d_to_planes + the fused 1 x 1 lvq_conv2d) and around each kernel call, in a
               run of their own (the events add host work between launches): median per call
  decode       the bytes lvq_anchor_decode has to move, computed from the shapes -- the cls | box | dir channel planes in, the anchors in,
               the logits, boxes, scores and labels out, the candidate list out -- over its median time, next to the HBM peak
               (8.0 TB/s by the data sheet, about 6.3 TB/s for a float4 copy)

Weights are seeded (synth.load_seeded); the cls biases are then shifted so that about `--survivors` anchors per scene reach SCORE_THRESH
(a forward on the seeded input gives the quantile); the input is a ReLU'd seeded normal map.

    python tools/bench_anchor_head.py [--batch 4] [--iters 20] [--reps 5] [--survivors 3000] [--out profiles/anchor_head.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lidar_vision_vqa_amd import anchor_head as AH, ops, synth  # noqa: E402

CLASSES = ["Car", "Pedestrian", "Cyclist"]
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


def config():
    sizes = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
    bottoms = [-1.78, -0.6, -0.6]
    gen = [Cfg(class_name=n, anchor_sizes=[s], anchor_rotations=[0, 1.57], anchor_bottom_heights=[b], align_center=False, feature_map_stride=2)
           for n, s, b in zip(CLASSES, sizes, bottoms)]
    head = Cfg(NAME="AnchorHeadSingle", USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
               ANCHOR_GENERATOR_CONFIG=gen, TARGET_ASSIGNER_CONFIG=Cfg(NAME="AxisAlignedTargetAssigner", BOX_CODER="ResidualCoder"), LOSS_CONFIG=Cfg())
    post = Cfg(SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False,
               NMS_CONFIG=Cfg(MULTI_CLASSES_NMS=False, NMS_TYPE="nms_gpu", NMS_THRESH=0.01, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=500))
    return head, post


def run(head, post, x, torch_post):
    if torch_post:
        os.environ["LVQ_HEAD_TORCH_POST"] = "1"
    else:
        os.environ.pop("LVQ_HEAD_TORCH_POST", None)
    with torch.no_grad():
        out = head(dict(spatial_features_2d=x, batch_size=x.shape[0]))
        return AH.post_processing(out, post, len(CLASSES))[0], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--survivors", type=int, default=3000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_anchor_head.py times the MI355X kernels: no GPU, no number"
    dev = torch.device("cuda:0")
    cfg, post = config()
    c_in, h, w = 384, 248, 216
    head = AH.AnchorHeadSingle(cfg, c_in, len(CLASSES), CLASSES, np.array([432, 496, 1]), [0.0, -39.68, -3.0, 69.12, 39.68, 1.0])
    synth.load_seeded(head, 93)
    with torch.no_grad():
        head.conv_cls.bias.zero_()
        head.conv_box.bias.zero_()
        head.conv_box.weight.mul_(0.1)
    head = head.to(dev).eval()
    head.candidate_score_thresh = post.SCORE_THRESH
    g = torch.Generator(device=dev).manual_seed(94)
    x = torch.relu(torch.randn((a.batch, c_in, h, w), device=dev, generator=g))
    n = h * w * head.num_anchors_per_location
    # the cls bias that lets about `survivors` anchors per scene through: the quantile of the best logit on this very input
    _, out = run(head, post, x, False)
    best = out["batch_cls_preds"].max(-1)[0].flatten()
    cut = torch.kthvalue(best, best.numel() - a.survivors * a.batch)[0]
    with torch.no_grad():
        head.conv_cls.bias.fill_(float(np.log(0.1 / 0.9)) - float(cut))
    res = dict(shape=[a.batch, c_in, h, w], anchors_per_scene=n, iters=a.iters, reps=a.reps)
    n_cls, n_bins, A = len(CLASSES), 2, head.num_anchors_per_location
    for mode in ("bf16x3", "bf16"):
        head.precision = mode
        lists, out = run(head, post, x, False)
        lists_t, _ = run(head, post, x, True)
        same = all(torch.equal(p["pred_labels"], q["pred_labels"]) and torch.equal(p["pred_boxes"], q["pred_boxes"]) for p, q in zip(lists, lists_t))
        survivors = out["anchor_candidates"][2].tolist()
        for _ in range(2):
            run(head, post, x, False), run(head, post, x, True)
        torch.cuda.synchronize()
        win = {False: [], True: []}
        for _ in range(a.reps):
            acc = {False: 0.0, True: 0.0}
            for _ in range(a.iters):
                for route in (False, True):                   # the two routes alternate inside the window
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(head, post, x, route)
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
                run(head, post, x, False)
            torch.cuda.synchronize()
            stages = {tag: float(np.median([s.elapsed_time(e) for s, e in ev])) * 1e3 for tag, ev in ops.EVENTS.items()}
        finally:
            ops.EVENTS = None
            del head._maps
        moved = a.batch * (4 * A * (n_cls + 7 + n_bins) * h * w + 4 * n * (n_cls + 9)) + 28 * n + 4 * sum(survivors)
        rate = moved / (stages["anchor_decode"] * 1e-6)
        res[mode] = dict(
            whole_ms={("torch_post" if r else "kernels"): dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for r, v in win.items()},
            stages_us=stages, survivors_per_scene=survivors, boxes_per_scene=[int(len(p["pred_scores"])) for p in lists], routes_agree=bool(same),
            decode=dict(bytes=int(moved), bytes_per_s=rate, of_hbm_peak=rate / HBM_PEAK, of_float4_copy=rate / HBM_COPY))
        print(mode, json.dumps(res[mode]), flush=True)
    res["launches"] = dict(kernels_route=dict(to_planes=1, conv=1, decode="1 + a 16-byte memset", select=1, nms=2, collect=1, device_to_host_copies=1),
                           torch_post_route="per scene: sigmoid, max, a mask and its compaction, a top-k, a sort, one lvq_boxes_iou_bev and one "
                                            f"device-to-host copy of its [n, n] mask, two gathers: {a.batch} host round trips")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
