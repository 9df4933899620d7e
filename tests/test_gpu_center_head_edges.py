"""The routes of csrc/center_head.hip that tests/test_gpu_center_head.py does not enter, on the MI355X against the restatements of
tests/center_head_cases.py (tests/test_center_head_edges_conditions.py asserts every case's condition on the CPU).

  decode   the tie route of the top-K select (ranges of 2 and 3 cells per thread, a plateau behind larger keys, a plateau that fills the
           remainder exactly, saturated and zero scores), NaN and infinite logits, K = 1, 2, 3, 1023, 1024 and K = n on distinct scores,
           stride = 1, score_thresh=None, centres exactly on the limit range:
           winners' flat indices, order, labels and counts exact; boxes and scores at 1e-5 relative
  NMS      16 mask words, the thresholds 0.7 and 0.01, count clamps, garbage behind the counts, a constructed suppression chain
  IoU      all 512 random pairs with no corner-margin mask, symmetry, the far-offset pair at the bar fp32 inputs allow
  collect  lvq_center_collect on hand-made inputs
  module   num_conv = 1 (maps and lists against the restatement) and a configuration without SCORE_THRESH (kernel route = torch route)
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import center_head_cases as CC  # noqa: E402
import test_gpu_center_head as TH  # noqa: E402
from lidar_vision_vqa_amd import dense_head as DH  # noqa: E402
from lidar_vision_vqa_amd import ops  # noqa: E402

DEV = "cuda:0"
BAR = 1e-3


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)


def decode(maps, chans, classes, ids, k, stride, voxel, rng, limit, thresh):
    out = ops.center_decode(dev(maps), chans, classes, [c for row in ids for c in row], k=k, box_dim=7, stride=stride, voxel_xy=voxel,
                            range_xy=rng, limit_range=limit, score_thresh=thresh)
    return [o.cpu().numpy() for o in out]


def check_values(boxes, scores, d, origin):
    """Boxes and scores of the first len(d) rows at the 1e-5 relative bar of test_decode_against_the_restatement (x and y measured against
    max(|value|, |origin|), values below 1e-2 against 1e-2); a zero score must be exactly zero."""
    n = len(d["scores"])
    if n == 0:
        return
    assert (np.abs(scores[:n] - d["scores"]) <= 1e-5 * d["scores"]).all()
    scale = np.maximum(np.abs(d["boxes"]), 1e-2)
    scale[:, 0], scale[:, 1] = np.maximum(scale[:, 0], abs(origin[0])), np.maximum(scale[:, 1], abs(origin[1]))
    assert (np.abs(boxes[:n] - d["boxes"]) / scale).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.TIE_CASES))
def test_decode_ties_go_to_the_lower_flat_index(name):
    h, w, k, classes, thresh, _ = CC.TIE_CASES[name]
    maps, chans, ids, tasks = CC.tie_case(name)
    boxes, scores, labels, counts = decode(maps, chans, classes, ids, k, CC.TIE_STRIDE, CC.TIE_VOXEL, [0.0, 0.0], CC.WIDE_LIMIT, thresh)
    for ti, task in enumerate(tasks):
        for s, d in enumerate(CC.decode_ref(task, k, CC.TIE_STRIDE, CC.TIE_VOXEL, [0.0, 0.0], CC.WIDE_LIMIT, thresh, ids[ti])):
            n = len(d["scores"])
            above, eq, need, chunk = CC.select_stats(task["hm"][s], k)
            print(f"{name} task {ti} scene {s}: n = {task['hm'][s].size}, chunk {chunk}, {above} above, need {need} of {eq} equal; {n} rows")
            assert n == k and counts[s, ti] == n                              # wide limits and scores above the threshold: every winner survives
            assert np.array_equal(labels[s, ti, :n], d["labels"])
            assert np.array_equal(CC.tie_flat(boxes[s, ti, :n], labels[s, ti, :n], ids[ti], h, w), d["flat"])
            check_values(boxes[s, ti], scores[s, ti], d, [0.0, 0.0])
            assert (np.diff(scores[s, ti, :n]) <= 0).all()


@pytest.mark.parametrize("thresh", [None, CC.SCORE_THRESH])
def test_decode_nan_sorts_first(thresh):
    """Six NaN logits, three of each sign bit, take the first six of the K slots (torch.topk's order).  Without a score threshold they are
    the first six rows (compared as a set: the order among NaNs is open); with one they fail it and K - 6 finite candidates remain."""
    _, h, w, k, classes, _, stride, _ = CC.DECODE_CASES["small_k32"]
    maps, chans, ids, tasks = CC.nan_case()
    voxel, rng, limit = CC.decode_geometry("small_k32")
    boxes, scores, labels, counts = decode(maps, chans, classes, ids, k, stride, voxel, rng, limit, thresh)
    nn = len(CC.NAN_CELLS)
    for s, d in enumerate(CC.decode_ref(tasks[0], k, stride, voxel, rng, limit, thresh, ids[0])):
        n = len(d["scores"])
        lead = int(np.isnan(d["scores"]).sum())
        print(f"thresh {thresh} scene {s}: {n} rows, {lead} NaN rows in the restatement; kernel count {counts[s, 0]}, NaN rows {int(np.isnan(scores[s, 0]).sum())}")
        assert lead == (nn if thresh is None else 0) and np.isnan(d["scores"][:lead]).all()
        assert counts[s, 0] == n and np.array_equal(labels[s, 0, :n], d["labels"])
        assert np.isnan(scores[s, 0, :lead]).all() and not np.isnan(scores[s, 0, lead:]).any()
        check_values(boxes[s, 0, lead:], scores[s, 0, lead:], dict(boxes=d["boxes"][lead:], scores=d["scores"][lead:]), rng)
        if lead:                                                              # the NaN rows as a set: both sides sorted by x
            got, want = boxes[s, 0, :lead], d["boxes"][:lead]
            one = np.ones(lead, np.float32)
            check_values(got[np.argsort(got[:, 0])], one, dict(boxes=want[np.argsort(want[:, 0])], scores=one), rng)
        assert not boxes[s, 0, n:].any() and not scores[s, 0, n:].any()


def test_decode_without_a_score_threshold():
    name = CC.DECODE_NO_THRESH
    _, h, w, k, classes, vel, stride, _ = CC.DECODE_CASES[name]
    maps, chans, ids, tasks = CC.decode_case(name)
    voxel, rng, limit = CC.decode_geometry(name)
    assert not vel
    boxes, scores, labels, counts = decode(maps, chans, classes, ids, k, stride, voxel, rng, limit, None)
    for ti, task in enumerate(tasks):
        for s, d in enumerate(CC.decode_ref(task, k, stride, voxel, rng, limit, None, ids[ti])):
            n = len(d["scores"])
            assert counts[s, ti] == n and n > 0 and np.array_equal(labels[s, ti, :n], d["labels"])     # scene 1, too: nothing cuts its low scores
            check_values(boxes[s, ti], scores[s, ti], d, rng)
            assert (np.diff(scores[s, ti, :n]) < 0).all()


@pytest.mark.parametrize("name, k", [("k_sizes", k) for k in CC.K_SIZES] + [("k_is_n", 1024), ("stride1", 32)])
def test_decode_sizes_of_k_and_stride_one(name, k):
    """Distinct scores, checked like test_decode_against_the_restatement: K = 1, 2, 3 (the bitonic sort over 2, 2, 4), 1023 and 1024 of
    n = 2048, K = n = 1024, and stride = 1."""
    _, h, w, _, classes, _, stride, _ = CC.DECODE_EDGE_CASES[name]
    maps, chans, ids, tasks = CC.decode_case(name)
    voxel, rng, limit = CC.decode_geometry(name)
    boxes, scores, labels, counts = decode(maps, chans, classes, ids, k, stride, voxel, rng, limit, CC.SCORE_THRESH)
    assert boxes.shape == (2, 1, k, 7)
    for s, d in enumerate(CC.decode_ref(tasks[0], k, stride, voxel, rng, limit, CC.SCORE_THRESH, ids[0])):
        distinct, _, near_thresh, near_limit = CC.decode_margins(d, k, limit, CC.SCORE_THRESH)
        assert distinct >= 4 and near_thresh >= 1e-4 and near_limit >= 1e-2                # the margin conditions of this case
        n = len(d["scores"])
        print(f"{name} K = {k} scene {s}: {n} rows")
        assert counts[s, 0] == n and np.array_equal(labels[s, 0, :n], d["labels"])
        check_values(boxes[s, 0], scores[s, 0], d, rng)
        assert (np.diff(scores[s, 0, :n]) < 0).all()
        assert not boxes[s, 0, n:].any() and not scores[s, 0, n:].any()


def test_decode_keeps_centres_on_the_limit_range():
    maps, chans, ids, tasks, limit, rng, cells = CC.limit_case()
    k = 32
    boxes, scores, labels, counts = decode(maps, chans, [1], ids, k, CC.TIE_STRIDE, CC.TIE_VOXEL, rng, limit, CC.SCORE_THRESH)
    kept = sorted(c for c, keep in cells.items() if keep)
    for s, d in enumerate(CC.decode_ref(tasks[0], k, CC.TIE_STRIDE, CC.TIE_VOXEL, rng, limit, CC.SCORE_THRESH, ids[0])):
        n = len(d["scores"])
        assert n == len(kept) and counts[s, 0] == n
        got = [(int(round((y - rng[1]) * 2)), int(round((x - rng[0]) * 2))) for x, y in boxes[s, 0, :n, :2]]
        want = [(int(f) // 16, int(f) % 16) for f in d["flat"]]
        assert got == want and sorted(got) == kept
        assert np.array_equal(boxes[s, 0, :n, :3], d["boxes"][:, :3].astype(np.float32))              # exact arithmetic: the centres to the bit
        check_values(boxes[s, 0], scores[s, 0], d, rng)


# ---------------------------------------------------------------------------------------------------------------------------------
# NMS
# ---------------------------------------------------------------------------------------------------------------------------------
def nms(boxes, counts, thresh, pre_max, post_max):
    keep, n = ops.nms_bev(dev(boxes), dev(counts, np.int32), thresh=thresh, pre_max=pre_max, post_max=post_max)
    return keep.cpu().numpy(), n.cpu().numpy()


def check_nms(keep, n, boxes, counts, ious, thresh, margin, pre_max, post_max):
    assert keep.shape == (len(counts), post_max)
    for g, cnt in enumerate(counts):
        want, near = CC.greedy_nms(boxes[g, :cnt], thresh, pre_max, post_max, ious[g])
        assert near >= margin                                                 # the margin condition of this case
        assert n[g] == len(want) and keep[g, :n[g]].tolist() == want, (g, cnt)
        assert (keep[g, n[g]:] == -1).all()


@pytest.mark.parametrize("pre_max, post_max", [(1000, 83), (4096, 500), (1024, 1024)])
def test_nms_sixteen_mask_words(pre_max, post_max):
    thresh, _, _, margin, _ = CC.NMS_EDGE_CASES["wide"]
    boxes, counts, ious = CC.nms_edge_case("wide")
    keep, n = nms(boxes, counts, thresh, pre_max, post_max)
    check_nms(keep, n, boxes, counts, ious, thresh, margin, pre_max, post_max)
    print(f"pre {pre_max} post {post_max}: kept {n.tolist()} of {counts}")


@pytest.mark.parametrize("name", ["high", "low"])
def test_nms_at_the_other_thresholds(name):
    thresh, _, _, margin, _ = CC.NMS_EDGE_CASES[name]
    boxes, counts, ious = CC.nms_edge_case(name)
    keep, n = nms(boxes, counts, thresh, 4096, 500)
    check_nms(keep, n, boxes, counts, ious, thresh, margin, 4096, 500)
    print(f"{name} ({thresh}): kept {n.tolist()} of {counts}")
    # rows behind every count filled with NaN, then with 1e30: nothing changes
    for fill in (np.nan, 1e30):
        dirty = boxes.copy()
        for g, cnt in enumerate(counts):
            dirty[g, cnt:] = fill
        k2, n2 = nms(dirty, counts, thresh, 4096, 500)
        assert np.array_equal(k2, keep) and np.array_equal(n2, n), fill


def test_nms_clamps_the_counts():
    thresh, _, n_max, margin, _ = CC.NMS_EDGE_CASES["full"]
    boxes, _, ious = CC.nms_edge_case("full")
    keep, n = nms(boxes, [5000, -3, 130], thresh, 1000, 130)
    check_nms(keep, n, boxes, [130, 0, 130], ious, thresh, margin, 1000, 130)
    assert n[1] == 0 and n[0] > 0


def test_nms_suppression_chain_across_chunks():
    boxes, want = CC.nms_chain_case()
    keep, n = nms(boxes, [1024], CC.NMS_THRESH, 4096, 1024)
    assert n[0] == len(want) and keep[0, :n[0]].tolist() == want
    rows = CC.NMS_CHAIN_ROWS
    kept = set(keep[0, :n[0]].tolist())
    assert {rows["a"], rows["c"], rows["a2"], rows["c2"]} <= kept and not {rows["b"], rows["b2"]} & kept


# ---------------------------------------------------------------------------------------------------------------------------------
# IoU
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_ious():
    a, b, _ = CC.iou_random_pairs()
    return np.diag(ops.boxes_iou_bev(dev(a), dev(b)).cpu().numpy()), np.diag(ops.boxes_iou_bev(dev(b), dev(a)).cpu().numpy())


def test_iou_random_pairs_without_the_corner_mask():
    """The kernel claims that clipping is continuous in the corners, so the bar holds for every pair, not only for those whose corners stay
    0.05 m off the other box's edge lines.  Measured 2026-10-20 on the MI355X, 512 pairs (centres within 60 m, sizes 0.3 - 12 m): 1.51e-7 at
    pair 459; 7.2e-8 over the 62 pairs the masked test drops.  The claim of continuity in the kernel's header holds."""
    a, b, keep = CC.iou_random_pairs()
    want = CC.iou_pairs(a, b)
    err = np.abs(random_ious()[0] - want)
    i = int(err.argmax())
    print(f"all {len(a)} pairs: max |iou - fp64| = {err.max():.3e} at pair {i} (masked by the old test: {not keep[i]}), a = {a[i].tolist()}, b = {b[i].tolist()}")
    print(f"worst among the {int((~keep).sum())} pairs the masked test drops: {err[~keep].max():.3e}")
    assert err.max() <= BAR


def test_iou_is_symmetric():
    """Measured 2026-10-20, the same 512 pairs: 1.19e-7."""
    ab, ba = random_ious()
    err = np.abs(ab - ba)
    print(f"max |iou(a, b) - iou(b, a)| = {err.max():.3e}")
    assert err.max() <= BAR


def test_iou_far_from_the_origin():
    """The 2 x 2 half-overlap pair at (4000, -3000) against CC.IOU_FAR_BAR = 2e-4, derived there from the 2.44e-4 m ulp of an fp32 coordinate at
    that offset.  Measured 2026-10-20: 0.3333333 both ways (error below 3e-8): the rotated centre difference keeps the scene's offset out."""
    a, b, want = CC.IOU_CLOSED_FORM[CC.IOU_FAR_PAIR]
    got = [float(ops.boxes_iou_bev(dev([p]), dev([q]))[0, 0]) for p, q in ((a, b), (b, a))]
    print(f"half overlap at {CC.IOU_FAR_OFFSET}: kernel {got[0]:.7f} / {got[1]:.7f}, closed form {want:.7f}, bar {CC.IOU_FAR_BAR}")
    assert max(abs(g - want) for g in got) <= CC.IOU_FAR_BAR


def test_iou_thin_crossed_boxes():
    """Two boxes of 0.05 x 20 crossed at pi / 2 and pi / 6: IoU 1.25e-3 and 2.5e-3, at CC.IOU_THIN_BAR = 1e-5 absolute, both ways round."""
    for i in CC.IOU_THIN_PAIRS:
        a, b, want = CC.IOU_CLOSED_FORM[i]
        got = [float(ops.boxes_iou_bev(dev([p]), dev([q]))[0, 0]) for p, q in ((a, b), (b, a))]
        print(f"thin pair {i}: kernel {got[0]:.4e} / {got[1]:.4e}, closed form {want:.4e}")
        assert max(abs(g - want) for g in got) <= CC.IOU_THIN_BAR


# ---------------------------------------------------------------------------------------------------------------------------------
# collect
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box_dim", [9, 7])
@pytest.mark.parametrize("post_max", [1, 83])
@pytest.mark.parametrize("run", range(len(CC.COLLECT_KEEP_COUNTS)))
def test_collect_on_hand_made_inputs(box_dim, post_max, run):
    keep_count = CC.COLLECT_KEEP_COUNTS[run]
    boxes, scores, labels, keep, want = CC.collect_case(box_dim, post_max, keep_count)
    out_b, out_s, out_l, out_n = ops.center_collect(dev(boxes), dev(scores), dev(labels, np.int32), dev(keep, np.int32), dev(keep_count, np.int32))
    assert tuple(out_b.shape) == (2, 3 * post_max, box_dim) and out_l.dtype == torch.int64 and out_n.dtype == torch.int32
    for s, (wb, ws, wl) in enumerate(want):
        n = len(ws)
        assert int(out_n[s]) == n == sum(max(0, min(c, post_max)) for c in keep_count[s])
        assert np.array_equal(out_b[s, :n].cpu().numpy(), wb) and np.array_equal(out_s[s, :n].cpu().numpy(), ws)
        assert np.array_equal(out_l[s, :n].cpu().numpy(), wl)


# ---------------------------------------------------------------------------------------------------------------------------------
# module
# ---------------------------------------------------------------------------------------------------------------------------------
def variant_model(name):
    c = CC.MODULE_CASES[CC.MODULE_VARIANTS[name][0]]
    cfg, sd = CC.variant_ref(name)[:2]
    m = DH.CenterHead(cfg, c["input_channels"], len(c["class_names"]), c["class_names"], np.array(c["grid_size"]), c["point_cloud_range"],
                      c["voxel_size"], predict_boxes_when_training=False)
    m.load_state_dict({k: TH.t(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV).eval()


def as_lists(final):
    return [dict(boxes=f["pred_boxes"], scores=f["pred_scores"], labels=f["pred_labels"]) for f in final]


def test_module_with_one_conv_per_branch():
    cfg, _, x, maps64, pre, final, near = CC.variant_ref("num_conv1")
    kth_gap, near_thresh, near_iou, near_limit = CC.module_margins(cfg, pre, near)
    assert kth_gap >= 1e-3 and near_thresh >= 1e-3 and near_iou >= 0.02 and near_limit >= 1e-2
    out, pred = TH.run(variant_model("num_conv1"), x)
    err = TH.maps_err(pred, maps64)
    print(f"num_conv = 1, bf16x3 maps vs fp64 restatement: {err:.3e}")
    assert err <= BAR
    TH.check_lists(out["final_box_dicts"], as_lists(final))


def test_module_without_a_score_threshold(monkeypatch):
    cfg, _, x, _, pre, final, near = CC.variant_ref("no_score_thresh")
    kth_gap, _, near_iou, near_limit = CC.module_margins(cfg, pre, near)
    assert kth_gap >= 1e-3 and near_iou >= 0.02 and near_limit >= 1e-2
    m = variant_model("no_score_thresh")
    kernel = [{k: v.cpu() for k, v in d.items()} for d in TH.run(m, x)[0]["final_box_dicts"]]
    TH.check_lists(kernel, as_lists(final))
    monkeypatch.setenv("LVQ_HEAD_TORCH_POST", "1")
    torch_route = TH.run(m, x)[0]["final_box_dicts"]
    for s, (a, b) in enumerate(zip(kernel, torch_route)):
        assert torch.equal(a["pred_labels"], b["pred_labels"].cpu()), s                    # the order is exact
        assert float((a["pred_boxes"] - b["pred_boxes"].cpu()).abs().max()) <= BAR and float((a["pred_scores"] - b["pred_scores"].cpu()).abs().max()) <= BAR
        assert len(a["pred_scores"]) > 0
