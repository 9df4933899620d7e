"""CenterHead on the MI355X (lidar-vision-vqa_amd/dense_head.py on csrc/conv2d.hip and csrc/center_head.hip) against the fp64 restatements
of tests/center_head_cases.py and the goldens of the unmodified reference class (tests/golden/center_head_*.npz).

  IoU      closed-form pairs and 512 seeded random pairs at the project's parity bar, 1e-3 absolute (IoU <= 1, so max(1, .) = 1)
  NMS      seven groups in one call; keep lists identical to the fp64 greedy walk (no pair's IoU within 0.02 of the threshold)
  decode   order, labels and counts exact, boxes and scores within 1e-5 relative (exp, atan2, sigmoid), under the margin conditions
  module   bf16x3: maps within 1e-3 max(1, max|ref|) of the golden, final lists equal in count, order and labels, boxes and scores within the
           same bar; plain bf16: the maps only, as a regression guard at twice PLAIN_MEASURED; LVQ_HEAD_TORCH_POST=1 gives the same lists
  chain    BaseBEVBackbone -> CenterHead on one batch_dict; run-to-run and batch-composition bit-identity; the refusals
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bev_backbone_cases as BC  # noqa: E402
import center_head_cases as CC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import backbone2d as B2  # noqa: E402
from lidar_vision_vqa_amd import dense_head as DH  # noqa: E402
from lidar_vision_vqa_amd import ops  # noqa: E402

DEV = "cuda:0"
BAR = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# max |maps - restatement| / max(1, max|restatement|) over every branch of every task in the plain bf16 form, measured on the MI355X
PLAIN_MEASURED = {"nusc": 6.79e-3, "single": 5.36e-3, "waymo": 5.15e-3}    # (bf16x3 on the same cases: 1.35e-5, 1.16e-5, 9.81e-6)
# waymo: measured 2026-10-20 on [2, 64, 16, 24], K = 96, stride 1, BN_EPS 1e-3, no bias before the norm


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# IoU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_iou_closed_form_pairs():
    a = np.float32([p[0] for p in CC.IOU_CLOSED_FORM])
    b = np.float32([p[1] for p in CC.IOU_CLOSED_FORM])
    want = np.array([p[2] for p in CC.IOU_CLOSED_FORM])
    got = ops.boxes_iou_bev(dev(a), dev(b)).cpu().numpy()
    for i, (g, w) in enumerate(zip(np.diag(got), want)):
        print(f"pair {i}: kernel {g:.7f}  closed form {w:.7f}")
    assert np.abs(np.diag(got) - want).max() <= BAR
    assert np.abs(got - CC.iou_matrix(a, b)).max() <= BAR          # every row against every column, too


def test_iou_random_pairs():
    a, b, keep = CC.iou_random_pairs()
    assert (~keep).mean() <= 0.2
    want = CC.iou_pairs(a, b)
    got = np.diag(ops.boxes_iou_bev(dev(a), dev(b)).cpu().numpy())
    err = np.abs(got - want)[keep]
    print(f"{int(keep.sum())} of {len(a)} pairs kept, {(want[keep] > 0).mean():.2f} overlap; max |iou - fp64| = {err.max():.3e}")
    assert err.max() <= BAR and got.max() <= 1.0 + 1e-6 and got.min() >= 0.0


@pytest.mark.parametrize("n, m", [(1, 1), (63, 65), (65, 130), (130, 63), (1, 130)])
def test_iou_matrix_shapes(n, m):
    a, b, _ = CC.iou_random_pairs()
    rng = np.random.default_rng(n * 1000 + m)
    a, b = a[rng.permutation(len(a))[:n]].copy(), b[rng.permutation(len(b))[:m]].copy()
    b[:, :2] = a[rng.integers(n, size=m), :2] + rng.uniform(-3, 3, (m, 2)).astype(np.float32)       # most columns meet a row
    want = CC.iou_matrix(a, b)
    got = ops.boxes_iou_bev(dev(a), dev(b)).cpu().numpy()
    ok = CC.corner_edge_distance(np.repeat(a, m, 0), np.tile(b, (n, 1))).reshape(n, m) >= CC.IOU_EDGE_MARGIN
    assert got.shape == (n, m) and np.abs(got - want)[ok].max(initial=0.0) <= BAR and ok.mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# NMS
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nms_run(pre_max, post_max):
    boxes, counts, _ = CC.nms_case()
    keep, n = ops.nms_bev(dev(boxes), dev(counts, np.int32), thresh=CC.NMS_THRESH, pre_max=pre_max, post_max=post_max)
    return keep.cpu().numpy(), n.cpu().numpy()


@pytest.mark.parametrize("pre_max, post_max", [(1000, 1000), (1000, 40), (100, 83), (64, 1)])
def test_nms_keep_lists_equal_the_fp64_walk(pre_max, post_max):
    """post_max above (1000) and below (40, 1) the keep counts, pre_max below the counts of the two largest groups (100, 64)."""
    boxes, counts, ious = CC.nms_case()
    keep, n = nms_run(pre_max, post_max)
    assert keep.shape == (len(counts), post_max)
    for g, cnt in enumerate(counts):
        want, near = CC.greedy_nms(boxes[g, :cnt], CC.NMS_THRESH, pre_max, post_max, ious[g])
        assert near >= CC.NMS_MARGIN                                         # the margin condition of this case
        assert n[g] == len(want) and keep[g, :n[g]].tolist() == want, (g, cnt)
        assert (keep[g, n[g]:] == -1).all()
    full = [len(CC.greedy_nms(boxes[g, :c], CC.NMS_THRESH, 10 ** 6, 10 ** 6, ious[g])[0]) for g, c in enumerate(counts)]
    print(f"pre {pre_max} post {post_max}: kept {n.tolist()} (untruncated walk: {full})")


def test_nms_strided_rows_and_argument_errors():
    boxes, counts, ious = CC.nms_case()
    wide = np.zeros((len(counts), CC.NMS_N_MAX, 9), np.float32)
    wide[:, :, :7], wide[:, :, 7:] = boxes, 99.0
    keep, n = ops.nms_bev(dev(wide), dev(counts, np.int32), thresh=CC.NMS_THRESH, pre_max=1000, post_max=1000)
    k0, n0 = nms_run(1000, 1000)
    assert np.array_equal(keep.cpu().numpy(), k0) and np.array_equal(n.cpu().numpy(), n0)
    with pytest.raises(F.LvqError):
        ops.nms_bev(torch.zeros((1, 1025, 7), device=DEV), torch.ones(1, dtype=torch.int32, device=DEV), thresh=0.2, pre_max=10, post_max=10)


# ---------------------------------------------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.DECODE_CASES))
def test_decode_against_the_restatement(name):
    b, h, w, k, classes, vel, stride, _ = CC.DECODE_CASES[name]
    maps, chans, ids, tasks = CC.decode_case(name)
    voxel, rng, limit = CC.decode_geometry(name)
    boxes, scores, labels, counts = ops.center_decode(dev(maps), chans, classes, [c for row in ids for c in row], k=k, box_dim=9 if vel else 7,
                                                      stride=stride, voxel_xy=voxel, range_xy=rng, limit_range=limit, score_thresh=CC.SCORE_THRESH)
    boxes, scores, labels, counts = boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy()
    assert boxes.shape == (b, len(classes), k, 9 if vel else 7)
    seen = []
    for ti, task in enumerate(tasks):
        for s, d in enumerate(CC.decode_ref(task, k, stride, voxel, rng, limit, CC.SCORE_THRESH, ids[ti])):
            distinct, _, near_thresh, near_limit = CC.decode_margins(d, k, limit, CC.SCORE_THRESH)
            assert distinct >= 4 and near_thresh >= 1e-4 and near_limit >= 1e-2            # the margin conditions of this case
            n = len(d["scores"])
            seen.append(n)
            assert counts[s, ti] == n
            assert np.array_equal(labels[s, ti, :n], d["labels"])
            if n:
                rel_s = np.abs(scores[s, ti, :n] - d["scores"]) / d["scores"]
                # relative to the value; x and y are sums with the range's origin ((col + c) * cell + range), which fp32 carries to an
                # ulp of the LARGER operand however the sum is written (the reference's own fp32 line included), so their scale is
                # max(|value|, |origin|); values below 1e-2 (a heading or velocity near zero) are measured against 1e-2
                scale = np.maximum(np.abs(d["boxes"]), 1e-2)
                scale[:, 0], scale[:, 1] = np.maximum(scale[:, 0], abs(rng[0])), np.maximum(scale[:, 1], abs(rng[1]))
                rel_b = np.abs(boxes[s, ti, :n] - d["boxes"]) / scale
                print(f"{name} task {ti} scene {s}: {n} of {k}; scores {rel_s.max():.2e}, boxes {rel_b.max():.2e}")
                assert rel_s.max() <= 1e-5 and rel_b.max() <= 1e-5
                # the order is the restatement's: scores descending, and the xy of a row identifies its cell
                assert (np.diff(scores[s, ti, :n]) < 0).all()
            assert not boxes[s, ti, n:].any() and not scores[s, ti, n:].any()             # rows behind the count are zeros
    assert 0 in seen and any(0 < n < k for n in seen)            # a scene where every candidate fails, one where only some do


def test_decode_equal_scores_go_to_the_lower_index():
    """A constant heat map: every score is equal, so the K winners are flat indices 0 .. K - 1 in that order (the documented rule)."""
    h, w, k = 7, 9, 20
    maps = np.zeros((1, 10, h, w), np.float32)
    maps[:, 8:] = 1.0                                                          # two classes, all sigmoid(1)
    args = dict(k=k, box_dim=7, stride=4, voxel_xy=[0.1, 0.1], range_xy=[0.0, 0.0], limit_range=[-100, -100, -100, 100, 100, 100], score_thresh=0.1)
    boxes, scores, labels, counts = ops.center_decode(dev(maps), [[0, 2, 3, 6, -1, 8]], [2], [0, 1], **args)
    assert int(counts[0, 0]) == k and (labels[0, 0] == 0).all()
    xy = boxes[0, 0, :, :2].cpu().numpy() / 0.4
    assert np.array_equal(np.rint(xy[:, 1] * w + xy[:, 0]).astype(int), np.arange(k))
    with pytest.raises(F.LvqError):
        ops.center_decode(dev(maps), [[0, 2, 3, 6, -1, 8]], [2], [0, 1], **dict(args, k=2 * h * w + 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# module
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(name):
    c = CC.MODULE_CASES[name]
    m = DH.dense_heads_all["CenterHead"](CC.case_cfg(name), c["input_channels"], len(c["class_names"]), c["class_names"], np.array(c["grid_size"]),
                                         c["point_cloud_range"], c["voxel_size"], predict_boxes_when_training=False)
    m.load_state_dict({k: t(v) for k, v in CC.case_state(name).items()}, strict=True)
    return m.to(DEV).eval()


def run(m, x, mode="bf16x3"):
    m.precision = mode
    with torch.no_grad():
        out = m(dict(spatial_features_2d=t(x).to(DEV), batch_size=x.shape[0]))
    return out, m.forward_ret_dict["pred_dicts"]


def maps_err(pred, ref):
    return max(float(np.abs(pred[i][n].cpu().numpy() - ref[i][n]).max()) / max(1.0, float(np.abs(ref[i][n]).max())) for i in range(len(ref)) for n in ref[i])


def golden(name):
    z = np.load(os.path.join(GOLDEN, CC.golden_name(name)))
    cfg = CC.case_cfg(name)
    maps = [{n: z[f"maps_{i}_{n}"] for n in CC.branch_names(cfg)} for i in range(len(cfg.CLASS_NAMES_EACH_HEAD))]
    final = [{k: z[f"final_{s}_{k}"] for k in ("boxes", "scores", "labels")} for s in range(CC.MODULE_CASES[name]["shape"][0])]
    return maps, final


def check_lists(got, want):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        gb, gs, gl = g["pred_boxes"].cpu().numpy(), g["pred_scores"].cpu().numpy(), g["pred_labels"].cpu().numpy()
        assert gl.dtype == np.int64 and gb.shape == w["boxes"].shape and np.array_equal(gl, w["labels"]), s
        err = max(float(np.abs(gb - w["boxes"]).max()) / max(1.0, float(np.abs(w["boxes"]).max())), float(np.abs(gs - w["scores"]).max()))
        print(f"scene {s}: {len(gl)} boxes, max error {err:.3e}")
        assert err <= BAR


@pytest.mark.parametrize("name", list(CC.MODULE_CASES))
def test_module_bf16x3_reproduces_the_reference_class(name):
    maps, final = golden(name)
    out, pred = run(model(name), CC.case_input(name))
    err = maps_err(pred, maps)
    print(f"{name} bf16x3 maps: vs golden {err:.3e}, vs fp64 restatement {maps_err(pred, CC.case_ref(name)[0]):.3e}")
    assert err <= BAR
    check_lists(out["final_box_dicts"], final)
    assert "rois" not in out


@pytest.mark.parametrize("name", list(CC.MODULE_CASES))
def test_module_plain_bf16_regression_guard(name):
    """The plain bf16 form has no bar known in advance: PLAIN_MEASURED holds the error measured on the MI355X and the test asserts twice
    that value (tests/test_gpu_backbone2d.py does the same).  Only the maps are checked: the lists of a plain-bf16 run may differ."""
    err = maps_err(run(model(name), CC.case_input(name), "bf16")[1], CC.case_ref(name)[0])
    print(f"{name} bf16 maps: vs fp64 restatement {err:.3e}")
    assert PLAIN_MEASURED[name] is not None and err <= 2 * PLAIN_MEASURED[name], err


@pytest.mark.parametrize("name", list(CC.MODULE_CASES))
def test_torch_post_route_gives_the_same_lists(name, monkeypatch):
    _, final = golden(name)
    monkeypatch.setenv("LVQ_HEAD_TORCH_POST", "1")
    check_lists(run(model(name), CC.case_input(name))[0]["final_box_dicts"], final)


def test_rois_for_refining():
    name = "single"
    c = CC.MODULE_CASES[name]
    m = DH.CenterHead(CC.case_cfg(name), c["input_channels"], 3, c["class_names"], np.array(c["grid_size"]), c["point_cloud_range"], c["voxel_size"])
    m.load_state_dict(model(name).state_dict(), strict=True)
    out, _ = run(m.to(DEV).eval(), CC.case_input(name))
    lists = out["final_box_dicts"]
    n = max(len(d["pred_scores"]) for d in lists)
    assert out["has_class_labels"] is True and tuple(out["rois"].shape) == (2, n, 7) and out["roi_labels"].dtype == torch.int64
    for s, d in enumerate(lists):
        k = len(d["pred_scores"])
        assert torch.equal(out["rois"][s, :k], d["pred_boxes"]) and torch.equal(out["roi_scores"][s, :k], d["pred_scores"])
        assert torch.equal(out["roi_labels"][s, :k], d["pred_labels"]) and not out["rois"][s, k:].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# chain, determinism, refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def chain_models():
    cfg, cin, _, _, _ = BC.CASES["nusc_second"]
    bb = B2.BaseBEVBackbone(BC.Cfg(cfg), cin)
    bb.load_state_dict({k: t(v) for k, v in BC.case_state("nusc_second").items()}, strict=True)
    hcfg = CC.head_cfg(CC.NUSC_HEADS, True, 8, 32)
    head = DH.CenterHead(hcfg, 512, 10, CC.NUSC_CLASSES, np.array([128, 128, 40]), [-6.4, -6.4, -5.0, 6.4, 6.4, 3.0], [0.1, 0.1, 0.2], False)
    sd = CC.state(hcfg, 512, 73, 2.5, -2.0)
    head.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    return bb.to(DEV).eval(), head.to(DEV).eval(), hcfg, sd


def test_backbone_to_head_on_one_batch_dict_and_determinism():
    bb, head, hcfg, sd = chain_models()
    x1 = BC.case_input("nusc_second")
    x3 = np.concatenate([x1, np.roll(x1, 3, axis=3), x1[:, ::-1].copy()], axis=0)

    def forward(x):
        with torch.no_grad():
            d = head(bb(dict(spatial_features=t(x).to(DEV), batch_size=x.shape[0])))
        return d, [{k: v.clone() for k, v in p.items()} for p in head.forward_ret_dict["pred_dicts"]]

    d3, p3 = forward(x3)
    assert tuple(d3["spatial_features_2d"].shape) == (3, 512, 16, 16) and len(d3["final_box_dicts"]) == 3
    assert all(len(f["pred_scores"]) > 0 for f in d3["final_box_dicts"])
    ref = CC.head_maps(hcfg, sd, d3["spatial_features_2d"].cpu().numpy())
    err = maps_err(p3, ref)
    print(f"chain: head maps on the backbone's output vs fp64 restatement {err:.3e}")
    assert err <= BAR
    d3b, p3b = forward(x3)
    d1, p1 = forward(x1)
    for a, b in zip(p3, p3b):
        assert all(torch.equal(a[k], b[k]) for k in a)                        # two runs are bit-identical
    for a, b in zip(p3, p1):
        assert all(torch.equal(a[k][:1], b[k]) for k in a)                    # scene 0 alone = scene 0 inside B = 3
    for key in ("pred_boxes", "pred_scores", "pred_labels"):
        assert torch.equal(d3["final_box_dicts"][0][key], d1["final_box_dicts"][0][key])
        assert all(torch.equal(d3["final_box_dicts"][s][key], d3b["final_box_dicts"][s][key]) for s in range(3))


def test_unsupported_branches_raise():
    name = "single"
    c = CC.MODULE_CASES[name]
    x = t(CC.case_input(name)).to(DEV)

    def build(cfg, **kw):
        return DH.CenterHead(cfg, 64, 3, c["class_names"], np.array(c["grid_size"]), c["point_cloud_range"], c["voxel_size"], False, **kw).to(DEV)

    def call(m):
        with torch.no_grad():
            return m(dict(spatial_features_2d=x, batch_size=2))

    m = build(CC.case_cfg(name))
    with pytest.raises(F.LvqError, match="eval"):
        call(m)                                                                 # train() mode
    m.eval()
    with pytest.raises(F.LvqError, match="eval"):
        m(dict(spatial_features_2d=x, batch_size=2))                            # gradients in reach
    for method in (m.assign_targets, m.get_loss):
        with pytest.raises(F.LvqError, match="out of scope"):
            method()
    m.precision = "fp8"
    with pytest.raises(F.LvqError):
        call(m)
    for nms_type in ("nms_normal_gpu", "class_specific_nms", "circle_nms"):
        with pytest.raises(F.LvqError, match=nms_type):
            call(build(CC.case_cfg(name, nms_type=nms_type)).eval())
    cfg = CC.case_cfg(name)
    cfg.POST_PROCESSING["USE_IOU_TO_RECTIFY_SCORE"] = True
    with pytest.raises(F.LvqError, match="USE_IOU_TO_RECTIFY_SCORE"):
        call(build(cfg).eval())
    cfg = CC.case_cfg(name)
    cfg.SEPARATE_HEAD_CFG.HEAD_DICT["iou"] = CC.Cfg(out_channels=1, num_conv=2)
    with pytest.raises(F.LvqError, match="iou"):
        call(build(cfg).eval())
    cfg = CC.case_cfg(name)
    cfg["SHARED_CONV_CHANNEL"] = 128
    with pytest.raises(F.LvqError, match="SHARED_CONV_CHANNEL"):
        call(build(cfg).eval())
    cfg = CC.case_cfg(name)
    cfg["NUM_HM_CONV"] = 1
    with pytest.raises(F.LvqError, match="num_conv"):
        call(build(cfg).eval())
    one = build(CC.case_cfg(name, num_conv=1)).eval()                          # num_conv = 1 everywhere is supported
    assert len(call(one)["final_box_dicts"]) == 2
    with pytest.raises(F.LvqError):
        one.cpu()(dict(spatial_features_2d=x.cpu(), batch_size=2))              # no CPU fallback
