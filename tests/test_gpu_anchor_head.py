"""AnchorHeadSingle on the MI355X (lidar-vision-vqa_amd/anchor_head.py on csrc/conv2d.hip and csrc/anchor_head.hip) against the fp64
restatements of tests/anchor_head_cases.py and the goldens of the unmodified reference classes (tests/golden/anchor_head_*.npz).

  decode   boxes and scores within 1e-5 max(1, |ref|) (the CenterHead decode bar), labels exact; the heading over ALL anchors but those
           within 1e-4 of a period boundary (at most 1 %); a NaN logit; the candidate set, with the threshold fed back from a score
  select   explicit score arrays: order, indices, rows and counts bit-exact against select_ref; ties, NaNs, the candidate-list route
  NMS      seven groups of up to 4096 rows in one call: keep lists identical to the fp64 greedy walk; equal to lvq_nms_bev up to 1024 rows
  module   bf16x3: dense outputs within 1e-3 max(1, max|ref|) of the golden, final lists matched one to one; plain bf16: the dense outputs
           only, at twice PLAIN_MEASURED; LVQ_HEAD_TORCH_POST=1 and the candidate-list route give the same lists; OUTPUT_RAW_SCORE;
           run-to-run and batch-composition bit-identity; the refusals
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import anchor_head_cases as AC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import anchor_head as AH  # noqa: E402
from lidar_vision_vqa_amd import ops  # noqa: E402

DEV = "cuda:0"
BAR, DECODE_BAR = 1e-3, 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = list(AC.MODULE_CASES)
# max |dense output - restatement| / max(1, max|restatement|) over batch_cls_preds and batch_box_preds in the plain bf16 form (the heading's
# error modulo the period: bf16 logits turn near-ties of the direction bins, which moves a heading by a whole period and says nothing about
# the convs), measured on the MI355X on 2026-10-21 at [2, 64, 16, 24] (2304 / 2304 / 768 anchors per scene)
PLAIN_MEASURED = {"kitti": 1.307e-3, "wide": 8.862e-4, "nodir": 1.662e-3}    # (bf16x3 on the same cases: 2.4e-6, 1.8e-6, 5.4e-6)


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------------------------------------------
def run_decode(shape, maps=None, thresh=None):
    b, h, w, a, n_cls, use_dir = shape
    m, anchors, (c0, c1, c2) = AC.decode_case(*shape)
    return ops.anchor_decode(dev(m if maps is None else maps), dev(anchors), n_anchors=a, n_cls=n_cls, cls_channel=c0, box_channel=c1,
                             dir_channel=c2, n_dir_bins=AC.NUM_DIR_BINS if use_dir else 0, dir_offset=AC.DIR_OFFSET,
                             dir_limit_offset=AC.DIR_LIMIT_OFFSET, score_thresh=thresh)


@pytest.mark.parametrize("shape", AC.DECODE_SHAPES)
def test_decode_against_the_restatement(shape):
    ref = AC.decode_case_ref(*shape)
    cls, box, scores, labels, cand, count = [None if v is None else v.cpu().numpy() for v in run_decode(shape)]
    assert cand is None and count is None
    assert np.array_equal(cls, ref["cls"].astype(np.float32))                   # the logits are copied, not computed
    assert np.array_equal(labels, ref["labels"])
    err_s = np.abs(scores - ref["scores"].astype(np.float64)) / np.maximum(1.0, np.abs(ref["scores"]))
    near = ~AC.heading_clear(ref["frac"]) if ref["frac"] is not None else np.zeros(scores.shape, bool)
    err_b = np.abs(box - ref["boxes"]) / np.maximum(1.0, np.abs(ref["boxes"]))
    err_b[..., 6][near] = 0.0
    print(f"{shape}: score err {err_s.max():.2e}, box err {err_b.max():.2e}, {int(near.sum())} of {near.size} headings left out")
    assert near.mean() <= 0.01 and err_s.max() <= DECODE_BAR and err_b.max() <= DECODE_BAR
    if ref["bins"] is not None:                                                  # the bin, from the heading itself: r lies in bin's period
        period = np.float64(np.float32(2 * np.pi / AC.NUM_DIR_BINS))
        got_bin = np.floor((box[..., 6].astype(np.float64) - np.float64(np.float32(AC.DIR_OFFSET))) / period + 1e-6)
        assert np.array_equal(got_bin[~near], ref["bins"][~near])


def test_decode_candidate_set_and_a_nan_logit():
    shape = (2, 5, 7, 6, 3, True)
    maps = AC.decode_case(*shape)[0].copy()
    a, n_cls = shape[3], shape[4]
    maps[1, 2 * n_cls + 1, 3, 4] = np.nan                                        # anchor 2 of pixel (3, 4) of scene 1, class 1
    nan_at = (3 * 7 + 4) * a + 2
    _, _, scores, labels, _, _ = run_decode(shape, maps)
    scores = scores.cpu().numpy()
    assert np.isnan(scores[1, nan_at]) and int(np.isnan(scores).sum()) == 1 and int(labels[1, nan_at]) == 1
    thresh = float(np.sort(scores[0])[scores.shape[1] // 2])                      # fed back from a computed score: one anchor sits ON it
    _, _, again, _, cand, count = run_decode(shape, maps, thresh)
    assert np.array_equal(bits(again.cpu().numpy()), bits(scores))
    cand, count = cand.cpu().numpy(), count.cpu().numpy()
    for s in range(2):
        with np.errstate(invalid="ignore"):
            want = np.nonzero(scores[s] >= np.float32(thresh))[0]
        got = cand[s, :count[s]]
        assert count[s] == len(want) and np.array_equal(np.sort(got), want)
        assert nan_at not in got or s == 0
    assert (scores[0] == np.float32(thresh)).any() and 0 < count[0] < scores.shape[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------------------------------------------------------------
def select_want(scores, labels, boxes, pre_max, thresh):
    b = scores.shape[0]
    out = dict(boxes=np.zeros((b, pre_max, 7), np.float32), scores=np.zeros((b, pre_max), np.float32), labels=np.zeros((b, pre_max), np.int32),
               index=np.full((b, pre_max), -1, np.int32), count=np.zeros(b, np.int32))
    for s in range(b):
        idx = AC.select_ref(scores[s], thresh, pre_max)
        k = len(idx)
        out["boxes"][s, :k], out["scores"][s, :k], out["labels"][s, :k], out["index"][s, :k], out["count"][s] = \
            boxes[s, idx], scores[s, idx], labels[s, idx], idx, k
    return out


def check_select(got, want):
    sel_boxes, sel_scores, sel_labels, sel_index, sel_count = [v.cpu().numpy() for v in got]
    assert np.array_equal(sel_count, want["count"])
    assert np.array_equal(sel_index, want["index"])
    assert np.array_equal(bits(sel_scores), bits(want["scores"])) and np.array_equal(sel_labels, want["labels"])
    assert np.array_equal(bits(sel_boxes), bits(want["boxes"]))


@pytest.mark.parametrize("name", list(AC.SELECT_CASES))
def test_select_against_the_restatement(name):
    scores, labels, boxes, pre_max, thresh = AC.select_case(name)
    want = select_want(scores, labels, boxes, pre_max, thresh)
    d_scores, d_labels, d_boxes = dev(scores), dev(labels, np.int32), dev(boxes)
    check_select(ops.anchor_select(d_scores, d_labels, d_boxes, score_thresh=thresh, pre_max=pre_max), want)
    if thresh is not None:                                                        # the candidate-list route: the same set, shuffled
        rng = np.random.default_rng(5)
        cand = np.zeros(scores.shape, np.int32)
        count = np.zeros(scores.shape[0], np.int32)
        for s in range(scores.shape[0]):
            with np.errstate(invalid="ignore"):
                idx = rng.permutation(np.nonzero(scores[s] >= np.float32(thresh))[0])
            cand[s, :len(idx)], count[s] = idx, len(idx)
        check_select(ops.anchor_select(d_scores, d_labels, d_boxes, score_thresh=thresh, pre_max=pre_max, cand=dev(cand, np.int32),
                                       cand_count=dev(count, np.int32)), want)


def test_select_refuses_more_than_4096_rows():
    scores, labels, boxes, _, thresh = AC.select_case("n65")
    with pytest.raises(F.LvqError, match="lvq_anchor_select"):
        ops.anchor_select(dev(scores), dev(labels, np.int32), dev(boxes), score_thresh=thresh, pre_max=4097)


# ---------------------------------------------------------------------------------------------------------------------------------
# the wide NMS
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nms_inputs():
    boxes, counts, ious = AC.nms_wide_case()
    return boxes, counts, ious, dev(boxes), dev(counts, np.int32)


def check_keep(keep, keep_count, boxes, counts, ious, pre_max, post_max):
    keep, keep_count = keep.cpu().numpy(), keep_count.cpu().numpy()
    for g, n in enumerate(counts):
        want, _ = AC.greedy_nms(boxes[g, :n], AC.NMS_WIDE_THRESH, pre_max, post_max, iou=ious[g])
        assert keep_count[g] == len(want), (g, n)
        assert np.array_equal(keep[g, :len(want)], want) and (keep[g, len(want):] == -1).all(), (g, n)


@pytest.mark.parametrize("pre_max, post_max", [(4096, 4096), (1000, 4096), (4096, 100), (4096, 1), (1090, 37)])
def test_wide_nms_against_the_greedy_walk(pre_max, post_max):
    boxes, counts, ious, d_boxes, d_counts = nms_inputs()
    keep, keep_count = ops.nms_bev_wide(d_boxes, d_counts, thresh=AC.NMS_WIDE_THRESH, pre_max=pre_max, post_max=post_max)
    check_keep(keep, keep_count, boxes, counts, ious, pre_max, post_max)
    if (pre_max, post_max) == (4096, 4096):
        kept = set(keep[-1, :int(keep_count[-1])].cpu().tolist())
        assert 0 in kept and not kept & set(AC.NMS_WIDE_DUPLICATES)               # a suppressor in word 0 reaches word 63


def test_wide_nms_with_a_box_stride_of_nine_and_against_the_narrow_kernel():
    boxes, counts, ious, d_boxes, d_counts = nms_inputs()
    nine = torch.full((*d_boxes.shape[:2], 9), 7.0, device=DEV)
    nine[..., :7] = d_boxes
    keep9, count9 = ops.nms_bev_wide(nine, d_counts, thresh=AC.NMS_WIDE_THRESH, pre_max=4096, post_max=500)
    check_keep(keep9, count9, boxes, counts, ious, 4096, 500)
    small = [g for g, n in enumerate(counts) if n <= 1024]
    assert len(small) >= 4
    sub, sub_counts = d_boxes[small, :1024].contiguous(), d_counts[small].contiguous()
    wide = ops.nms_bev_wide(sub, sub_counts, thresh=AC.NMS_WIDE_THRESH, pre_max=1024, post_max=500)
    narrow = ops.nms_bev(sub, sub_counts, thresh=AC.NMS_WIDE_THRESH, pre_max=1024, post_max=500)
    assert torch.equal(wide[0], narrow[0]) and torch.equal(wide[1], narrow[1])
    assert torch.equal(wide[0], keep9[small]) and torch.equal(wide[1], count9[small])


def test_wide_nms_refuses_4097_rows():
    with pytest.raises(F.LvqError, match="lvq_nms_bev_wide"):
        ops.nms_bev_wide(torch.zeros((1, 4097, 7), device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV), thresh=0.2, pre_max=4096,
                         post_max=10)


# ---------------------------------------------------------------------------------------------------------------------------------
# module
# ---------------------------------------------------------------------------------------------------------------------------------
def golden(name):
    return np.load(os.path.join(GOLDEN, AC.golden_name(name)))


@functools.lru_cache(maxsize=None)
def head(name):
    c = AC.MODULE_CASES[name]
    m = AH.AnchorHeadSingle(AC.case_cfg(name), c["shape"][1], len(c["class_names"]), c["class_names"], np.array(c["grid_size"]),
                            c["point_cloud_range"])
    sd = AC.case_state(name)
    m.load_state_dict({k: torch.from_numpy(sd[k]) for k in m.state_dict()}, strict=True)
    return m.to(DEV).eval()


def forward(name, precision=None, x=None, thresh=None):
    m = head(name)
    m.precision, m.candidate_score_thresh = precision, thresh
    x = AC.case_input(name) if x is None else x
    with torch.no_grad():
        out = m(dict(spatial_features_2d=dev(x), batch_size=x.shape[0]))
    m.precision, m.candidate_score_thresh = None, None
    return out


def post(name, out, **kw):
    return AH.post_processing(out, AC.case_post(name, **kw), len(AC.MODULE_CASES[name]["class_names"]))[0]


def dense_error(name, out, ref_cls, ref_box, wrap=False):
    """max |dense - ref| / max(1, max|ref|) of the logits and of the boxes, the headings within 1e-4 of a period boundary left out.
    wrap: the heading's error is taken modulo the direction classifier's period instead (the distance to the nearest multiple), so that
    it measures the heading residual whichever way a near-tie of the bins or of the floor went."""
    _, dec, _ = AC.case_ref(name)
    near = ~AC.heading_clear(dec["frac"]) if dec["frac"] is not None else np.zeros(ref_box.shape[:2], bool)
    assert near.mean() <= 0.01
    e_cls = np.abs(out["batch_cls_preds"].cpu().numpy() - ref_cls).max() / max(1.0, np.abs(ref_cls).max())
    err = np.abs(out["batch_box_preds"].cpu().numpy() - ref_box)
    if wrap and dec["frac"] is not None:
        period = 2 * np.pi / AC.NUM_DIR_BINS
        err[..., 6] = np.abs(err[..., 6] - period * np.rint(err[..., 6] / period))
    else:
        err[..., 6][near] = 0.0
    return e_cls, err.max() / max(1.0, np.abs(ref_box).max())


@pytest.mark.parametrize("name", CASES)
def test_module_dense_outputs_bf16x3(name):
    g, out = golden(name), forward(name)
    assert out["cls_preds_normalized"] is False and out["batch_cls_preds"].dtype == torch.float32
    assert tuple(out["batch_cls_preds"].shape) == g["batch_cls_preds"].shape and tuple(out["batch_box_preds"].shape) == g["batch_box_preds"].shape
    e_cls, e_box = dense_error(name, out, g["batch_cls_preds"], g["batch_box_preds"])
    print(f"{name}: bf16x3 dense error cls {e_cls:.2e} box {e_box:.2e}")
    assert e_cls <= BAR and e_box <= BAR
    ret, c = head(name).forward_ret_dict, AC.MODULE_CASES[name]
    b, _, h, w = c["shape"]
    a, n_cls = AC.n_anchors(name), len(c["class_names"])
    assert tuple(ret["cls_preds"].shape) == (b, h, w, a * n_cls) and tuple(ret["box_preds"].shape) == (b, h, w, a * 7)
    assert torch.equal(ret["cls_preds"].reshape(b, -1, n_cls), out["batch_cls_preds"])
    assert ("dir_cls_preds" in ret) == c["use_dir"] and tuple(ret["anchor_scores"].shape) == (b, h * w * a)
    sc = torch.sigmoid(out["batch_cls_preds"]).max(-1)
    assert (ret["anchor_scores"] - sc[0]).abs().max() <= 1e-6 and torch.equal(ret["anchor_labels"].long(), sc[1])


def match_lists(got, g, s, bar_box):
    """One scene's kernel list against the golden's: equal counts, non-increasing scores, a one-to-one match of rows with equal label and
    boxes / scores within the bar; a row sits at another position than its golden row only among golden scores within 1e-4."""
    gb, gs, gl = g[f"final_{s}_boxes"], g[f"final_{s}_scores"], g[f"final_{s}_labels"]
    kb, ks, kl = got["pred_boxes"].cpu().numpy(), got["pred_scores"].cpu().numpy(), got["pred_labels"].cpu().numpy()
    assert len(ks) == len(gs) and kl.dtype == np.int64
    assert np.all(np.diff(ks) <= 0)
    dist = np.abs(kb[:, None, :2] - gb[None, :, :2]).max(-1) + np.where(kl[:, None] == gl[None, :], 0.0, np.inf)
    partner = dist.argmin(1) if len(gs) else np.zeros(0, np.int64)
    assert len(set(partner.tolist())) == len(gs)
    assert np.array_equal(kl, gl[partner])
    assert np.abs(kb - gb[partner]).max(initial=0.0) <= bar_box and np.abs(ks - gs[partner]).max(initial=0.0) <= BAR
    moved = partner != np.arange(len(gs))
    assert np.abs(gs[partner][moved] - gs[moved]).max(initial=0.0) <= 1e-4
    return int(moved.sum())


@pytest.mark.parametrize("name", CASES)
def test_module_final_lists_bf16x3(name):
    g, out = golden(name), forward(name)
    bar_box = BAR * max(1.0, np.abs(g["batch_box_preds"]).max())
    for s, d in enumerate(post(name, out)):
        moved = match_lists(d, g, s, bar_box)
        print(f"{name} scene {s}: {len(d['pred_scores'])} rows, {moved} at another position than in the golden")


@pytest.mark.parametrize("name", CASES)
def test_module_plain_bf16_stays_where_it_was_measured(name):
    maps64, dec, _ = AC.case_ref(name)
    out = forward(name, "bf16")
    e_cls, e_box = dense_error(name, out, dec["cls"], dec["boxes"], wrap=True)
    print(f"{name}: plain bf16 dense error cls {e_cls:.3e} box {e_box:.3e} (measured {PLAIN_MEASURED[name]})")
    assert max(e_cls, e_box) <= 2 * PLAIN_MEASURED[name]
    x3 = forward(name)
    assert max(dense_error(name, x3, dec["cls"], dec["boxes"], wrap=True)) < max(e_cls, e_box)    # and bf16x3 is the more exact of the two


def same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(x[k], y[k]), k


@pytest.mark.parametrize("name", CASES)
def test_torch_route_and_candidate_route_give_the_same_lists(name, monkeypatch):
    out = forward(name)
    kernel = post(name, out)
    listed = forward(name, thresh=AC.MODULE_CASES[name]["post"]["score_thresh"])
    assert (listed["anchor_candidates"] is None) == (AC.MODULE_CASES[name]["post"]["score_thresh"] is None)
    same_lists(kernel, post(name, listed))
    foreign = dict(batch_cls_preds=out["batch_cls_preds"].clone(), batch_box_preds=out["batch_box_preds"].clone(), batch_size=2,
                   cls_preds_normalized=False)                                    # batch_cls_preds from elsewhere: scores by torch ops
    same_lists(kernel, post(name, foreign))
    monkeypatch.setenv("LVQ_HEAD_TORCH_POST", "1")
    same_lists(kernel, post(name, out))


@pytest.mark.parametrize("name", ["kitti", "nodir"])
def test_output_raw_score(name, monkeypatch):
    out = forward(name)
    plain, raw = post(name, out), post(name, out, raw=True)
    for s, (p, r) in enumerate(zip(plain, raw)):
        assert torch.equal(p["pred_boxes"], r["pred_boxes"]) and torch.equal(p["pred_labels"], r["pred_labels"])
        assert (torch.sigmoid(r["pred_scores"]) - p["pred_scores"]).abs().max() <= 1e-6
        rows = (out["batch_box_preds"][s][None] == r["pred_boxes"][:, None]).all(-1).float().argmax(1)      # the anchors, from their boxes
        assert torch.equal(r["pred_scores"], out["batch_cls_preds"][s][rows].max(-1)[0])
    monkeypatch.setenv("LVQ_HEAD_TORCH_POST", "1")
    same_lists(raw, post(name, out, raw=True))


@pytest.mark.parametrize("name", ["kitti", "wide"])
def test_run_to_run_and_batch_composition_bit_identity(name):
    thresh = AC.MODULE_CASES[name]["post"]["score_thresh"]
    a, b = forward(name, thresh=thresh), forward(name, thresh=thresh)
    for k in ("batch_cls_preds", "batch_box_preds", "anchor_scores", "anchor_labels"):
        assert torch.equal(a[k], b[k]), k
    la, lb = post(name, a), post(name, b)
    same_lists(la, lb)
    x = AC.case_input(name)
    alone = forward(name, x=x[:1], thresh=thresh)
    assert torch.equal(alone["batch_cls_preds"][0], a["batch_cls_preds"][0]) and torch.equal(alone["batch_box_preds"][0], a["batch_box_preds"][0])
    same_lists(post(name, alone), la[:1])


def test_refusals_on_the_device():
    c = AC.MODULE_CASES["nodir"]
    wide_in = AH.AnchorHeadSingle(AC.case_cfg("nodir"), 576, 1, c["class_names"], np.array(c["grid_size"]), c["point_cloud_range"]).to(DEV).eval()
    with torch.no_grad(), pytest.raises(F.LvqError, match="512"):
        wide_in(dict(spatial_features_2d=torch.zeros((1, 576, 16, 24), device=DEV), batch_size=1))
    with torch.no_grad(), pytest.raises(F.LvqError, match="anchors were built"):
        head("nodir")(dict(spatial_features_2d=torch.zeros((1, 64, 8, 24), device=DEV), batch_size=1))
    with pytest.raises(F.LvqError, match="inference-only"):
        head("nodir")(dict(spatial_features_2d=torch.zeros((1, 64, 16, 24), device=DEV), batch_size=1))       # grad mode
    head("nodir").precision = "fp8"
    with torch.no_grad(), pytest.raises(F.LvqError, match="runs in"):
        head("nodir")(dict(spatial_features_2d=torch.zeros((1, 64, 16, 24), device=DEV), batch_size=1))
    head("nodir").precision = None
    out = forward("nodir")
    for kw, word in ((dict(multi=True), "MULTI_CLASSES_NMS"), (dict(nms_type="nms_normal_gpu"), "nms_normal_gpu"), (dict(pre=4097), "4096")):
        with pytest.raises(F.LvqError, match=word):
            post("nodir", out, **kw)
    with pytest.raises(F.LvqError, match="roi_labels"):
        post("nodir", dict(out, roi_labels=torch.ones((2, 4), device=DEV)))
