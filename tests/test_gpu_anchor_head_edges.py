"""The routes of csrc/anchor_head.hip and anchor_head.py that tests/test_gpu_anchor_head.py does not reach, on the MI355X against the fp64
restatements of tests/anchor_head_cases.py (tests/test_head_edges_conditions.py asserts on the CPU that each case reaches its route).

  decode   the tile widths 32, 16, 8, 2, 1 (the last two exactly at 48 KB of LDS), through the C ABI into filled buffers with a tail; the
           refusals leave every output filled; 2, 3 and 4 direction bins with a dir_limit_offset; the bin argmax's tie and NaN rules; the
           candidate set with every slot of every tile taken, and with none
  select   signed scores (-0.0 and +0.0 are one score, +-inf, denormals, -FLT_MAX, NaNs of both signs), with and without a threshold,
           -0.0 ON the threshold; pre_max 1, 2, 3, 4095, 4096; lists with entries that take no part and counts outside 0 .. n
  NMS      lvq_nms_bev_wide clamps its counts; NaN / 1e30 rows behind them change nothing
  module   a scene of zeros among two others on four routes; a candidate list made for another threshold is ignored; in-place edits of
           the dense outputs after the forward; normalized and single-column batch_cls_preds; torch.inference_mode()

Measured on the MI355X on 2026-10-21 against DECODE_BAR = 1e-5: scores 5.96e-8 at every shape; boxes 4.23e-7 (px 32), 2.01e-7 (16),
2.33e-7 (8), 2.39e-7 (2), 2.59e-7 (1), 1.00e-7 (the four-scene shape); 4 / 3 / 2 bins 1.91e-7 / 1.90e-7 / 2.35e-7 with 1 / 0 / 1 of 420
headings left out.  Everything else here is exact.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import anchor_head_cases as AC  # noqa: E402
import test_gpu_anchor_head as T  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import ops  # noqa: E402

DEV = T.DEV
dev, bits = T.dev, T.bits
LVQ_EINVAL = -1                                   # include/lvq.h
FILL, FILL_I, TAIL = -777.25, -12345, 37


# ---------------------------------------------------------------------------------------------------------------------------------
# decode, through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def decode_abi(shape, n_bins=AC.NUM_DIR_BINS, dir_offset=AC.DIR_OFFSET, limit_offset=AC.DIR_LIMIT_OFFSET, maps=None, thresh=None, c_total=None,
               cand_count=True):
    """One lvq_anchor_decode into buffers filled with FILL / FILL_I that carry TAIL more elements than the call may write.  -> (rc, dict of
    numpy arrays WITH their tails, N).  thresh None: cand and cand_count are NULL; cand_count False: cand without cand_count."""
    b, h, w, a, n_cls, use_dir = shape
    m, anchors, (c0, c1, c2) = AC.decode_case(*shape, n_bins if use_dir else AC.NUM_DIR_BINS)
    d_maps, d_anchors = dev(m if maps is None else maps), dev(anchors)
    n, d = h * w * a, torch.device(DEV)
    out = dict(cls=torch.full((b * n * n_cls + TAIL,), FILL, dtype=torch.float32, device=d),
               box=torch.full((b * n * 7 + TAIL,), FILL, dtype=torch.float32, device=d),
               scores=torch.full((b * n + TAIL,), FILL, dtype=torch.float32, device=d),
               labels=torch.full((b * n + TAIL,), FILL_I, dtype=torch.int32, device=d),
               cand=torch.full((b * n + TAIL,), FILL_I, dtype=torch.int32, device=d),
               count=torch.full((b + TAIL,), FILL_I, dtype=torch.int32, device=d))
    listed = thresh is not None
    rc = F.lib().lvq_anchor_decode(F.ptr(d_maps), b, m.shape[1] if c_total is None else c_total, h, w, c0, c1, c2, a, n_cls,
                                   n_bins if use_dir else 0, float(dir_offset), float(limit_offset), F.ptr(d_anchors),
                                   float(thresh) if listed else 0.0, F.ptr(out["cls"]), F.ptr(out["box"]), F.ptr(out["scores"]),
                                   F.ptr(out["labels"]), F.ptr(out["cand"] if listed else None),
                                   F.ptr(out["count"] if listed and cand_count else None), F.stream_ptr(d))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}, n


def fills(name):
    return FILL_I if name in ("labels", "cand", "count") else np.float32(FILL)


def tails_kept(out, b, n, n_cls):
    sizes = dict(cls=b * n * n_cls, box=b * n * 7, scores=b * n, labels=b * n, cand=b * n, count=b)
    return all((out[k][sizes[k]:] == fills(k)).all() and len(out[k]) == sizes[k] + TAIL for k in sizes)


def check_against_ref(shape, out, n, ref, n_bins=AC.NUM_DIR_BINS, dir_offset=AC.DIR_OFFSET, limit_offset=AC.DIR_LIMIT_OFFSET):
    """The bars of test_decode_against_the_restatement: logits and labels exact, scores and boxes within DECODE_BAR, the headings within
    1e-4 of a period boundary left out (at most 1 %), the bin recovered from the heading."""
    b, _, _, a, n_cls, use_dir = shape
    cls, box = out["cls"][:b * n * n_cls].reshape(b, n, n_cls), out["box"][:b * n * 7].reshape(b, n, 7)
    scores, labels = out["scores"][:b * n].reshape(b, n), out["labels"][:b * n].reshape(b, n)
    assert np.array_equal(bits(cls), bits(ref["cls"].astype(np.float32)))
    assert np.array_equal(labels, ref["labels"])
    ok = ~np.isnan(ref["scores"])
    assert np.array_equal(np.isnan(scores), ~ok)
    err_s = (np.abs(scores - ref["scores"].astype(np.float64)) / np.maximum(1.0, np.abs(ref["scores"])))[ok]
    near = ~AC.heading_clear(ref["frac"]) if ref["frac"] is not None else np.zeros(scores.shape, bool)
    err_b = np.abs(box - ref["boxes"]) / np.maximum(1.0, np.abs(ref["boxes"]))
    err_b[..., 6][near] = 0.0
    print(f"{shape} bins {n_bins if use_dir else 0}: score err {err_s.max():.2e}, box err {err_b.max():.2e}, {int(near.sum())} of {near.size} "
          "headings left out")
    assert near.mean() <= 0.01 and err_s.max() <= T.DECODE_BAR and err_b.max() <= T.DECODE_BAR
    got_bin = None
    if use_dir:
        period = np.float64(np.float32(2 * np.pi / n_bins))
        got_bin = np.floor((box[..., 6].astype(np.float64) - np.float64(np.float32(dir_offset))) / period + np.float64(np.float32(limit_offset))
                           + 1e-6)
        assert np.array_equal(got_bin[~near], ref["bins"][~near])
    return got_bin, near


@pytest.mark.parametrize("shape", list(AC.DECODE_EDGE_SHAPES))
def test_decode_tile_widths_against_the_restatement(shape):
    b, _, _, a, n_cls, _ = shape
    rc, out, n = decode_abi(shape)
    assert rc == F.LVQ_OK
    assert tails_kept(out, b, n, n_cls)
    assert (out["cand"] == FILL_I).all() and (out["count"] == FILL_I).all()          # not asked for
    check_against_ref(shape, out, n, AC.decode_case_ref(*shape))


@pytest.mark.parametrize("what", ["167_anchors", "65_classes", "channels_past_c_total", "cand_without_count"])
def test_decode_refusals_write_nothing(what):
    shape, kw, want = {"167_anchors": ((1, 1, 1, AC.DECODE_REFUSED[0], AC.DECODE_REFUSED[1], True), {}, F.LVQ_EUNSUPPORTED),
                       "65_classes": ((1, 1, 1, 2, 65, True), {}, F.LVQ_EUNSUPPORTED),
                       "channels_past_c_total": ((2, 5, 7, 6, 3, True), dict(c_total=6 * 3 + 6 * 7 + 6 * 2 - 1), LVQ_EINVAL),
                       "cand_without_count": ((2, 5, 7, 6, 3, True), dict(thresh=0.3, cand_count=False), LVQ_EINVAL)}[what]
    rc, out, _ = decode_abi(shape, **kw)
    assert rc == want
    assert all((v == fills(k)).all() for k, v in out.items())


@pytest.mark.parametrize("n_bins, limit_offset, dir_offset", AC.DIR_PARAMS)
def test_decode_direction_parameters(n_bins, limit_offset, dir_offset):
    shape = AC.DIR_SHAPE
    rc, out, n = decode_abi(shape, n_bins, dir_offset, limit_offset)
    assert rc == F.LVQ_OK and tails_kept(out, shape[0], n, shape[4])
    ref = AC.decode_case_ref(*shape, n_bins, dir_offset, limit_offset)
    got_bin, near = check_against_ref(shape, out, n, ref, n_bins, dir_offset, limit_offset)
    assert set(np.unique(got_bin[~near]).astype(int).tolist()) == set(range(n_bins))      # every bin is taken somewhere


@pytest.mark.parametrize("rule", ["tie", "nan0", "nan2", "nan13"])
def test_decode_bin_argmax_rules(rule):
    """Two equal top logits give the lower bin; a NaN wins wherever it stands; of two NaNs the lower bin wins.  Through the heading's bin."""
    shape = AC.DIR_SHAPE
    maps, want = AC.dir_bin_case(rule)
    rc, out, n = decode_abi(shape, 4, 0.0, 0.5, maps=maps)
    assert rc == F.LVQ_OK
    ref = AC.decode_case_ref(*shape, 4, 0.0, 0.5, maps=maps)
    got_bin, near = check_against_ref(shape, out, n, ref, 4, 0.0, 0.5)
    rows = np.arange(n) % shape[3] == 1                                               # anchor 1 of every pixel of scene 0
    assert (ref["bins"][0, rows] == want).all() and (got_bin[0, rows][~near[0, rows]] == want).all() and (~near[0, rows]).sum() >= 30


@pytest.mark.parametrize("shape", AC.CAND_SHAPES)
def test_decode_candidate_sets_full_and_empty(shape):
    b, h, w, a, n_cls, _ = shape
    maps = AC.decode_case(*shape)[0].copy()
    maps[1, 2 * n_cls + 1, 3, 4] = np.nan                                             # anchor 2 of pixel (3, 4) of scene 1, class 1
    nan_at = (3 * w + 4) * a + 2
    rc, full, n = decode_abi(shape, maps=maps, thresh=0.0)
    assert rc == F.LVQ_OK and tails_kept(full, b, n, n_cls)
    scores = full["scores"][:b * n].reshape(b, n)
    assert np.isnan(scores[1, nan_at]) and int(np.isnan(scores).sum()) == 1 and (scores[~np.isnan(scores)] > 0).all()
    count, cand = full["count"][:b], full["cand"][:b * n].reshape(b, n)
    assert count.tolist() == [n, n - 1, n]                                           # every slot of every tile, but the NaN's
    for s in range(b):
        assert np.array_equal(np.sort(cand[s, :count[s]]), np.setdiff1d(np.arange(n), [nan_at] if s == 1 else []))
    assert cand[1, n - 1] == FILL_I                                                   # behind the count nothing is written
    rc, none, _ = decode_abi(shape, maps=maps, thresh=2.0)
    assert rc == F.LVQ_OK and tails_kept(none, b, n, n_cls)
    assert (none["count"][:b] == 0).all() and (none["cand"] == FILL_I).all()
    for k in ("cls", "box", "scores", "labels"):
        assert np.array_equal(bits(none[k]), bits(full[k]))


# ---------------------------------------------------------------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------------------------------------------------------------
def shuffled_list(scores, thresh, seed=5):
    rng = np.random.default_rng(seed)
    cand, count = np.zeros(scores.shape, np.int32), np.zeros(scores.shape[0], np.int32)
    for s in range(scores.shape[0]):
        with np.errstate(invalid="ignore"):
            idx = rng.permutation(np.nonzero(scores[s] >= np.float32(thresh))[0])
        cand[s, :len(idx)], count[s] = idx, len(idx)
    return cand, count


@pytest.mark.parametrize("name", AC.SELECT_EDGE_CASES)
def test_select_signed_scores_and_k_sizes(name):
    scores, labels, boxes, variants = AC.select_edge_variants(name)
    d_scores, d_labels, d_boxes = dev(scores), dev(labels, np.int32), dev(boxes)
    assert np.array_equal(bits(d_scores.cpu().numpy()), bits(scores))                 # the NaN payloads and the zeros' signs arrive
    for thresh, pre_max in variants:
        want = T.select_want(scores, labels, boxes, pre_max, thresh)
        print(f"{name}: thresh {thresh}, pre_max {pre_max}: counts {want['count'].tolist()}")
        T.check_select(ops.anchor_select(d_scores, d_labels, d_boxes, score_thresh=thresh, pre_max=pre_max), want)
        if thresh is not None:
            cand, count = shuffled_list(scores, thresh)
            T.check_select(ops.anchor_select(d_scores, d_labels, d_boxes, score_thresh=thresh, pre_max=pre_max, cand=dev(cand, np.int32),
                                             cand_count=dev(count, np.int32)), want)


@pytest.mark.parametrize("name", ["plateau_across_pre_max", "counts_around_pre_max"])
def test_select_lists_with_entries_that_take_no_part(name):
    """-1, n, n + 7, 2^31 - 1 and anchors below the threshold in the list; cand_count above n (clamped to n: the whole row is read, -1
    behind the entries) and negative (clamped to 0: an empty scene)."""
    scores, labels, boxes, pre_max, thresh = AC.select_case(name)
    b, n = scores.shape
    want = T.select_want(scores, labels, boxes, pre_max, thresh)
    d_scores, d_labels, d_boxes = dev(scores), dev(labels, np.int32), dev(boxes)
    scan = ops.anchor_select(d_scores, d_labels, d_boxes, score_thresh=thresh, pre_max=pre_max)
    T.check_select(scan, want)
    rng = np.random.default_rng(6)
    lists = [AC.spliced_list(scores[s], thresh, rng, -1) for s in range(b)]
    cand = np.stack([row for row, _ in lists])
    exact = np.array([m for _, m in lists], np.int32)
    for count in (exact, np.full(b, n + 1000, np.int32), np.full(b, 2 ** 31 - 1, np.int32)):
        got = ops.anchor_select(d_scores, d_labels, d_boxes, score_thresh=thresh, pre_max=pre_max, cand=dev(cand, np.int32),
                                cand_count=dev(count, np.int32))
        T.check_select(got, want)
        assert all(torch.equal(x, y) for x, y in zip(got, scan))
    count = exact.copy()
    count[-1] = -5                                                                    # the last scene's list is not read
    gone = np.array(scores)
    gone[-1] = 0.0                                                                    # ... as if nothing in it reached the threshold
    T.check_select(ops.anchor_select(d_scores, d_labels, d_boxes, score_thresh=thresh, pre_max=pre_max, cand=dev(cand, np.int32),
                                     cand_count=dev(count, np.int32)), T.select_want(gone, labels, boxes, pre_max, thresh))


# ---------------------------------------------------------------------------------------------------------------------------------
# the wide NMS
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_nms_clamps_the_counts():
    """test_nms_clamps_the_counts of the narrow kernel at 64 words: counts above n_max and below zero; NaN / 1e30 rows behind the counts."""
    boxes, counts, ious, _, _ = T.nms_inputs()
    assert counts[0] == 0 and counts[-1] == AC.NMS_WIDE_N_MAX
    given = list(counts)
    given[0], given[-1] = -5, 5000
    dirty = np.array(boxes)
    for g, n in enumerate(counts):
        dirty[g, n::2] = np.nan
        dirty[g, n + 1::2] = 1e30
    for pre_max, post_max in ((4096, 4096), (1090, 37)):
        keep, keep_count = ops.nms_bev_wide(dev(dirty), dev(given, np.int32), thresh=AC.NMS_WIDE_THRESH, pre_max=pre_max, post_max=post_max)
        T.check_keep(keep, keep_count, boxes, counts, ious, pre_max, post_max)
    assert int(keep_count[0]) == 0 and int(keep_count[-1]) == 37


# ---------------------------------------------------------------------------------------------------------------------------------
# module
# ---------------------------------------------------------------------------------------------------------------------------------
def as_golden(final):
    g = {}
    for s, f in enumerate(final):
        g[f"final_{s}_boxes"], g[f"final_{s}_scores"], g[f"final_{s}_labels"] = f["pred_boxes"], f["pred_scores"], f["pred_labels"]
    return g


def is_empty(d):
    return (tuple(d["pred_boxes"].shape), tuple(d["pred_scores"].shape), tuple(d["pred_labels"].shape)) == ((0, 7), (0,), (0,)) and \
        (d["pred_boxes"].dtype, d["pred_scores"].dtype, d["pred_labels"].dtype) == (torch.float32, torch.float32, torch.int64)


def in_order(got, f, bar_box):
    kb, ks, kl = got["pred_boxes"].cpu().numpy(), got["pred_scores"].cpu().numpy(), got["pred_labels"].cpu().numpy()
    assert len(ks) == len(f["pred_scores"]) > 0 and np.array_equal(kl, f["pred_labels"])
    assert np.abs(kb - f["pred_boxes"]).max() <= bar_box and np.abs(ks - f["pred_scores"]).max() <= T.BAR


def plateau_invariants(got, f):
    """What holds for the zero scene of `wide` whichever 1400 of the equal scores were taken: the one score, labels 1 and 2 only, no box
    twice (twins have IoU 1), and a row count between 700 (every kept row removes at most its one twin of the other class) and 768
    (the distinct (cell, rotation) boxes of classes 0 and 1)."""
    kb, ks, kl = got["pred_boxes"].cpu().numpy(), got["pred_scores"].cpu().numpy(), got["pred_labels"].cpu().numpy()
    assert 700 <= len(ks) <= 768 and len(f["pred_scores"]) == 700
    assert np.abs(ks - f["pred_scores"][0]).max() <= T.BAR and set(kl.tolist()) <= {1, 2}
    apart = np.abs(kb[:, None] - kb[None]).max(-1) + np.eye(len(kb))
    assert apart.min() > 1e-2                                                         # (the two rotations of a cell differ in the heading)
    to_scene = np.abs(kb[:, None] - f["all_boxes"][None]).max(-1).min(1)
    assert to_scene.max() <= T.BAR * max(1.0, np.abs(f["all_boxes"]).max())           # every row is one of the scene's boxes


@pytest.mark.parametrize("name", ["kitti", "wide"])
def test_a_scene_of_zeros_among_two_others(name, monkeypatch):
    """Scene 1 of 3 is all zeros: its logits are the cls biases.  kitti: far below SCORE_THRESH, three empty tensors.  wide: its classes 0
    and 1 have a bias of +0.8, so 1536 anchors share ONE score above the threshold and NMS_PRE_MAXSIZE 1400 cuts that plateau: the
    restatement's lists there as well (torch.topk leaves the order of equal scores open, so the torch route is compared on scenes 0 and 2)."""
    x = AC.empty_scene_input(name)
    _, dec, final = AC.case_ref_x(name, x)
    g = as_golden(final)
    bar_box = T.BAR * max(1.0, np.abs(dec["boxes"]).max())
    thresh = AC.MODULE_CASES[name]["post"]["score_thresh"]
    empty = len(final[1]["pred_scores"]) == 0
    final[1]["all_boxes"] = dec["boxes"][1].astype(np.float32)
    assert empty == (name == "kitti") and len(final[0]["pred_scores"]) and len(final[2]["pred_scores"])
    out = T.forward(name, x=x)
    kernel = T.post(name, out)
    listed = T.forward(name, x=x, thresh=thresh)
    assert int(listed["anchor_candidates"][2][1]) == final[1]["survivors"]
    raw = T.post(name, out, raw=True)
    monkeypatch.setenv("LVQ_HEAD_TORCH_POST", "1")
    by_torch = T.post(name, out)
    monkeypatch.delenv("LVQ_HEAD_TORCH_POST")
    for route, lists in (("kernel", kernel), ("candidates", T.post(name, listed)), ("torch", by_torch), ("raw", raw)):
        assert len(lists) == 3
        for s in range(3):
            if empty and s == 1:
                assert is_empty(lists[s]), route
            elif route == "raw":
                assert torch.equal(lists[s]["pred_boxes"], kernel[s]["pred_boxes"]) and torch.equal(lists[s]["pred_labels"], kernel[s]["pred_labels"])
                assert (torch.sigmoid(lists[s]["pred_scores"]) - kernel[s]["pred_scores"]).abs().max() <= 1e-6
            elif s == 1 and route != "torch":                                         # equal scores, and the two rotations of a cell share a
                in_order(lists[s], final[s], bar_box)                                 # centre: row by row, in the documented tie order
            elif s != 1:
                T.match_lists(lists[s], g, s, bar_box)
            else:                                                                     # torch.topk takes ANY 1400 of the 1536 equal scores
                plateau_invariants(lists[s], final[s])
    T.same_lists(kernel, T.post(name, listed))


@pytest.mark.parametrize("name", ["kitti", "wide"])
def test_a_candidate_list_for_another_threshold_is_ignored(name):
    thresh = AC.MODULE_CASES[name]["post"]["score_thresh"]
    plain = T.post(name, T.forward(name))
    for other in (thresh + 0.2, thresh - 0.05):
        listed = T.forward(name, thresh=other)
        assert listed["anchor_candidates"] is not None and listed["anchor_candidates"][0] == other
        T.same_lists(plain, T.post(name, listed))


@pytest.mark.parametrize("which", ["batch_cls_preds", "batch_box_preds"])
def test_in_place_edits_after_the_forward(which, monkeypatch):
    """The forward's scores, labels and candidate list belong to the dense tensors as the forward left them: after an in-place edit the
    lists are those of the tensors as they are now."""
    name = "kitti"
    out = T.forward(name, thresh=AC.MODULE_CASES[name]["post"]["score_thresh"])
    before = T.post(name, out)
    out[which].mul_(0.5)
    after = T.post(name, out)
    monkeypatch.setenv("LVQ_HEAD_TORCH_POST", "1")
    want = T.post(name, out)
    T.same_lists(after, want)
    assert sum(len(d["pred_scores"]) for d in want) > 0
    assert any(len(a["pred_scores"]) != len(b["pred_scores"]) or not torch.equal(a["pred_boxes"], b["pred_boxes"]) for a, b in zip(before, after))


@pytest.mark.parametrize("form", ["normalized", "one_column"])
def test_foreign_forms_of_batch_cls_preds(form, monkeypatch):
    name = "kitti"
    out = T.forward(name)
    cls = torch.sigmoid(out["batch_cls_preds"]) if form == "normalized" else out["batch_cls_preds"][..., :1]
    foreign = dict(batch_cls_preds=cls, batch_box_preds=out["batch_box_preds"].clone(), batch_size=2, cls_preds_normalized=form == "normalized")
    got = T.post(name, foreign)
    monkeypatch.setenv("LVQ_HEAD_TORCH_POST", "1")
    want = T.post(name, foreign)
    T.same_lists(got, want)
    assert sum(len(d["pred_scores"]) for d in want) > 0
    if form == "one_column":
        assert all((d["pred_labels"] == 1).all() for d in got)


@pytest.mark.parametrize("name", ["kitti", "nodir"])
def test_forward_and_post_processing_under_inference_mode(name, monkeypatch):
    """torch.inference_mode() is how the reference's driver runs its detector.  The outputs are inference tensors, which count no versions:
    no version is recorded, post_processing takes the "from elsewhere" route, and the lists are those of a torch.no_grad() forward; after
    an in-place edit they are those of the tensors as they are now."""
    thresh = AC.MODULE_CASES[name]["post"]["score_thresh"]
    plain = T.post(name, T.forward(name, thresh=thresh))
    with torch.inference_mode():
        out = T.forward(name, thresh=thresh)
        assert out["batch_cls_preds"].is_inference() and out["anchor_source"][2] is None
        T.same_lists(plain, T.post(name, out))
        if name == "kitti":
            out["batch_cls_preds"].mul_(0.5)
            after = T.post(name, out)
            monkeypatch.setenv("LVQ_HEAD_TORCH_POST", "1")
            T.same_lists(after, T.post(name, out))
            monkeypatch.delenv("LVQ_HEAD_TORCH_POST")
            assert any(len(a["pred_scores"]) != len(b["pred_scores"]) or not torch.equal(a["pred_boxes"], b["pred_boxes"])
                       for a, b in zip(plain, after))
    T.same_lists(plain, T.post(name, T.forward(name, thresh=thresh)))                 # and a no_grad forward behind it is what it was
