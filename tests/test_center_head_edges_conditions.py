"""CPU-side conditions of the cases that tests/test_gpu_center_head_edges.py runs: the tie classes the radix select meets, the separation of
scores that are not equal, the NaN order pinned to torch.topk, the NMS margins and suppressed shares, the exact limit geometry."""
import numpy as np
import pytest
import torch

import center_head_cases as CC

# name -> per task (strictly above the K-th, equal to it, needed of those, cells per thread) that both scenes must show
TIE_ROUTES = {
    "plateau_straddles_k": [(23, 200, 41, 2), (23, 200, 41, 1)],
    "plateau_chunk3": [(23, 700, 477, 3), (23, 700, 477, 1)],
    "plateau_fills_exactly": [(23, 41, 41, 2), (23, 41, 41, 1)],
    "saturated": [(0, 100, 64, 2), (0, 100, 64, 1)],
    "all_equal_chunked": [(0, 2048, 1024, 2), (0, 1024, 1024, 1)],
    "zeros_at_the_bottom": [(40, 1400, 24, 2), (40, 680, 24, 1)],
}


@pytest.mark.parametrize("name", list(CC.TIE_CASES))
def test_tie_cases_reach_their_routes(name):
    h, w, k, classes, thresh, _ = CC.TIE_CASES[name]
    maps, chans, ids, tasks = CC.tie_case(name)
    assert sorted(c for row in ids for c in row) == list(range(sum(classes)))           # a permutation
    for ti, task in enumerate(tasks):
        assert not task["center"].any()
        dec = CC.decode_ref(task, k, CC.TIE_STRIDE, CC.TIE_VOXEL, [0.0, 0.0], CC.WIDE_LIMIT, thresh, ids[ti])
        layouts = []
        for s, d in enumerate(dec):
            stats = CC.select_stats(task["hm"][s], k)
            print(f"{name} task {ti} scene {s}: above {stats[0]}, equal {stats[1]}, need {stats[2]}, chunk {stats[3]}")
            assert stats == TIE_ROUTES[name][ti]
            assert len(d["scores"]) == k                                                  # every winner survives the masks
            assert CC.tie_separation(d["cand_scores"]) >= 64                             # not bit-equal: at least 64 ulps apart
            assert np.array_equal(CC.tie_flat(d["boxes"], d["labels"], ids[ti], h, w), d["flat"])       # a row names its cell
            layouts.append(d["flat"])
        if name != "all_equal_chunked":
            assert not np.array_equal(layouts[0], layouts[1])
    if name.startswith("plateau") or name == "saturated":
        hm = tasks[0]["hm"][0].reshape(-1)
        level = hm == CC.PLATEAU if name.startswith("plateau") else hm >= 20
        chunk = TIE_ROUTES[name][0][3]
        per_thread = np.add.reduceat(level.astype(int), np.arange(0, hm.size, chunk))
        assert level[0] and level[-1] and per_thread.max() == chunk and (per_thread == 0).any()
        assert level[:h * w].any() and level[h * w:].any()                               # both classes


def test_saturated_and_zero_classes_are_exact():
    x = np.float32(CC.SATURATED)
    assert (np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32)) == 1).all() and (CC.scores32(x) == 1).all()
    assert CC.scores32(np.float32([np.inf, -np.inf])).tolist() == [1.0, 0.0]
    assert np.isinf(CC.tie_case("saturated")[3][0]["hm"]).any()


def test_nan_order_is_torch_topk_s():
    maps, chans, ids, tasks = CC.nan_case()
    bits = tasks[0]["hm"].reshape(2, -1).view(np.uint32)
    assert sorted(bits[0, list(CC.NAN_CELLS)].tolist()) == [0x7fc00000] * 3 + [0xffc00000] * 3
    k, nn = 32, len(CC.NAN_CELLS)
    _, _, _, _, _, _, stride, _ = CC.DECODE_CASES["small_k32"]
    voxel, rng, limit = CC.decode_geometry("small_k32")
    for thresh in (None, CC.SCORE_THRESH):
        for s, d in enumerate(CC.decode_ref(tasks[0], k, stride, voxel, rng, limit, thresh, ids[0])):
            sc = torch.from_numpy(CC.scores32(tasks[0]["hm"][s]).reshape(-1))
            top = torch.topk(sc, k)
            assert torch.isnan(top.values[:nn]).all() and set(top.indices[:nn].tolist()) == set(CC.NAN_CELLS)
            if thresh is None:
                assert set(d["flat"][:nn].tolist()) == set(CC.NAN_CELLS) and len(d["scores"]) >= nn + 20
                assert np.array_equal(np.sort(top.indices[nn:].numpy()), np.sort(np.setdiff1d(top.indices[nn:].numpy(), CC.NAN_CELLS)))
            else:
                assert not np.isnan(d["scores"]).any() and len(d["scores"]) <= k - nn
                if s == 0:                                                    # more than K finite scores pass: NaNs sorted last would show as K rows
                    assert int((sc > np.float32(thresh)).sum()) >= k + nn and len(d["scores"]) >= k - nn - 4
            full = CC.decode_ref(tasks[0], k, stride, voxel, rng, limit, thresh, ids[0])[s]
            distinct, _, near_thresh, near_limit = CC.decode_margins(CC.without_nans(full, nn), k - nn, limit, thresh)
            assert distinct >= 4 and near_thresh >= 1e-4 and near_limit >= 1e-2


def test_decode_without_threshold_keeps_its_margins():
    name = CC.DECODE_NO_THRESH
    _, _, _, k, classes, _, stride, _ = CC.DECODE_CASES[name]
    _, _, ids, tasks = CC.decode_case(name)
    voxel, rng, limit = CC.decode_geometry(name)
    for ti, task in enumerate(tasks):
        for d in CC.decode_ref(task, k, stride, voxel, rng, limit, None, ids[ti]):
            distinct, _, _, near_limit = CC.decode_margins(d, k, limit, None)
            assert distinct >= 4 and near_limit >= 1e-2 and 0 < len(d["scores"]) < k


def test_limit_case_is_exact_in_fp32():
    maps, chans, ids, tasks, limit, rng, cells = CC.limit_case()
    for s, d in enumerate(CC.decode_ref(tasks[0], 32, CC.TIE_STRIDE, CC.TIE_VOXEL, rng, limit, CC.SCORE_THRESH, ids[0])):
        assert np.array_equal(d["cand_boxes"][:, :3], d["cand_boxes"][:, :3].astype(np.float32))       # every centre is an fp32 number
        got = sorted((int(f) // 16, int(f) % 16) for f in d["flat"])
        assert got == sorted(c for c, keep in cells.items() if keep)
        on = d["boxes"][:, :3]
        lim = np.asarray(limit)
        assert all((on[:, a] == lim[a]).any() and (on[:, a] == lim[a + 3]).any() for a in range(3))    # a kept row ON each of the six limits
        assert CC.tie_separation(d["cand_scores"][:len(cells)]) >= 64


@pytest.mark.parametrize("name", list(CC.NMS_EDGE_CASES))
def test_nms_edge_cases_keep_their_margins(name):
    thresh, counts, n_max, margin, _ = CC.NMS_EDGE_CASES[name]
    boxes, cnts, ious = CC.nms_edge_case(name)
    assert boxes.shape == (len(counts), n_max, 7) and cnts == list(counts)
    for g, n in enumerate(cnts):
        keep, near = CC.greedy_nms(boxes[g, :n], thresh, 10 ** 6, 10 ** 6, ious[g])
        print(f"{name} group {g}: {n} boxes, {len(keep)} kept, |iou - {thresh}| >= {near:.4f}")
        assert near >= margin
        if name == "low" and n > 1:
            up = ious[g][np.triu_indices(n, 1)]
            assert ((up < 0.005) | (up > 0.015)).all()
        if n >= 64:
            assert len(keep) <= 0.75 * n                                                  # at least a quarter is suppressed
    if name == "wide":
        for g in (0, 1):                                                                  # pre_max = 1000 cuts the two largest groups:
            assert max(CC.greedy_nms(boxes[g, :cnts[g]], thresh, 10 ** 6, 10 ** 6, ious[g])[0]) >= 1000       # a row behind it is kept without it
        assert np.array_equal(boxes, CC.nms_edge_case("wide")[0]) and boxes.dtype == np.float32


def test_nms_case_default_stream_is_pinned():
    """The existing NMS tests run on nms_case() with its defaults: its boxes are pinned by a checksum, so a change of the generator shows."""
    import zlib
    boxes, counts, _ = CC.nms_case()
    assert counts == CC.NMS_COUNTS and zlib.crc32(boxes.tobytes()) == 0xbca11475


def test_nms_chain_case_is_what_it_says():
    boxes, want = CC.nms_chain_case()
    r = CC.NMS_CHAIN_ROWS
    iou = CC.iou_matrix(boxes[0], boxes[0])
    for a, b, c in ((r["a"], r["b"], r["c"]), (r["a2"], r["b2"], r["c2"])):
        assert abs(iou[a, b] - 2.4 / 5.6) < 1e-5 and abs(iou[b, c] - 2.4 / 5.6) < 1e-5 and abs(iou[a, c] - 0.8 / 7.2) < 1e-5     # -99.2 in fp32
    assert r["a"] // 64 == 0 and r["b"] // 64 == 1 and r["c"] // 64 == 10 and r["a2"] // 64 == 0 and r["b2"] // 64 == r["c2"] // 64 == 15
    off = iou.copy()
    for a in r.values():
        for b in r.values():
            off[a, b] = 0
    np.fill_diagonal(off, 0)
    assert off.max() == 0                                                                 # everything else is disjoint
    assert CC.greedy_nms(boxes[0], CC.NMS_THRESH, 4096, 1024, iou)[0] == want and len(want) == 1022


def test_iou_far_bar_is_what_fp32_carries():
    a, b, want = CC.IOU_CLOSED_FORM[CC.IOU_FAR_PAIR]
    assert a[:2] == list(CC.IOU_FAR_OFFSET) and want == 1.0 / 3.0
    ulp = float(np.spacing(np.float32(max(abs(v) for v in CC.IOU_FAR_OFFSET))))
    assert abs(ulp - 2.44e-4) < 1e-6 and 3 * ulp * 2.0 / 9.0 <= CC.IOU_FAR_BAR <= 2 * 3 * ulp * 2.0 / 9.0


def test_collect_case_expectations():
    for run, kc in enumerate(CC.COLLECT_KEEP_COUNTS):
        for post_max in (1, 83):
            _, _, labels, keep, want = CC.collect_case(9, post_max, kc)
            for s in range(2):
                assert len(want[s][1]) == sum(max(0, min(c, post_max)) for c in kc[s]) and (keep[s] < 70).all()
                assert want[s][2].dtype == np.int64 and (len(want[s][2]) == 0 or want[s][2].min() >= 1)


@pytest.mark.parametrize("name", list(CC.MODULE_VARIANTS))
def test_module_variants_keep_their_margins(name):
    cfg, sd, _, _, pre, final, near = CC.variant_ref(name)
    kth_gap, near_thresh, near_iou, near_limit = CC.module_margins(cfg, pre, near)
    print(f"{name}: K-th gap {kth_gap:.2e}, |score - thresh| {near_thresh:.2e}, |iou - thresh| {near_iou:.2e}, |centre - limit| {near_limit:.2e}")
    assert kth_gap >= 1e-3 and near_thresh >= 1e-3 and near_iou >= 0.02 and near_limit >= 1e-2
    assert all(0 < len(f["pred_scores"]) < sum(len(t[s]["scores"]) for t in pre) for s, f in enumerate(final))
    if name == "num_conv1":
        assert not any(".0.0." in k for k in sd if k.startswith("heads_list"))            # one conv per branch
    else:
        assert "SCORE_THRESH" not in cfg.POST_PROCESSING


@pytest.mark.parametrize("name, ks", [("k_sizes", CC.K_SIZES), ("k_is_n", (1024,)), ("stride1", (32,))])
def test_decode_edge_cases_keep_their_margins(name, ks):
    b, h, w, k_max, classes, _, stride, _ = CC.DECODE_EDGE_CASES[name]
    _, _, ids, tasks = CC.decode_case(name)
    voxel, rng, limit = CC.decode_geometry(name)
    assert max(ks) == k_max and (name != "k_sizes" or classes[0] * h * w == 2048) and (name != "k_is_n" or classes[0] * h * w == k_max)
    assert (name == "stride1") == (stride == 1)
    for k in ks:
        counts = []
        for ti, task in enumerate(tasks):
            for d in CC.decode_ref(task, k, stride, voxel, rng, limit, CC.SCORE_THRESH, ids[ti]):
                distinct, _, near_thresh, near_limit = CC.decode_margins(d, k, limit, CC.SCORE_THRESH)
                assert distinct >= 4 and near_thresh >= 1e-4 and near_limit >= 1e-2
                counts.append(len(d["scores"]))
        print(f"{name} K = {k}: survivors {counts}")
        assert 0 in counts and (k < 32 or any(0 < n < k for n in counts))


def test_thin_crossed_pairs_have_their_own_bar():
    for i in CC.IOU_THIN_PAIRS:
        a, b, want = CC.IOU_CLOSED_FORM[i]
        assert a[3] == 0.05 and a[4] == 20.0 and 1e-3 < want < 3e-3 and CC.IOU_THIN_BAR <= 0.01 * want
