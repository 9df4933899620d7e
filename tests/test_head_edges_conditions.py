"""CPU-side conditions of the cases that tests/test_gpu_anchor_head_edges.py and tests/test_gpu_voxelnext_head_edges.py run: each case
reaches the route it is there for, the restatements keep inside the shares the GPU tests allow them, and the default random streams of the
case builders that earlier tests run on are where they were."""
import zlib

import numpy as np
import pytest

import anchor_head_cases as AC
import voxelnext_head_cases as VC


def crc(*arrays):
    return zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))


# ---------------------------------------------------------------------------------------------------------------------------------
# the streams of the existing cases
# ---------------------------------------------------------------------------------------------------------------------------------
DECODE_CRC = {(1, 1, 1, 2, 1, True): (0xd39b76a7, 0x26072952), (2, 5, 7, 6, 3, True): (0xd51f72bf, 0x4c0a310f),
              (1, 16, 24, 6, 3, True): (0x3defc71a, 0x7c431fe8), (1, 16, 24, 6, 3, False): (0x35673524, 0xb232a5a9),
              (1, 3, 70, 4, 2, True): (0x21aaf518, 0xf3847635)}
SELECT_CRC = {"n1": 0x57ef8d4f, "n63": 0xea530127, "n65": 0x3fd7e95d, "counts_around_pre_max": 0x206ea37f, "over_1024": 0x8bb8b7ac,
              "over_4096": 0xbd7b92ba, "empty_next_to_full": 0x7fc19713, "plateau_across_pre_max": 0x49b785a7, "plateau_wide": 0xf212280c,
              "nan_no_thresh": 0xfc192ad3, "nan_thresh": 0xda0f9b88}


def test_decode_and_select_default_streams_are_pinned():
    assert list(DECODE_CRC) == AC.DECODE_SHAPES and list(SELECT_CRC) == list(AC.SELECT_CASES)
    for shape, want in DECODE_CRC.items():
        maps, anchors, _ = AC.decode_case(*shape)
        assert (crc(maps), crc(anchors)) == want, shape
        again = AC.decode_case(*shape, AC.NUM_DIR_BINS)[0]
        assert np.array_equal(maps, again)
    for name, want in SELECT_CRC.items():
        assert crc(*AC.select_case(name)[:3]) == want, name


def test_rows_case_default_stream_is_pinned():
    import test_gpu_voxelnext_head as T                                           # the builder lives with the tests that run on it
    for args, kw, want in ((((60, 50), 2, True, 31), {}, 0x1a4e8277), (((40, 0, 45), 2, False, 32), dict(extra_b=3), 0x1cecad80)):
        idx, task = T.rows_case(*args, **kw)
        assert crc(idx, *[task[k] for k in sorted(task)]) == want


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_anchor_decode
# ---------------------------------------------------------------------------------------------------------------------------------
def test_decode_shapes_force_their_tile_widths():
    assert sorted(AC.DECODE_EDGE_SHAPES.values()) == [1, 2, 8, 16, 32, 64]
    for shape, px in AC.DECODE_EDGE_SHAPES.items():
        a, n_cls = shape[3], shape[4]
        assert AC.decode_px(a, n_cls) == px, shape
        assert px == 64 or AC.decode_tile_bytes(2 * px, a, n_cls) > AC.DECODE_LDS
        hw = shape[1] * shape[2]
        print(f"{shape}: px {px}, {a * (n_cls + 10)} words per pixel, tiles of {[min(px, hw - p) for p in range(0, hw, px)]} pixels")
    assert AC.decode_tile_bytes(64, 12, 6) - AC.DECODE_LDS == 16                 # 192 words per pixel: 16 bytes over at 64
    assert [min(16, 35 - p) for p in range(0, 35, 16)] == [16, 16, 3]
    assert all(a * (n_cls + 10) <= 78 for _, _, _, a, n_cls, _ in AC.DECODE_SHAPES)          # what the first suite runs: always 64
    for shape in AC.CAND_SHAPES:
        assert shape[0] == 3 and AC.decode_px(shape[3], shape[4]) in (64, 16)
    assert {AC.decode_px(s[3], s[4]) for s in AC.CAND_SHAPES} == {64, 16}


def test_decode_limit_shapes_sit_exactly_on_48_kb():
    for a, n_cls, px in AC.DECODE_ON_THE_LIMIT:
        assert AC.decode_tile_bytes(px, a, n_cls) == AC.DECODE_LDS == 49152 and AC.decode_px(a, n_cls) == px
        assert (1, 1, 5 if px == 2 else 3, a, n_cls, True) in AC.DECODE_EDGE_SHAPES
    a, n_cls = AC.DECODE_REFUSED
    assert AC.decode_px(a, n_cls) is None and a * (n_cls + 10) == 12284 + 74 and 166 * 74 == 12284          # lvq.h's limit
    assert AC.decode_px(2, 64) == 64                                              # 65 classes are refused for the class count alone


def test_decode_output_runs_start_at_every_residue():
    starts = [s % 4 for shape, px in AC.DECODE_EDGE_SHAPES.items() for s in AC.decode_run_starts(shape, px)]
    assert set(starts) == {0, 1, 2, 3}


def test_heading_shares_of_the_restatement():
    """The GPU tests leave out the headings within 1e-4 of a period boundary and cap their share at 1 %: the restatement alone stays
    within that for the chosen seeds, whatever a kernel does."""
    cases = [(shape, ()) for shape in AC.DECODE_EDGE_SHAPES if shape[5]]
    cases += [(AC.DIR_SHAPE, (bins, off, lim)) for bins, lim, off in AC.DIR_PARAMS]
    for shape, extra in cases:
        ref = AC.decode_case_ref(*shape, *extra)
        share = float((~AC.heading_clear(ref["frac"])).mean())
        print(f"{shape} {extra}: {share:.4f} of the headings within 1e-4 of a boundary")
        assert share <= 0.01
        bins = extra[0] if extra else AC.NUM_DIR_BINS
        assert set(np.unique(ref["bins"]).tolist()) == set(range(bins))
    for rule, want in (("tie", 1), ("nan0", 0), ("nan2", 2), ("nan13", 1)):
        maps, w = AC.dir_bin_case(rule)
        ref = AC.decode_case_ref(*AC.DIR_SHAPE, 4, 0.0, 0.5, maps=maps)
        rows = np.arange(ref["bins"].shape[1]) % AC.DIR_SHAPE[3] == 1
        assert w == want and (ref["bins"][0, rows] == want).all() and (~AC.heading_clear(ref["frac"]))[0, rows].mean() <= 0.01
        assert not np.isnan(ref["boxes"]).any()                                   # a NaN logit picks the bin, it does not reach the heading


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_anchor_select
# ---------------------------------------------------------------------------------------------------------------------------------
def test_signed_scores_hold_what_they_claim():
    scores, _, _ = AC.signed_case()
    for s in range(2):
        u = scores[s].view(np.uint32)
        assert sorted(np.nonzero(u == 0x80000000)[0].tolist()) == sorted(AC.SIGNED_ZEROS["neg"])
        assert sorted(np.nonzero(u == 0)[0].tolist()) == sorted(AC.SIGNED_ZEROS["pos"])
        assert (u == 0x7fc00000).sum() == 3 and (u == 0xffc00000).sum() == 3 and np.isnan(scores[s]).sum() == 6
        for v in (np.inf, -np.inf, 1e-45, -1e-45, -AC.FLT_MAX):
            assert (scores[s] == np.float32(v)).sum() == 1
        assert len(np.unique(u)) == AC.SIGNED_N - 8 - 4                           # everything else is distinct (two zeros, two NaN patterns)
    merged = sorted(AC.SIGNED_ZEROS["neg"] + AC.SIGNED_ZEROS["pos"])
    signs = [i in AC.SIGNED_ZEROS["neg"] for i in merged]
    assert signs[0] and signs[-1] and sum(a != b for a, b in zip(signs, signs[1:])) >= 7          # interleaved


@pytest.mark.parametrize("thresh", [None, -1.5, 0.0])
def test_the_zero_block_straddles_the_cut(thresh):
    scores, _, _ = AC.signed_case()
    cut = AC.signed_cut(scores, thresh)
    merged = sorted(AC.SIGNED_ZEROS["neg"] + AC.SIGNED_ZEROS["pos"])
    for s in range(2):
        order = AC.select_ref(scores[s], thresh, 4096)
        block = order[cut - 4:cut + 6]
        assert block.tolist() == merged and (scores[s][block] == 0).all()         # ten zeros by index, four in front of the cut
        assert scores[s][order[cut - 5]] == np.float32(1e-45)
        assert AC.select_ref(scores[s], thresh, cut).tolist() == order[:cut].tolist()
        taken = order[cut - 4:cut]
        assert {i in AC.SIGNED_ZEROS["neg"] for i in taken.tolist()} == {True, False}          # an order by sign would take other anchors
        by_sign = sorted(AC.SIGNED_ZEROS["pos"])[:4]
        assert taken.tolist() != by_sign
        if thresh is None:
            assert np.isnan(scores[s][order[:6]]).all() and scores[s][order[6]] == np.inf and scores[s][order[-1]] == -np.inf
            assert scores[s][order[-2]] == -AC.FLT_MAX and order[:6].tolist() == sorted(order[:6].tolist())
        elif thresh == 0.0:
            assert len(order) == cut + 6 and (scores[s][order] >= 0).all()       # -0.0 passes `>= 0.0`


@pytest.mark.parametrize("name", AC.SELECT_EDGE_CASES)
def test_select_ref_is_the_documented_order(name):
    scores, _, _, variants = AC.select_edge_variants(name)
    for thresh, pre_max in variants:
        for s in range(scores.shape[0]):
            assert np.array_equal(AC.select_ref(scores[s], thresh, pre_max), AC.select_by_keys(scores[s], thresh, pre_max))
    keys = AC.documented_keys(np.float32([-0.0, 0.0, -np.inf, np.inf, np.nan, -1e-45, 1e-45, -AC.FLT_MAX]))
    assert keys[0] == keys[1] == 0x80000000 and keys[2] == 0x007fffff and keys[4] == 0xffffffff and keys[5] == 0x7ffffffe and keys.min() > 0
    if name == "k_sizes":
        with np.errstate(invalid="ignore"):
            assert ((scores >= np.float32(AC.SELECT_THRESH)).sum(1) == AC.K_SIZES_SURVIVORS).all()
        sort_sizes = [max(2, 1 << (k - 1).bit_length()) for k in AC.K_SIZES]
        assert sort_sizes == [2, 2, 4, 4096, 4096]


@pytest.mark.parametrize("name", ["plateau_across_pre_max", "counts_around_pre_max"])
def test_spliced_lists(name):
    scores, _, _, _, thresh = AC.select_case(name)
    rng = np.random.default_rng(6)
    for s in range(scores.shape[0]):
        row, m = AC.spliced_list(scores[s], thresh, rng, -1)
        n = scores[s].size
        head = row[:m]
        live = head[(head >= 0) & (head < n)]
        assert len(np.unique(live)) == len(live)                                  # the contract: all different
        assert {-1, 2 ** 31 - 1} <= set(head.tolist()) and (head == n).sum() == 1 and (head == n + 7).sum() == 1
        with np.errstate(invalid="ignore"):
            assert (scores[s][live] < np.float32(thresh)).sum() == 20 and (row[m:] == -1).all()
            assert np.array_equal(np.sort(live[scores[s][live] >= np.float32(thresh)]), np.nonzero(scores[s] >= np.float32(thresh))[0])


def test_zero_scene_of_the_module_cases():
    """A scene of zeros: kitti's cls biases lie far below SCORE_THRESH (nothing survives); wide's classes 0 and 1 have a bias of +0.8, so
    every one of their anchors survives with ONE score, and NMS_PRE_MAXSIZE cuts that plateau."""
    for name, survivors in (("kitti", 0), ("wide", 1536)):
        _, dec, final = AC.case_ref_x(name, AC.empty_scene_input(name))
        ref = AC.case_ref(name)[2]
        assert final[1]["survivors"] == survivors and [final[0]["survivors"], final[2]["survivors"]] == [ref[0]["survivors"], ref[1]["survivors"]]
        for a, b in ((final[0], ref[0]), (final[2], ref[1])):
            assert np.array_equal(a["index"], b["index"])
        if survivors:
            sc = dec["scores"][1]
            assert len(np.unique(sc[sc >= AC.SCORE_THRESH])) == 1 and survivors > AC.MODULE_CASES[name]["post"]["pre"]
            assert final[1]["sel"].tolist() == np.nonzero(sc >= AC.SCORE_THRESH)[0][:1400].tolist()
            iou = final[1]["iou"]
            assert (np.abs(iou[np.triu_indices(len(iou), 1)] - 0.7) > 0.2).all() and 0 < len(final[1]["index"]) < 1400
            fr = dec["frac"][1][final[1]["sel"]]
            assert np.abs(fr - np.rint(fr)).min() > 0.1
        else:
            assert len(final[1]["index"]) == 0 and dec["scores"][1].max() < 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_sparse_head
# ---------------------------------------------------------------------------------------------------------------------------------
def test_edge_layouts_launch_the_four_branch_kernel():
    assert sorted(len(w) for ws in VC.EDGE_LAYOUTS.values() for w in ws) == [1, 2, 3, 4]
    for name, kvol, n in VC.EDGE_SIZES:
        c = VC.edge_head_case(name, n, kvol)
        assert max(c["n_br"]) <= 4 and c["bs"] == max(c["n_br"]) and c["ref"].shape == (16 * len(c["n_br"]), n)
        assert all(sum(w) <= VC.TASK_C for w in VC.EDGE_LAYOUTS[name])
    c = VC.edge_head_case("wide_pitch", 200, 9, 8)
    assert c["n_br"] == [5, 5] and c["bs"] == 8 and c["w1"].shape[:2] == (2, 8) and c["scale"].shape[:2] == (2, 8)


def test_tables_lack_the_offsets_they_claim():
    n = 200
    nbr = VC.edge_head_case("three_four", n, 9, None, "structured")["nbr"]
    tiles, blocks = VC.tile_lacks(nbr, n)
    print(f"structured: tiles lack {tiles}, blocks lack {blocks}")
    full = [[o for o in range(9) if o not in have] for have in VC.STRUCTURED_OFFSETS]
    assert tiles == [[], [], [], [1, 2, 3, 5, 6, 7, 8]]                          # the last tile has rows 192 .. 199 only: offsets 0 and 4
    for t, b in enumerate(blocks):
        assert b == full[:len(b)] and len(b) == (4 if t < 3 else 1)
    nbr = VC.edge_head_case("three_four", n, 9, None, "sparse5")["nbr"]
    tiles, blocks = VC.tile_lacks(nbr, n)
    print(f"sparse5: tiles lack {tiles}, blocks lack {blocks}")
    ok = (nbr >= 0) & (nbr < n)
    assert (nbr[:, 4] == np.arange(n)).all() and 0.03 <= ok[:, [0, 1, 2, 3, 5, 6, 7, 8]].mean() <= 0.07
    assert any(tiles) and all(4 not in b for bs in blocks for b in bs) and sum(len(b) for bs in blocks for b in bs) >= 40
    dense = VC.edge_head_case("three_four", n, 9)["nbr"]
    assert not any(VC.tile_lacks(dense, n)[0][:3])                                # the 60 % tables skip nothing in a full tile


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_voxel_decode
# ---------------------------------------------------------------------------------------------------------------------------------
def test_multi_task_case():
    idx, tasks = VC.multi_task_case()
    assert [t["hm"].shape[1] for t in tasks] == list(VC.MULTI_N_CLS) and all("vel" in t for t in tasks)
    assert np.bincount(idx[:, 0] + 1).tolist() == [2, *VC.MULTI_ROWS, 3]          # b = -1 twice, the scenes, b = batch three times
    ids = [c for row in VC.MULTI_IDS for c in row]
    assert len(set(ids)) == len(ids) == sum(VC.MULTI_N_CLS)
    b = idx[:, 0]
    assert (np.diff(b) != 0).mean() > 0.5                                         # interleaved
    buf, chans = VC.head_buffer(tasks)
    assert buf.shape == (48, len(idx)) and [row[5] for row in chans] == [16 * t + 10 for t in range(3)]
    cut = [-2.8, -10.0, -10.0, 2.8, 10.0, 10.0]                                   # test_gpu_voxelnext_head.CUT
    for t, task in enumerate(tasks):
        for s, d in enumerate(VC.decode_ref(task, idx, 3, VC.MULTI_K, 4, (0.2, 0.2), (-3.2, -3.2), cut, 0.1, VC.MULTI_IDS[t])):
            distinct, _, near_thresh, near_limit = VC.decode_margins(d, min(VC.MULTI_K, len(d["cand_boxes"])), cut, 0.1)
            print(f"task {t} scene {s}: {len(d['scores'])} rows of n_b {d['n_b']}; margins {distinct} ulps, {near_thresh:.1e}, {near_limit:.1e}")
            assert distinct >= 4 and near_thresh >= 1e-4 and near_limit >= 1e-3 and 0 < len(d["scores"]) <= VC.MULTI_K


def test_plateau_case_reaches_its_route():
    idx, task = VC.plateau_case()
    above, equal, need, chunk, owners, between = VC.plateau_stats(idx, task, 1, VC.PLATEAU_K)
    print(f"plateau: above {above}, equal {equal}, need {need}, {chunk} keys per thread, {owners} threads own plateau keys, "
          f"{between} foreign positions inside the plateau's span")
    assert (above, equal, need, chunk) == (VC.PLATEAU_ABOVE, VC.PLATEAU_EQUAL, VC.PLATEAU_K - VC.PLATEAU_ABOVE, 3) == (23, 700, 41, 3)
    assert len(idx) == 1500 and task["hm"].shape[1] == 2 and owners >= 400 and between >= 300
    rows1 = idx[:, 0] == 1
    level = (task["hm"] == np.float32(VC.PLATEAU_LOGIT)) & rows1[:, None]
    assert level[:, 0].any() and level[:, 1].any() and int(level.sum()) == 700   # both classes
