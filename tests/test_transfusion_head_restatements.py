"""CPU-side checks of the TransFusionHead work: the module's structure and initial values against the fixtures made from the reference's own
class (tools/make_transfusion_head_golden.py), the fp64 restatements of tests/transfusion_head_cases.py against the same fixtures -- the check
that goldens and restatement agree before any kernel is involved --, the margin conditions every GPU comparison leans on, the non-square
position formula, the registry and the refusals that need no GPU."""
import os

import numpy as np
import pytest
import torch

import transfusion_head_cases as TC
from lidar_vision_vqa_amd import _ffi as F
from lidar_vision_vqa_amd import anchor_head
from lidar_vision_vqa_amd import transfusion_head as TH

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = list(TC.MODULE_CASES)


def golden(name):
    return np.load(os.path.join(GOLDEN, TC.golden_name(name)))


def build(name, seed=0, **kw):
    torch.manual_seed(seed)
    return TH.TransFusionHead(**TC.case_args(name, **kw))


def close(a, ref, tol=1e-5):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return bool((np.abs(a - ref) <= tol * np.maximum(1.0, np.abs(ref))).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# structure
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_state_dict_and_initial_values_are_the_references(name):
    g, m = golden(name), build(name)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]] == [k for k, _ in TC.case_shapes(name)]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g["shapes"]]
    if not TC.MODULE_CASES[name]["bias"]:
        assert len(sd) == 96                       # the reference's yaml: USE_BIAS_BEFORE_NORM False
    # the constructor draws from the RNG in the reference's order: per key, the sum of the fresh values after torch.manual_seed(0)
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    assert np.abs(sums - g["init_sums"]).max() <= 1e-9 * max(1.0, np.abs(g["init_sums"]).max())
    TC.load_state(m, TC.case_state(name))
    assert all(not p.is_cuda for p in m.parameters())
    assert "bev_pos" not in sd and isinstance(m.bev_pos, torch.Tensor) and not isinstance(m.bev_pos, torch.nn.Parameter)
    assert all(mod.momentum == 0.1 for mod in m.modules() if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)))


def test_registry_and_training_refusals():
    assert TH.dense_heads_all["TransFusionHead"] is TH.TransFusionHead
    assert set(anchor_head.dense_heads_all) < set(TH.dense_heads_all)
    m = build("plain")
    for fn in (m.loss, m.get_targets, m.get_targets_single, m.encode_bbox):
        with pytest.raises(F.LvqError):
            fn(None)
    assert list(dict(m.named_children())) == ["loss_cls", "loss_bbox", "loss_heatmap", "shared_conv", "heatmap_head", "class_encoding", "decoder",
                                              "prediction_head"]
    with pytest.raises(F.LvqError, match="use_sigmoid"):
        build("plain", use_sigmoid=False)
    with pytest.raises(F.LvqError), torch.no_grad():          # a CPU tensor: there is no fallback
        m.eval()(dict(spatial_features_2d=torch.zeros(1, 64, 12, 20)))


@pytest.mark.parametrize("kw, word", [(dict(hidden=64), "HIDDEN_CHANNEL"), (dict(ffn=96), "FFN_CHANNEL"), (dict(ffn=1024), "FFN_CHANNEL"),
                                      (dict(activation="gelu"), "ACTIVATION"), (dict(num_conv=1, hm_conv=1), "num_conv"), (dict(hm_conv=3), "num_conv"),
                                      (dict(p=1025), "NUM_PROPOSALS"), (dict(nms_kernel=5), "NMS_KERNEL_SIZE"),
                                      (dict(branches=["center", "height", "dim", "rot", "iou"]), "branches"),
                                      (dict(branches=["center", "dim", "height", "rot"]), "branches"), (dict(dataset="nuScenes"), "classes"),
                                      (dict(heads=16), "NUM_HEADS")])
def test_family_refusals_name_the_limit(kw, word):
    """_plan() is what forward runs before any launch; it needs no GPU."""
    m = build("plain", **kw)
    with pytest.raises(F.LvqError, match=word):
        m._plan()


def test_more_refusals_of_the_family():
    c = TC.MODULE_CASES["waymo"]
    args = TC.case_args("waymo")
    args.update(num_class=2, class_names=c["class_names"][:2], model_cfg=TC.case_cfg("waymo", n_cls=2))
    with pytest.raises(F.LvqError, match="classes"):
        TH.TransFusionHead(**args)._plan()                     # Waymo mode indexes classes 1 and 2
    args = TC.case_args("plain")
    args.update(input_channels=640)
    with pytest.raises(F.LvqError, match="input channels"):
        TH.TransFusionHead(**args)._plan()
    args = TC.case_args("plain")
    args.update(num_class=65, class_names=[str(i) for i in range(65)], model_cfg=TC.case_cfg("plain", n_cls=65))
    with pytest.raises(F.LvqError, match="classes"):
        TH.TransFusionHead(**args)._plan()
    build("waymo")._plan()
    build("nusc")._plan()


# ---------------------------------------------------------------------------------------------------------------------------------
# positions
# ---------------------------------------------------------------------------------------------------------------------------------
def test_position_formula_on_a_non_square_grid():
    """bev_pos, as the reference builds it (an `ij` meshgrid over (x_size, y_size), flattened), indexed with the row-major cell and flipped,
    is (n % y_size + 0.5, n // y_size + 0.5): on 16 x 28 that is NOT (column + 0.5, row + 0.5)."""
    m = build("waymo")
    h, w = TC.MODULE_CASES["waymo"]["shape"][2:]
    assert tuple(m.bev_pos.shape) == (1, h * w, 2)
    flipped = m.bev_pos[0].flip(dims=[-1]).numpy()
    n = np.arange(h * w)
    assert np.array_equal(flipped, TC.positions(n, h).astype(np.float32))
    assert np.array_equal(TH.grid_positions(h, w).numpy(), flipped)
    naive = np.stack([n % w + 0.5, n // w + 0.5], axis=-1)
    assert not np.array_equal(flipped, naive)
    sq = build("nusc")
    n = np.arange(24 * 24)
    assert np.array_equal(sq.bev_pos[0].flip(dims=[-1]).numpy(), np.stack([n % 24 + 0.5, n // 24 + 0.5], axis=-1).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# restatement against the fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_fixture(name):
    g, ref, c = golden(name), TC.case_ref(name), TC.MODULE_CASES[name]
    assert np.array_equal(g["x"], TC.case_input(name))
    assert close(ref["dense_heatmap"], g["dense_heatmap"])
    b, p = g["query_labels"].shape
    hw = c["shape"][2] * c["shape"][3]
    # the proposal SET by (class, cell) key; the order only where the scores are more than 1e-4 apart
    gold_cls = g["query_labels"]
    gold_score = g["query_heatmap_score"][np.arange(b)[:, None], gold_cls, np.arange(p)[None, :]]
    for s in range(b):
        assert sorted(ref["query_labels"][s].tolist()) == sorted(gold_cls[s].tolist())
        order_r, order_g = np.argsort(-ref["prop_score"][s], kind="stable"), np.argsort(-gold_score[s], kind="stable")
        assert close(ref["prop_score"][s][order_r], gold_score[s][order_g])
    # rows matched by key: (class, score) identifies a proposal given the cut and local margins
    for s in range(b):
        key_r = {(int(k), round(float(v), 5)): i for i, (k, v) in enumerate(zip(ref["query_labels"][s], ref["prop_score"][s]))}
        perm = np.array([key_r[(int(k), round(float(v), 5))] for k, v in zip(gold_cls[s], gold_score[s])])
        assert sorted(perm.tolist()) == list(range(p))
        gaps = np.abs(np.diff(gold_score[s]))
        assert all(perm[i] < perm[i + 1] for i in range(p - 1) if gaps[i] > 1e-4)
        assert close(ref["query_heatmap_score"][s][:, perm], g["query_heatmap_score"][s])
        for n in TC.branch_names(c["vel"]):
            assert close(ref["raw"][n][s][:, perm], g[n][s]), n
        kept = [i for i in perm if ref["keep"][s][i]]
        assert len(kept) == len(g[f"final_{s}_scores"])
        assert close(ref["boxes"][s][kept], g[f"final_{s}_boxes"]) and close(ref["scores"][s][kept], g[f"final_{s}_scores"])
        assert np.array_equal(ref["labels"][s][kept], g[f"final_{s}_labels"]) and g[f"final_{s}_labels"].dtype == np.int32
    assert g["final_0_boxes"].shape[1] == (9 if c["vel"] else 7)
    assert ref["flat"].max() < len(c["class_names"]) * hw


@pytest.mark.parametrize("name", CASES)
def test_margin_conditions_hold(name):
    c = TC.MODULE_CASES[name]
    m = TC.case_margins(name)
    assert TC.margins_ok(m, c["p"]), m
    if name == "nusc":                             # the mask drops some rows and keeps some in each scene, for both of its reasons
        ref = TC.case_ref(name)
        assert all(0 < k < c["p"] for k in ref["keep"].sum(axis=1))
        assert (ref["scores"] <= c["score_thresh"]).any() and (ref["scores"] > c["score_thresh"]).any()
        lim = np.asarray(c["center_range"])
        inside = (ref["boxes"][..., :3] >= lim[:3]).all(-1) & (ref["boxes"][..., :3] <= lim[3:]).all(-1)
        assert (~inside).any() and inside.any()


def test_proposals_ref_rules():
    """The restatement's own rules on a hand-made map: plateau, saturated pair, border, point class, zero fill, NaN."""
    x = np.full((1, 2, 5, 7), -3.0, np.float32)
    x[0, 0, 1, 1] = x[0, 0, 1, 2] = 2.0            # a plateau: both survive
    x[0, 0, 3, 5] = 30.0
    x[0, 0, 4, 0] = 40.0                           # border of a 3 x 3 class: never
    x[0, 1, 0, 6] = 1.0                            # point class: kept on the border
    flat, score, qhs, sup = TC.proposals_ref(x, (1,), 44)
    assert sup[0, 0, 4, 0] == 0 and sup[0, 0, 3, 5] == 1.0 and sup[0, 0, 1, 1] == sup[0, 0, 1, 2] > 0 and sup[0, 0, 1, 3] == 0
    assert list(flat[0, :6]) == [26, 8, 9, 41, 11, 12]          # then the -3 plateau: interior cells of class 0 away from a peak tie with class 1's
    assert (sup[0, 1] > 0).all() and score[0, 3] > score[0, 4] > 0 and score[0, 41] > 0 and score[0, 42] == 0 and list(flat[0, 42:44]) == [0, 1]
    assert qhs.shape == (1, 2, 44) and qhs[0, 1, 0] == sup[0, 1, 3, 5] and qhs[0, 0, 3] == 0
    x[0, 0, 2, 2] = np.nan
    flat, score, _, sup = TC.proposals_ref(x, (1,), 3)
    assert flat[0, 0] == 16 and np.isnan(score[0, 0]) and sup[0, 0, 3, 5] == 1.0 and sup[0, 0, 1, 1] == 0 and flat[0, 1] == 26
