"""TransFusionHead on the MI355X: the four kernels of csrc/transfusion_head.hip against the fp64 restatements of
tests/transfusion_head_cases.py, and the module against the fixtures made from the reference's own class
(tools/make_transfusion_head_golden.py).

Bars.  Kernel outputs (fp32 arithmetic): 1e-5 * max(1, |ref|), the decode bar of the other heads; indices, labels, counts and orders exact
(the inputs keep every decision clear of rounding: exactly representable logits, condition (iii) asserted on the restatement).  Module,
bf16x3: 1e-3 * max(1, max|ref|), the project's bar.  Module, plain bf16: dense_heatmap only, at twice PLAIN_MEASURED.
"""
import os
import warnings

import numpy as np
import pytest
import torch

import transfusion_head_cases as TC
from lidar_vision_vqa_amd import _ffi as F
from lidar_vision_vqa_amd import ops
from lidar_vision_vqa_amd import transfusion_head as TH

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = list(TC.MODULE_CASES)
DEV = "cuda:0"
# max |dense_heatmap - golden| / max(1, max|golden|) of precision = "bf16", measured on an MI355X on 2026-10-21 at the fixtures' shapes
# ([2, 32, 24, 24], [2, 32, 16, 28], [1, 64, 12, 20]); the test asserts twice these
PLAIN_MEASURED = {"nusc": 3.491e-3, "waymo": 3.501e-3, "plain": 2.861e-3}


def golden(name):
    return np.load(os.path.join(GOLDEN, TC.golden_name(name)))


def close(a, ref, tol=1e-5):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    a, ref = a.astype(np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    bad = ~(np.abs(a - ref) <= tol * np.maximum(1.0, np.abs(ref)))
    both_nan = np.isnan(a) & np.isnan(ref)
    return bool(not (bad & ~both_nan).any())


def rel_err(a, ref):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    ref = np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a.astype(np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


@pytest.fixture(scope="module")
def heads():
    """One module per case on the device, fed with the case's seeded state; shared and never edited (tests that edit build their own)."""
    out = {}
    for name in CASES:
        out[name] = make_head(name)
    return out


def make_head(name, **kw):
    torch.manual_seed(0)
    m = TH.TransFusionHead(**TC.case_args(name, **kw))
    TC.load_state(m, TC.case_state(name))
    return m.to(DEV).eval()


def run(m, x):
    with torch.no_grad():
        return m(dict(spatial_features_2d=torch.as_tensor(x, device=DEV), batch_size=len(x)))["final_box_dicts"]


@pytest.fixture(scope="module")
def forwards(heads):
    """The bf16x3 forward of every case, once: (final lists, forward_ret_dict snapshot, query_labels)."""
    out = {}
    for name, m in heads.items():
        final = run(m, TC.case_input(name))
        out[name] = (final, dict(m.forward_ret_dict), m.query_labels.clone())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_heatmap_proposals
# ---------------------------------------------------------------------------------------------------------------------------------
LEVELS = np.arange(-2.0, 1.0, 0.125, dtype=np.float32)         # 24 exactly representable logits, 0.125 apart: ties everywhere, no near-ties


def level_map(shape, seed, saturated=8):
    rng = np.random.default_rng(seed)
    x = LEVELS[rng.integers(0, len(LEVELS), size=shape)]
    flat = x.reshape(-1)
    flat[rng.choice(flat.size, size=saturated, replace=False)] = np.float32(30.0)
    flat[rng.choice(flat.size, size=saturated, replace=False)] = np.float32(40.0)       # 30 and 40: both 1.0f under any sigmoid
    return x


def check_proposals(logits, point, p, c_total=None, first=0):
    b, n, h, w = logits.shape
    maps = logits
    if c_total is not None:
        maps = np.full((b, c_total, h, w), 50.0, np.float32)                            # other channels would win if they were read
        maps[:, first:first + n] = logits
    flat, score, qhs = ops.heatmap_proposals(torch.from_numpy(maps).to(DEV), first_channel=first, n_cls=n,
                                             point_class_mask=sum(1 << c for c in point), n_proposals=p)
    rf, rs, rq, _ = TC.proposals_ref(logits, point, p)
    assert flat.dtype == torch.int32 and np.array_equal(flat.cpu().numpy(), rf)
    assert close(score, rs) and close(qhs, rq)
    return flat, score, qhs


def test_proposals_channel_window_and_point_classes():
    check_proposals(level_map((2, 10, 12, 20), 1), (8, 9), 32, c_total=64, first=3)


def test_proposals_whole_grid_with_one_interior_cell():
    flat, score, _ = check_proposals(level_map((1, 3, 3, 3), 2, saturated=2), (1, 2), 27)
    assert sorted(flat[0].tolist()) == list(range(27)) and int((score[0] > 0).sum()) in (18, 19)    # class 0: its centre cell at the most


def test_proposals_full_sort_buffer():
    check_proposals(level_map((1, 10, 24, 24), 3), (8, 9), 1024)


def test_proposals_plateau_saturated_pair_border_and_nan():
    x = np.full((1, 2, 5, 7), -3.0, np.float32)
    x[0, 0, 1, 1] = x[0, 0, 1, 2] = 2.0            # a plateau: both survive
    x[0, 0, 3, 4] = 30.0
    x[0, 0, 3, 5] = 40.0                           # a saturated pair: equal in fp32, both survive, the lower index first
    x[0, 0, 4, 0] = 40.0                           # border of a 3 x 3 class: never
    x[0, 1, 0, 6] = 1.0                            # point class: kept on the border
    flat, score, qhs = check_proposals(x, (1,), 44)
    assert flat[0, :5].tolist() == [25, 26, 8, 9, 41] and float(score[0, 0]) == float(score[0, 1]) == 1.0
    assert float(score[0, 43]) == 0.0 and flat[0, 42:44].tolist() == [0, 1]            # fewer than P positives: zeros, ascending flat index
    x[0, 0, 2, 2] = np.nan
    flat, score, _ = check_proposals(x, (1,), 4)
    assert flat[0, 0].item() == 16 and bool(torch.isnan(score[0, 0])) and flat[0, 1:3].tolist() == [25, 26]


def test_proposals_fewer_positives_than_p():
    x = np.full((2, 3, 6, 6), -np.inf, np.float32)
    x[0, 0, 2, 2], x[0, 2, 3, 3], x[1, 1, 4, 1] = 0.5, 0.25, -1.0
    flat, score, _ = check_proposals(x, (), 8)
    assert flat[0].tolist() == [14, 72 + 21, 0, 1, 2, 3, 4, 5] and flat[1].tolist() == [36 + 25, 0, 1, 2, 3, 4, 5, 6]
    assert (score[:, 2:] == 0).all()


def test_proposals_refusals():
    maps = torch.zeros((1, 64, 8, 8), device=DEV)
    for kw in (dict(n_proposals=1025), dict(nms_kernel_size=1), dict(n_proposals=65 * 64, n_cls=64), dict(n_cls=65), dict(first_channel=60)):
        args = dict(first_channel=0, n_cls=10, point_class_mask=0, n_proposals=16)
        args.update(kw)
        with pytest.raises(F.LvqError):
            ops.heatmap_proposals(maps, **args)
    with pytest.raises(F.LvqError):
        ops.heatmap_proposals(torch.zeros((1, 4, 2, 8), device=DEV), first_channel=0, n_cls=4, point_class_mask=0, n_proposals=4)


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_pos_embed_learned, lvq_transfusion_queries
# ---------------------------------------------------------------------------------------------------------------------------------
def pe_operands(state, prefix, dev=DEV):
    h = prefix + ".position_embedding_head"
    scale, shift = TC.fold_bn(state, h + ".1")
    shift = TC._t(state[h + ".0.bias"]) * scale + shift
    ops_ = (state[h + ".0.weight"][:, :, 0], scale.numpy(), shift.numpy(), state[h + ".3.weight"][:, :, 0], state[h + ".3.bias"])
    return tuple(torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.float32))).to(dev) for t in ops_)


def test_pos_embed_rows_and_widths():
    state = TC.case_state("nusc")
    pos = (np.random.default_rng(5).random((13, 2)) * 30).astype(np.float32)           # 13 rows: a partial last tile
    w1, scale, shift, w2, b2 = pe_operands(state, "decoder.cross_posembed")
    out = ops.pos_embed_learned(torch.from_numpy(pos).to(DEV), w1, scale, shift, w2, b2)
    ref = TC.pos_embed_ref(state, "decoder.cross_posembed", pos.astype(np.float64)).numpy()
    assert close(out, ref)
    one = ops.pos_embed_learned(torch.from_numpy(pos[12:13]).to(DEV), w1, scale, shift, w2, b2)
    assert torch.equal(one[0], out[12])                                                 # a row's bits do not depend on its position
    w2f = torch.cat([w2, -w2[:64]]).contiguous()                                        # d_out = 192: the folded form
    wide = ops.pos_embed_learned(torch.from_numpy(pos).to(DEV), w1, scale, shift, w2f, torch.cat([b2, -b2[:64]]).contiguous())
    assert torch.equal(wide[:, :128], out) and torch.equal(wide[:, 128:], -out[:, :64])


@pytest.mark.parametrize("split", [True, False])
def test_queries_gather_class_column_positions(split):
    b, h, w, d, n_cls, p = 2, 16, 28, 128, 3, 24
    state = TC.case_state("waymo")
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.standard_normal((b, h, w, d)).astype(np.float32))
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16) if split else None
    flat = np.stack([rng.choice(n_cls * h * w, size=p, replace=False) for _ in range(b)]).astype(np.int32)
    flat[0, 0], flat[1, 1] = 0, n_cls * h * w - 1
    cw, cb = state["class_encoding.weight"][:, :, 0], state["class_encoding.bias"]
    pe = pe_operands(state, "decoder.self_posembed")

    def go(class_w, class_b):
        return ops.transfusion_queries(hi.view(torch.int16).to(DEV), None if lo is None else lo.view(torch.int16).to(DEV),
                                       torch.from_numpy(flat).to(DEV), n_cls=n_cls, y_size=h,
                                       class_w=torch.from_numpy(np.ascontiguousarray(class_w)).to(DEV), class_b=torch.from_numpy(class_b).to(DEV), pe=pe)
    feat, pos, labels, qpe = go(cw, cb)
    cls, cell = flat // (h * w), flat % (h * w)
    rows = hi.float().double() + (lo.float().double() if split else 0.0)
    rows = rows.view(b, h * w, d).numpy()[np.arange(b)[:, None], cell]
    assert close(feat, rows + cw.T.astype(np.float64)[cls] + cb.astype(np.float64))
    assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), cls)
    assert np.array_equal(pos.cpu().numpy(), TC.positions(cell, h).astype(np.float32))           # (n % 16 + 0.5, n // 16 + 0.5) on 16 x 28
    assert close(qpe, TC.pos_embed_ref(state, "decoder.self_posembed", TC.positions(cell, h)).numpy())
    bare, _, _, _ = go(np.zeros_like(cw), np.zeros_like(cb))
    fp32_rows = hi.float() + (lo.float() if split else 0.0)                             # hi + lo of the planes row, bit for bit
    assert torch.equal(bare.cpu(), fp32_rows.view(b, h * w, d)[torch.arange(b)[:, None], torch.from_numpy(cell)])


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_transfusion_tail
# ---------------------------------------------------------------------------------------------------------------------------------
def tail_case(b, p, n_cls, ffn, vel, seed, score_thresh=0.3, center_range=(-2.9, -2.9, -1.5, 2.9, 2.9, 1.5)):
    """Seeded rows, positions on an 8 x 8 map centred on the origin, labels, proposal scores -> (module, inputs, fp64 restatement)."""
    state = TC.seeded_state(TC.state_shapes(n_cls, 32, ffn, vel, False), seed)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((b, p, 128)).astype(np.float32)
    qpos = (rng.integers(0, 8, size=(b, p, 2)) + 0.5).astype(np.float32)
    labels = rng.integers(0, n_cls, size=(b, p)).astype(np.int32)
    pscore = (0.2 + 0.8 * rng.random((b, p))).astype(np.float32)
    grid, voxel = np.array([64, 64, 40]), [0.1, 0.1, 0.2]
    pc_range = np.array([-3.2, -3.2, -5.0, 3.2, 3.2, 3.0])
    ref = TC.tail_ref(state, x.astype(np.float64), qpos.astype(np.float64), labels, pscore.astype(np.float64), vel, TC.STRIDE, voxel, pc_range,
                      list(center_range), score_thresh)
    cfg = TC.head_cfg(n_cls, "KITTI", p, 8, ffn, vel, False, score_thresh, list(center_range))
    torch.manual_seed(0)
    m = TH.TransFusionHead(cfg, 32, n_cls, [str(i) for i in range(n_cls)], grid, pc_range, voxel)
    TC.load_state(m, state)
    return m, (x, qpos, labels, pscore), ref, list(center_range), score_thresh


@pytest.mark.parametrize("b, p, n_cls, ffn, vel, seed, kw", [
    (2, 40, 10, 256, True, 21, {}), (1, 1, 3, 64, False, 12, {}), (2, 40, 64, 512, True, 13, {}), (2, 40, 3, 512, False, 14, {}),
    (2, 40, 10, 64, True, 45, dict(score_thresh=2.0)),                                        # all rows masked
    (2, 40, 10, 256, False, 16, dict(score_thresh=-1.0, center_range=(-1e4, -1e4, -1e4, 1e4, 1e4, 1e4)))])       # none masked
def test_tail_against_the_restatement(b, p, n_cls, ffn, vel, seed, kw):
    m, (x, qpos, labels, pscore), ref, center_range, thresh = tail_case(b, p, n_cls, ffn, vel, seed, **kw)
    lim = np.asarray(center_range)
    xyz = ref["boxes"][..., :3]
    assert np.abs(ref["scores"] - thresh).min() >= 1e-4                                      # condition (iii) for these inputs
    assert min(np.abs(xyz - lim[:3]).min(), np.abs(xyz - lim[3:]).min()) >= 1e-2
    m = m.to(DEV).eval()
    t = lambda a: torch.from_numpy(a).to(DEV)
    raw, boxes, scores, out_labels, counts = ops.transfusion_tail(t(x), t(qpos), t(labels), t(pscore), **m.tail_args())
    names = TC.branch_names(vel)
    ref_raw = np.concatenate([ref["raw"][n] for n in names], axis=1)
    assert tuple(raw.shape) == (b, (10 if vel else 8) + n_cls, p) and close(raw, ref_raw)
    keep = ref["keep"]
    assert counts.dtype == torch.int32 and counts.cpu().tolist() == keep.sum(axis=1).tolist()
    assert out_labels.dtype == torch.int32 and tuple(boxes.shape) == (b, p, 9 if vel else 7)
    for s in range(b):
        n = int(keep[s].sum())
        assert close(boxes[s, :n], ref["boxes"][s][keep[s]]) and close(scores[s, :n], ref["scores"][s][keep[s]])      # proposal order kept
        assert np.array_equal(out_labels[s, :n].cpu().numpy(), ref["labels"][s][keep[s]])
        assert not boxes[s, n:].any() and not scores[s, n:].any() and not out_labels[s, n:].any()                     # zeros behind the count
    if "score_thresh" in kw:
        assert counts.cpu().tolist() == ([0] * b if kw["score_thresh"] > 1 else [p] * b)
    # a row's bits do not depend on its position or on the other scene
    raw1, boxes1, scores1, _, counts1 = ops.transfusion_tail(t(x[-1:, -1:]), t(qpos[-1:, -1:]), t(labels[-1:, -1:]), t(pscore[-1:, -1:]),
                                                             **m.tail_args())
    assert torch.equal(raw1[0, :, 0], raw[-1, :, -1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the module against the fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
def golden_rows(g, ref, s):
    """perm with golden proposal j of scene s = restatement proposal perm[j], by (class, heat): the CPU suite checks the match is one to one."""
    p = g["query_labels"].shape[1]
    gold_score = g["query_heatmap_score"][s][g["query_labels"][s], np.arange(p)]
    key = {(int(k), round(float(v), 5)): i for i, (k, v) in enumerate(zip(ref["query_labels"][s], ref["prop_score"][s]))}
    return np.array([key[(int(k), round(float(v), 5))] for k, v in zip(g["query_labels"][s], gold_score)])


@pytest.mark.parametrize("name", CASES)
def test_module_bf16x3_against_the_fixture(name, forwards):
    g, ref, c = golden(name), TC.case_ref(name), TC.MODULE_CASES[name]
    final, ret, qlab = forwards[name]
    b, p = g["query_labels"].shape
    hw = c["shape"][2] * c["shape"][3]
    err = {"dense_heatmap": rel_err(ret["dense_heatmap"], g["dense_heatmap"])}
    assert qlab.dtype == torch.int64 and tuple(qlab.shape) == (b, p)
    # the proposal set by (class, cell): the restatement's flat indices, which the CPU suite holds to the fixture
    flat_gpu = ret["top_proposals"].cpu().numpy()
    assert np.array_equal(flat_gpu // hw, qlab.cpu().numpy())
    for s in range(b):
        assert sorted(flat_gpu[s].tolist()) == sorted(ref["flat"][s].tolist())            # the proposal set is equal
        where = {int(f): i for i, f in enumerate(flat_gpu[s])}
        at = np.array([where[int(f)] for f in ref["flat"][s]])                             # restatement row r sits at GPU row at[r]
        gaps = np.abs(np.diff(ref["prop_score"][s]))
        assert all(at[i] < at[i + 1] for i in range(p - 1) if gaps[i] > 1e-4)              # descending wherever the gap is clear
        perm = golden_rows(g, ref, s)                                                      # golden j = restatement row perm[j]
        rows = at[perm]                                                                    # ... = GPU row rows[j]
        for n in TC.branch_names(c["vel"]) + ["query_heatmap_score"]:
            e = rel_err(ret[n][s].cpu().numpy()[:, rows], g[n][s])
            err[n] = max(err.get(n, 0.0), e)
        # final lists one to one by key: kept golden rows, in GPU proposal order
        kept_gold = [j for j in range(p) if ref["keep"][s][perm[j]]]
        assert len(final[s]["pred_scores"]) == len(g[f"final_{s}_scores"]) == len(kept_gold)
        gpu_order = sorted(kept_gold, key=lambda j: rows[j])                              # the GPU compacts in ITS proposal order
        pos_in_gold = [kept_gold.index(j) for j in gpu_order]
        err["boxes"] = max(err.get("boxes", 0.0), rel_err(final[s]["pred_boxes"], g[f"final_{s}_boxes"][pos_in_gold]))
        err["scores"] = max(err.get("scores", 0.0), rel_err(final[s]["pred_scores"], g[f"final_{s}_scores"][pos_in_gold]))
        assert final[s]["pred_labels"].dtype == torch.int32
        assert np.array_equal(final[s]["pred_labels"].cpu().numpy(), g[f"final_{s}_labels"][pos_in_gold])
    print(f"transfusion_head {name} bf16x3 errors: " + " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    assert max(err.values()) <= 1e-3, err
    assert tuple(ret["dense_heatmap"].shape) == g["dense_heatmap"].shape


@pytest.mark.parametrize("name", CASES)
def test_module_plain_bf16_dense_outputs(name):
    g = golden(name)
    m = make_head(name)
    m.precision = "bf16"
    run(m, TC.case_input(name))
    e = rel_err(m.forward_ret_dict["dense_heatmap"], g["dense_heatmap"])
    print(f"transfusion_head {name} plain bf16 dense_heatmap error: {e:.3e}")
    assert e <= 2 * PLAIN_MEASURED[name]


def lists_equal(a, b):
    return len(a) == len(b) and all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("pred_boxes", "pred_scores", "pred_labels"))


@pytest.mark.parametrize("name", CASES)
def test_torch_op_switch_gives_the_same_lists(name, heads, forwards, monkeypatch):
    monkeypatch.setenv("LVQ_HEAD_TORCH_POST", "1")
    final = run(heads[name], TC.case_input(name))
    ours = forwards[name][0]
    assert [len(d["pred_scores"]) for d in final] == [len(d["pred_scores"]) for d in ours]
    for a, b in zip(final, ours):
        assert torch.equal(a["pred_labels"], b["pred_labels"]) and a["pred_labels"].dtype == torch.int32
        assert close(a["pred_boxes"], b["pred_boxes"].cpu().numpy()) and close(a["pred_scores"], b["pred_scores"].cpu().numpy())


def test_run_to_run_and_batch_composition_bit_identity(heads, forwards):
    m, x = heads["nusc"], TC.case_input("nusc")
    again = run(m, x)
    assert lists_equal(again, forwards["nusc"][0])
    ret_pair = {k: v.clone() for k, v in m.forward_ret_dict.items()}
    alone = run(m, x[1:2])
    assert lists_equal(alone, again[1:2])                                                # scene 1 alone = scene 1 of the pair
    for k, v in m.forward_ret_dict.items():
        assert torch.equal(v[0], ret_pair[k][1]), k


def test_weight_edit_and_second_map_size_are_seen():
    m, x = make_head("plain"), TC.case_input("plain")
    first = run(m, x)
    heat0 = m.forward_ret_dict["heatmap"].clone()
    with torch.no_grad():
        m.decoder.cross_posembed.position_embedding_head[3].weight.mul_(1.5)               # only the folded key table sees this one
    run(m, x)
    assert not torch.equal(m.forward_ret_dict["heatmap"], heat0)
    with torch.no_grad():
        m.decoder.cross_posembed.position_embedding_head[3].weight.div_(1.5)
        m.prediction_head.height[1].bias.add_(0.25)
    third = run(m, x)
    assert close(third[0]["pred_boxes"][:, 2], first[0]["pred_boxes"][:, 2].cpu().numpy() + 0.25, tol=1e-4)
    # a second (H, W) through the same module: its own key table; then the first again, bit for bit
    small = run(m, np.ascontiguousarray(x[:, :, :10, :14]))
    assert len(small) == 1 and tuple(m.forward_ret_dict["dense_heatmap"].shape[2:]) == (10, 14)
    assert lists_equal(run(m, x), third)


def test_one_device_to_host_copy_per_forward(heads):
    m, x = heads["waymo"], torch.from_numpy(TC.case_input("waymo")).to(DEV)
    with torch.no_grad():
        m(dict(spatial_features_2d=x, batch_size=2))                                       # warm: workspaces, tables, packed weights
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                m(dict(spatial_features_2d=x, batch_size=2))
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in seen if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, [str(w.message) for w in syncs]


def test_train_mode_and_grad_refusals(heads):
    m = make_head("plain")
    x = torch.from_numpy(TC.case_input("plain")).to(DEV)
    with pytest.raises(F.LvqError, match="inference-only"):
        m(dict(spatial_features_2d=x, batch_size=1))                                       # grad mode with trainable parameters
    m.train()
    with pytest.raises(F.LvqError, match="inference-only"), torch.no_grad():
        m(dict(spatial_features_2d=x, batch_size=1))
    m.eval()
    m.precision = "fp8"
    with pytest.raises(F.LvqError, match="bf16x3"), torch.no_grad():
        m(dict(spatial_features_2d=x, batch_size=1))
    m.precision = None
    with pytest.raises(F.LvqError, match="proposals"), torch.no_grad():
        m(dict(spatial_features_2d=x[:, :, :2], batch_size=1))                            # H < 3


@pytest.mark.parametrize("kw, word", [(dict(ffn=96), "FFN_CHANNEL"), (dict(activation="gelu"), "ACTIVATION"), (dict(heads=16), "NUM_HEADS"),
                                      (dict(p=1025), "NUM_PROPOSALS"), (dict(nms_kernel=1), "NMS_KERNEL_SIZE"), (dict(hm_conv=3), "num_conv")])
def test_family_refusals_come_before_any_launch(kw, word):
    torch.manual_seed(0)
    m = TH.TransFusionHead(**TC.case_args("plain", **kw)).to(DEV).eval()
    x = torch.from_numpy(TC.case_input("plain")).to(DEV)
    with pytest.raises(F.LvqError, match=word), torch.no_grad():
        m(dict(spatial_features_2d=x, batch_size=1))
    assert not m.forward_ret_dict
