"""VoxelNeXtHead on the MI355X (lidar-vision-vqa_amd/sparse_head.py on csrc/sparse_head.hip and csrc/center_head.hip) against the fp64
restatements of tests/voxelnext_head_cases.py and the goldens of the unmodified reference class (tests/golden/voxelnext_head_*.npz).

  lvq_sparse_head   N in {1, 63, 64, 65, 200} x k_vol {1 (NULL table), 9} with one, three and six tasks against an fp64 dictionary form;
                    tables carry -1 and out-of-range entries; bf16x3 within 1e-3 max(1, max|ref|); plain bf16 as a regression guard at twice
                    PLAIN_MEASURED; unowned channels exact zeros; row permutation, batch composition and run-to-run bit-identity
  lvq_voxel_decode  order, labels and counts exact, boxes and scores within 1e-5 relative (the bar of test_decode_against_the_restatement):
                    interleaved scenes, an empty scene, n_b < K, n_cls * n_b < K, ties across the K-th place, a NaN, K = 1 and 1024, b = batch
  module            per golden case: branch outputs within the bar, final lists equal in count, order and labels, LVQ_HEAD_TORCH_POST=1 the
                    same lists, strict=True load; the refusals
  chain             VoxelResBackBone8xVoxelNeXt -> VoxelNeXtHead on one batch_dict, bit-identical run to run
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sparse_conv_cases as SC  # noqa: E402
import voxelnext_head_cases as VC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import backbone3d as B3  # noqa: E402
from lidar_vision_vqa_amd import ops  # noqa: E402
from lidar_vision_vqa_amd import sparse_head as SH  # noqa: E402
from lidar_vision_vqa_amd import synth  # noqa: E402

DEV = "cuda:0"
BAR = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C, TASK_C = 128, 16
# max |out - fp64| / max(1, max|fp64|) in the plain bf16 form, measured on the MI355X 2026-10-20: lvq_sparse_head over the kernel cases
# below per k_vol, and the module's branch outputs per golden case (bf16x3 on the same: kernel cases 2.3e-6 .. 5.2e-6, nusc 8.07e-6, k3
# 4.76e-6).  nc1 has num_conv = 1: its only conv is the fp32 fmaf chain, so both forms give the same bits and the figure is fp32 rounding.
PLAIN_MEASURED = {"kvol1": 2.10e-3, "kvol9": 2.14e-3, "nusc": 3.85e-3, "k3": 2.82e-3, "nc1": 3.73e-7}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_sparse_head
# ---------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = [[2, 1, 3, 2, 2, 1], [2, 1, 3, 2, 3], [4, 1], [2, 1, 3, 2, 2, 2], [1], [2, 1, 3, 2, 2, 2, 1, 3]]      # widths per branch; 6, 5, 2, 6, 1, 8 branches
SIZES = [(1, 1, 1), (63, 1, 3), (64, 1, 6), (65, 1, 1), (200, 1, 6), (1, 9, 3), (63, 9, 6), (64, 9, 1), (65, 9, 3), (200, 9, 6)]


@functools.lru_cache(maxsize=None)
def head_case(n, kvol, n_tasks, seed=11):
    """Operands of one lvq_sparse_head call and its fp64 result [16 T, n] (voxelnext_head_cases.sparse_head_case, seeded per size)."""
    return VC.sparse_head_case(np.random.default_rng([seed, n, kvol, n_tasks]), LAYOUTS[:n_tasks], n, kvol)


def pack(w1, split):
    """[T, BS, C_out, K, C_in] fp32 -> packed hi (+ lo) [T, BS, K * 128 * 128] int16 through lvq_sparse_conv_pack_weights"""
    n_tasks, bs, _, kvol, _ = w1.shape
    hi = torch.zeros((n_tasks, bs, kvol * C * C), dtype=torch.int16, device=DEV)
    lo = torch.zeros_like(hi) if split else None
    for i in range(n_tasks):
        for j in range(bs):
            w = dev(w1[i, j])
            F.check(F.lib().lvq_sparse_conv_pack_weights(F.ptr(w), C, kvol, C, F.ptr(hi[i, j]), F.ptr(lo[i, j]) if split else F.ptr(None),
                                                         F.stream_ptr(torch.device(DEV))), "lvq_sparse_conv_pack_weights")
    return hi, lo


def run_head(c, split=True, feat=None, nbr=None):
    hi, lo = pack(c["w1"], split)
    feat = c["feat"] if feat is None else feat
    nbr = c["nbr"] if nbr is None else nbr
    kvol = c["w1"].shape[3]
    return ops.sparse_head(dev(feat), None if nbr is None else dev(nbr, np.int32), k_vol=kvol, task_n_br=c["n_br"], chan_owner=c["owner"],
                           num_conv=2, br_stride=c["bs"], w_hi=hi, w_lo=lo, scale=dev(c["scale"]), shift=dev(c["shift"]),
                           w_last=dev(c["w_last"]), bias=dev(c["bias"]))


def rel_err(got, ref):
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("n, kvol, n_tasks", SIZES)
def test_sparse_head_bf16x3_meets_the_parity_bar(n, kvol, n_tasks):
    c = head_case(n, kvol, n_tasks)
    out = run_head(c)
    got = out.cpu().numpy()
    err = rel_err(got, c["ref"])
    print(f"N={n} k_vol={kvol} tasks={n_tasks} bf16x3: {err:.3e} (max|ref| {np.abs(c['ref']).max():.2f})")
    assert got.shape == (TASK_C * n_tasks, n) and err <= BAR
    unowned = [TASK_C * ti + ch for ti, o in enumerate(c["owner"]) for ch, b in enumerate(o) if b < 0]
    assert unowned and not got[unowned].any()                                    # exact zeros
    assert torch.equal(out, run_head(c))                                         # two runs give the same bits


@pytest.mark.parametrize("kvol", [1, 9])
def test_sparse_head_plain_bf16_regression_guard(kvol):
    """The plain bf16 form has no bar known in advance: PLAIN_MEASURED holds the error measured on the MI355X, the test asserts twice that."""
    errs = []
    for n, kv, n_tasks in SIZES:
        if kv == kvol:
            c = head_case(n, kv, n_tasks)
            errs.append(rel_err(run_head(c, split=False).cpu().numpy(), c["ref"]))
    print(f"k_vol={kvol} bf16: {' '.join(f'{e:.3e}' for e in errs)}; max {max(errs):.3e}")
    assert PLAIN_MEASURED[f"kvol{kvol}"] is not None and max(errs) <= 2 * PLAIN_MEASURED[f"kvol{kvol}"], max(errs)


@pytest.mark.parametrize("kvol", [1, 9])
def test_sparse_head_row_permutation_permutes_the_bits(kvol):
    n = 200
    c = head_case(n, kvol, 6)
    base = run_head(c).cpu().numpy()
    p = np.random.default_rng(3).permutation(n)                                  # new row j holds old row p[j]
    inv = np.empty(n, np.int64)
    inv[p] = np.arange(n)
    nbr = None
    if kvol == 9:
        old = c["nbr"][p].astype(np.int64)
        nbr = np.where((old >= 0) & (old < n), inv[np.clip(old, 0, n - 1)], old).astype(np.int32)
    got = run_head(c, feat=c["feat"][p], nbr=nbr).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), base[:, p].view(np.uint32))


def test_sparse_head_num_conv_1_and_argument_errors():
    c = head_case(65, 1, 3)
    out = ops.sparse_head(dev(c["feat"]), None, k_vol=1, task_n_br=c["n_br"], chan_owner=c["owner"], num_conv=1, br_stride=c["bs"], w_hi=None,
                          w_lo=None, scale=None, shift=None, w_last=dev(c["w_last"]), bias=dev(c["bias"])).cpu().numpy()
    ref = np.einsum("nk,tck->tcn", c["feat"].astype(np.float64), c["w_last"].astype(np.float64)) + c["bias"][:, :, None]
    ref[np.array(c["owner"]) < 0] = 0.0
    assert rel_err(out, ref.reshape(-1, 65)) <= 1e-5 and not out[np.array(c["owner"]).reshape(-1) < 0].any()       # fp32 fmaf chain
    with pytest.raises(F.LvqError):
        ops.sparse_head(dev(c["feat"][:, :64]), None, k_vol=1, task_n_br=c["n_br"], chan_owner=c["owner"], num_conv=1, br_stride=c["bs"],
                        w_hi=None, w_lo=None, scale=None, shift=None, w_last=dev(c["w_last"]), bias=dev(c["bias"]))
    with pytest.raises(F.LvqError):
        ops.sparse_head(t(c["feat"]), None, k_vol=1, task_n_br=c["n_br"], chan_owner=c["owner"], num_conv=1, br_stride=c["bs"],
                        w_hi=None, w_lo=None, scale=None, shift=None, w_last=dev(c["w_last"]), bias=dev(c["bias"]))      # a CPU tensor


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_voxel_decode
# ---------------------------------------------------------------------------------------------------------------------------------
WIDE = [-1e3, -1e3, -1e3, 1e3, 1e3, 1e3]
CUT = [-2.8, -10.0, -10.0, 2.8, 10.0, 10.0]                                      # an 8 x 8 grid of 0.8 m cells spans +-3.2 m
NAMES = VC.DECODE_NAMES


def rows_case(n_rows, n_cls, vel, seed, grid=8, interleave=True, extra_b=None):
    """Scenes with n_rows[s] rows each on a grid x grid map, interleaved; extra_b: rows with that batch index appended in between."""
    rng = np.random.default_rng(seed)
    extra = [(extra_b, 1, 1), (extra_b, 2, 5), (-1, 3, 3)] if extra_b is not None else []
    idx = VC.scene_rows(rng, n_rows, grid, extra, interleave)
    return idx, VC.task_rows(rng, len(idx), n_cls, vel)


def head_buffer(task, n_cls):
    """one task's rows -> (channel-major [16, N] buffer, task_channels row)"""
    buf, chans = VC.head_buffer([task])
    return buf, chans[0]


def check_decode_tasks(idx, tasks, batch, k, thresh, limit, ids, stride=4, voxel=(0.2, 0.2), origin=(-3.2, -3.2), margins=True):
    """ONE lvq_voxel_decode over all `tasks` (ids: per task its class ids) against decode_ref per task: counts, labels and order exact,
    scores and boxes within 1e-5 relative, rows behind a count zeros.  -> ([task][scene] rows seen, [task][scene] decode_ref dicts)."""
    buf, chans = VC.head_buffer(tasks)
    dim = 9 if "vel" in tasks[0] else 7
    n_cls = [t["hm"].shape[1] for t in tasks]
    boxes, scores, labels, counts = ops.voxel_decode(dev(buf), dev(idx, np.int32), batch, chans, n_cls, [c for row in ids for c in row], k=k,
                                                     box_dim=dim, stride=stride, voxel_xy=list(voxel), range_xy=list(origin), limit_range=limit,
                                                     score_thresh=thresh)
    boxes, scores, labels, counts = boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy()
    assert boxes.shape == (batch, len(tasks), k, dim) and counts.shape == (batch, len(tasks))
    seen, refs = [], []
    for t, task in enumerate(tasks):
        ref = VC.decode_ref(task, idx, batch, k, stride, voxel, origin, limit, thresh, ids[t])
        seen.append([])
        refs.append(ref)
        for s, d in enumerate(ref):
            if margins and len(d["cand_scores"]):
                distinct, _, near_thresh, near_limit = VC.decode_margins(d, min(k, len(d["cand_boxes"])), limit, thresh)
                assert distinct >= 4 and near_thresh >= 1e-4 and near_limit >= 1e-3, (t, s, distinct, near_thresh, near_limit)
            n = len(d["scores"])
            seen[t].append(n)
            assert counts[s, t] == n, (t, s, counts[s, t], n)
            assert np.array_equal(labels[s, t, :n], d["labels"]), (t, s)
            if n:
                ok = ~np.isnan(d["scores"])
                assert np.array_equal(np.isnan(scores[s, t, :n]), ~ok)
                rel_s = np.abs(scores[s, t, :n] - d["scores"])[ok] / d["scores"][ok]
                scale = np.maximum(np.abs(d["boxes"]), 1e-2)
                scale[:, 0], scale[:, 1] = np.maximum(scale[:, 0], abs(origin[0])), np.maximum(scale[:, 1], abs(origin[1]))
                rel_b = np.abs(boxes[s, t, :n] - d["boxes"]) / scale
                print(f"task {t} scene {s}: {n} of {k} (n_b {d['n_b']}); scores {rel_s.max(initial=0):.2e}, boxes {rel_b.max():.2e}")
                assert rel_s.max(initial=0) <= 1e-5 and rel_b.max() <= 1e-5
            assert not boxes[s, t, n:].any() and not scores[s, t, n:].any() and not labels[s, t, n:].any()      # rows behind the count are zeros
    return seen, refs


def check_decode(idx, task, batch, k, thresh, limit, ids, stride=4, voxel=(0.2, 0.2), origin=(-3.2, -3.2), margins=True):
    seen, refs = check_decode_tasks(idx, [task], batch, k, thresh, limit, [ids], stride, voxel, origin, margins)
    return seen[0], refs[0]


def test_decode_interleaved_scenes():
    idx, task = rows_case((60, 50), 2, True, 31)
    seen, _ = check_decode(idx, task, 2, 32, 0.1, CUT, [3, 7])
    assert all(0 < n < 32 for n in seen)                                         # the score threshold and the limit range both cut


def test_decode_an_empty_scene_and_foreign_rows():
    """Scene 1 of 3 has no rows (count 0, nothing read); rows with b = batch and b = -1 take no part."""
    idx, task = rows_case((40, 0, 45), 2, False, 32, extra_b=3)
    assert (idx[:, 0] == 3).sum() == 2 and (idx[:, 0] == -1).sum() == 1
    task["hm"][idx[:, 0] == 3] = 9.0                                             # they would win every scene's top-K
    task["hm"][idx[:, 0] == -1] = 9.0
    seen, ref = check_decode(idx, task, 3, 16, 0.1, WIDE, [0, 1])
    assert seen[1] == 0 and seen[0] > 0 and seen[2] > 0 and ref[1]["n_b"] == 0
    assert all(s["scores"].max() < 0.9 for s in (ref[0], ref[2]))


def test_decode_fewer_rows_than_k():
    """n_b < K (scene 0: 20 rows, 60 pairs) and n_cls * n_b < K (scene 1: 5 rows, 15 pairs): the class is the matrix row."""
    idx, task = rows_case((20, 5), 3, False, 5)
    seen, ref = check_decode(idx, task, 2, 32, None, WIDE, [4, 5, 6])
    assert seen == [32, 15] and set(ref[1]["labels"].tolist()) == {4, 5, 6}
    buf, chans = head_buffer(task, 3)
    empty = ops.voxel_decode(dev(buf[:, :0]), dev(idx[:0], np.int32), 2, [chans], [3], [4, 5, 6], k=8, box_dim=7, stride=4, voxel_xy=[0.2, 0.2],
                             range_xy=[0.0, 0.0], limit_range=WIDE, score_thresh=None)
    assert not empty[3].any() and not empty[0].any()                             # no rows at all


def test_decode_ties_take_the_lower_class_and_row():
    """A block of equal scores across the K-th place: 12 candidates above it, then 40 equal ones for 20 places."""
    idx, task = rows_case((50, 40), 2, False, 33)
    rng = np.random.default_rng(34)
    rows0 = np.nonzero(idx[:, 0] == 0)[0]
    task["hm"][rows0] = rng.uniform(-6.0, -3.0, (len(rows0), 2)).astype(np.float32)
    pairs = rng.permutation(2 * len(rows0))
    high, plateau = pairs[:12], pairs[12:52]
    task["hm"][rows0[high % len(rows0)], high // len(rows0)] = np.linspace(1.0, 2.1, 12).astype(np.float32)
    task["hm"][rows0[plateau % len(rows0)], plateau // len(rows0)] = 0.5
    seen, ref = check_decode(idx, task, 2, 32, 0.1, WIDE, [0, 1], margins=False)
    assert seen[0] == 32
    tied = ref[0]["flat"][12:]
    want = np.sort((plateau // len(rows0)) * len(idx) + rows0[plateau % len(rows0)])[:20]
    assert np.array_equal(tied, want) and np.all(ref[0]["scores"][12:] == ref[0]["scores"][12])


@pytest.mark.parametrize("thresh", [0.1, None])
def test_decode_one_nan_score(thresh):
    """A NaN sorts first, as torch.topk has it; it fails `score > thresh` and is kept when there is no threshold."""
    idx, task = rows_case((60, 50), 2, True, 35)
    row = np.nonzero(idx[:, 0] == 1)[0][7]
    task["hm"][row, 1] = np.float32(np.nan)
    seen, ref = check_decode(idx, task, 2, 16, thresh, WIDE, [2, 5], margins=False)
    if thresh is None:
        assert seen == [16, 16] and np.isnan(ref[1]["scores"][0]) and ref[1]["labels"][0] == 5 and ref[1]["rows"][0] == row
    else:
        assert not np.isnan(ref[1]["scores"]).any() and seen[1] < 16


@pytest.mark.parametrize("k, n_rows", [(1, (30, 1)), (1024, (700, 600))])
def test_decode_k_sizes(k, n_rows):
    idx, task = rows_case(n_rows, 2, False, 36 + k, grid=32)
    seen, _ = check_decode(idx, task, 2, k, None, WIDE, [0, 1], stride=1, voxel=(0.2, 0.2), origin=(-3.2, -3.2), margins=(k == 1))
    assert seen == [min(k, 2 * n) for n in n_rows]


# ---------------------------------------------------------------------------------------------------------------------------------
# module
# ---------------------------------------------------------------------------------------------------------------------------------
def build(name, cfg=None, **kw):
    c = VC.CASES[name]
    return SH.dense_heads_all["VoxelNeXtHead"](VC.case_cfg(name) if cfg is None else cfg, kw.pop("input_channels", VC.C), len(c["class_names"]),
                                               c["class_names"], np.array(c["grid_size"]), c["point_cloud_range"], c["voxel_size"], **kw)


@functools.lru_cache(maxsize=None)
def model(name):
    m = build(name)
    m.load_state_dict({k: t(v) for k, v in VC.case_state(name).items()}, strict=True)
    return m.to(DEV).eval()


def tensor(name, feats=None, idx=None, batch=2, **kw):
    f0, i0 = VC.case_input(name)
    feats, idx = f0 if feats is None else feats, i0 if idx is None else idx
    return B3.SparseConvTensor(t(feats).to(DEV), t(idx).to(DEV), list(VC.CASES[name]["grid"]), batch, **kw)


def run(m, x, mode="bf16x3", batch=2):
    m.precision = mode
    with torch.no_grad():
        out = m(dict(encoded_spconv_tensor=x, batch_size=batch))
    return out, m.forward_ret_dict["pred_dicts"]


def rows_err(pred, ref):
    return max(rel_err(pred[i][n].cpu().numpy(), np.asarray(ref[i][n])) for i in range(len(ref)) for n in ref[i])


def golden(name):
    z = np.load(os.path.join(GOLDEN, VC.golden_name(name)))
    cfg = VC.case_cfg(name)
    rows = [{n: z[f"rows_{i}_{n}"] for n in VC.branch_names(cfg)} for i in range(len(cfg.CLASS_NAMES_EACH_HEAD))]
    final = [{k: z[f"final_{s}_{k}"] for k in ("boxes", "scores", "labels")} for s in range(2)]
    return z, rows, final


def check_lists(got, want, n_tasks):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        gb, gs, gl = g["pred_boxes"].cpu().numpy(), g["pred_scores"].cpu().numpy(), g["pred_labels"].cpu().numpy()
        assert gl.dtype == np.int64 and gb.shape == w["boxes"].shape and np.array_equal(gl, w["labels"]), s
        err = max(float(np.abs(gb - w["boxes"]).max()) / max(1.0, float(np.abs(w["boxes"]).max())), float(np.abs(gs - w["scores"]).max()))
        print(f"scene {s}: {len(gl)} boxes, max error {err:.3e}")
        assert err <= BAR and g["pred_ious"] == [None] * n_tasks


@pytest.mark.parametrize("name", list(VC.CASES))
def test_module_bf16x3_reproduces_the_reference_class(name):
    z, rows, final = golden(name)
    m = model(name)
    assert list(m.state_dict()) == list(z["keys"])                               # the strict=True load above took the golden's keys
    out, pred = run(m, tensor(name))
    err = rows_err(pred, rows)
    print(f"{name} bf16x3 rows: vs golden {err:.3e}, vs fp64 restatement {rows_err(pred, VC.case_ref(name)[0]):.3e}")
    assert err <= BAR
    n_tasks = len(pred)
    check_lists(out["final_box_dicts"], final, n_tasks)
    assert "rois" not in out and all(tuple(pred[i][n].shape) == rows[i][n].shape for i in range(n_tasks) for n in rows[i])
    assert torch.equal(m.forward_ret_dict["voxel_indices"].cpu(), t(z["indices"])) and torch.equal(m.forward_ret_dict["batch_index"].cpu(), t(z["indices"][:, 0]))
    # int64 indices are cast; precision None follows the tensor's
    m.precision = None
    f, i = VC.case_input(name)
    with torch.no_grad():
        out2 = m(dict(encoded_spconv_tensor=tensor(name, idx=i.astype(np.int64), precision="bf16x3"), batch_size=2))
    for a, b in zip(out["final_box_dicts"], out2["final_box_dicts"]):
        assert torch.equal(a["pred_boxes"], b["pred_boxes"]) and torch.equal(a["pred_labels"], b["pred_labels"])


@pytest.mark.parametrize("name", list(VC.CASES))
def test_module_plain_bf16_regression_guard(name):
    err = rows_err(run(model(name), tensor(name), "bf16")[1], VC.case_ref(name)[0])
    print(f"{name} bf16 rows: vs fp64 restatement {err:.3e}")
    assert PLAIN_MEASURED[name] is not None and err <= 2 * PLAIN_MEASURED[name], err


@pytest.mark.parametrize("name", list(VC.CASES))
def test_torch_post_route_gives_the_same_lists(name, monkeypatch):
    _, rows, final = golden(name)
    monkeypatch.setenv("LVQ_HEAD_TORCH_POST", "1")
    check_lists(run(model(name), tensor(name))[0]["final_box_dicts"], final, len(rows))


def test_a_scene_carries_the_same_bits_alone_and_as_scene_1_of_2():
    """k3 (3 x 3 branch convs; the seam rows of the two scenes share their cells): scene 1's rows alone, as scene 0 of a batch of one."""
    name = "k3"
    m = model(name)
    feats, idx = VC.case_input(name)
    _, both = run(m, tensor(name))
    both = [{k: v.clone() for k, v in p.items()} for p in both]
    sel = idx[:, 0] == 1
    alone_idx = idx[sel].copy()
    alone_idx[:, 0] = 0
    out, alone = run(m, tensor(name, feats[sel], alone_idx, batch=1), batch=1)
    sel_t = t(sel).to(DEV)
    for a, b in zip(both, alone):
        assert all(torch.equal(a[k][sel_t], b[k]) for k in a)
    assert len(out["final_box_dicts"]) == 1
    out2, _ = run(m, tensor(name))
    assert torch.equal(out["final_box_dicts"][0]["pred_boxes"], out2["final_box_dicts"][1]["pred_boxes"])


def test_rois_for_refining():
    name = "nc1"
    m = build(name, predict_boxes_when_training=True)
    m.load_state_dict(model(name).state_dict(), strict=True)
    out, _ = run(m.to(DEV).eval(), tensor(name))
    lists = out["final_box_dicts"]
    n = max(len(d["pred_scores"]) for d in lists)
    assert out["has_class_labels"] is True and tuple(out["rois"].shape) == (2, n, 7) and out["roi_labels"].dtype == torch.int64
    for s, d in enumerate(lists):
        k = len(d["pred_scores"])
        assert torch.equal(out["rois"][s, :k], d["pred_boxes"]) and torch.equal(out["roi_labels"][s, :k], d["pred_labels"])


def test_unsupported_configurations_raise():
    name = "nusc"

    def call(m, x=None):
        with torch.no_grad():
            return m(dict(encoded_spconv_tensor=tensor(name) if x is None else x, batch_size=2))

    m = build(name).to(DEV)
    with pytest.raises(F.LvqError, match="eval"):
        call(m)                                                                 # train() mode
    m.eval()
    x = tensor(name)
    x.features.requires_grad_(True)
    with pytest.raises(F.LvqError, match="eval"):
        m(dict(encoded_spconv_tensor=x, batch_size=2))                          # a requires_grad input
    for method in (m.assign_targets, m.get_loss):
        with pytest.raises(F.LvqError, match="out of scope"):
            method()
    m.precision = "fp8"
    with pytest.raises(F.LvqError):
        call(m)
    for key in ("IOU_BRANCH", "DOUBLE_FLIP"):
        cfg = VC.case_cfg(name)
        cfg[key] = True
        with pytest.raises(F.LvqError, match=key):
            call(build(name, cfg).to(DEV).eval())
    cfg = VC.case_cfg(name)
    cfg["SHARED_CONV_CHANNEL"] = 64
    with pytest.raises(F.LvqError, match="SHARED_CONV_CHANNEL"):
        call(build(name, cfg, input_channels=64).to(DEV).eval())
    for key, val, match in (("KERNEL_SIZE_HEAD", 5, "KERNEL_SIZE_HEAD"), ("NUM_HM_CONV", 1, "num_conv")):
        cfg = VC.case_cfg(name)
        cfg[key] = val
        with pytest.raises(F.LvqError, match=match):
            call(build(name, cfg).to(DEV).eval())
    cfg = VC.case_cfg(name)
    cfg.POST_PROCESSING.NMS_CONFIG["NMS_TYPE"] = "circle_nms"
    with pytest.raises(F.LvqError, match="circle_nms"):
        call(build(name, cfg).to(DEV).eval())
    cfg = VC.case_cfg(name)
    cfg.POST_PROCESSING["MAX_OBJ_PER_SAMPLE"] = 1025
    with pytest.raises(F.LvqError, match="MAX_OBJ_PER_SAMPLE"):
        call(build(name, cfg).to(DEV).eval())
    f, i = VC.case_input(name)
    with pytest.raises(F.LvqError):
        call(model(name), tensor(name, f[:, :64].copy(), i))                    # 64 channels
    with pytest.raises(F.LvqError):
        build(name).eval()(dict(encoded_spconv_tensor=B3.SparseConvTensor(t(f), t(i), [16, 16], 2), batch_size=2))      # no CPU fallback


# ---------------------------------------------------------------------------------------------------------------------------------
# chain
# ---------------------------------------------------------------------------------------------------------------------------------
def test_backbone_to_head_on_one_batch_dict_and_determinism():
    """bb_mid of tests/sparse_conv_cases.py: grid (88, 72, 16), three scenes of which scene 1 is empty -> an 11 x 9 BEV tensor at stride 8."""
    idx, _, batch = SC.coords("bb_mid")
    feat = synth.randn((len(idx), 4), 21)
    bb = B3.VoxelResBackBone8xVoxelNeXt({}, 4, [88, 72, 16])
    bb.load_state_dict({k: t(np.asarray(v)) for k, v in SC.backbone_state(4, 5).items()}, strict=True)
    cfg = VC.head_cfg(VC.NUSC_HEADS, True, 8, 8, kernel_size=1, bias_before_norm=True, limit=WIDE, score_thresh=None)
    head = SH.VoxelNeXtHead(cfg, 128, 10, VC.NUSC_CLASSES, np.array([88, 72, 16]), [0.0, 0.0, -2.0, 8.8, 7.2, 1.2], [0.1, 0.1, 0.2])
    head.load_state_dict({k: t(v) for k, v in VC.state(cfg, 84, 2.5, -2.0).items()}, strict=True)
    bb, head = bb.to(DEV).eval(), head.to(DEV).eval()

    def forward():
        bd = dict(voxel_features=t(feat).to(DEV), voxel_coords=t(idx).to(DEV), batch_size=batch)
        with torch.no_grad():
            bd = head(bb(bd))
        return bd, [{k: v.clone() for k, v in p.items()} for p in head.forward_ret_dict["pred_dicts"]]

    d1, p1 = forward()
    x = d1["encoded_spconv_tensor"]
    assert len(x.spatial_shape) == 2 and x.features.shape[1] == 128 and len(d1["final_box_dicts"]) == batch
    counts = torch.bincount(x.indices[:, 0].long(), minlength=batch).tolist()
    for s, f in enumerate(d1["final_box_dicts"]):
        assert f["pred_boxes"].shape[1] == 9 and len(f["pred_boxes"]) == len(f["pred_scores"]) == len(f["pred_labels"])
        assert (len(f["pred_scores"]) > 0) == (counts[s] > 0), (s, counts)
    ref = VC.head_rows(cfg, VC.state(cfg, 84, 2.5, -2.0), x.features.cpu().numpy(), x.indices.cpu().numpy())
    err = rows_err(p1, ref)
    print(f"chain: {counts} rows per scene; head rows on the backbone's output vs fp64 restatement {err:.3e}")
    assert err <= BAR
    d2, p2 = forward()
    for a, b in zip(p1, p2):
        assert all(torch.equal(a[k], b[k]) for k in a)
    for a, b in zip(d1["final_box_dicts"], d2["final_box_dicts"]):
        assert all(torch.equal(a[k], b[k]) for k in ("pred_boxes", "pred_scores", "pred_labels"))
