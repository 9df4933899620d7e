"""The routes of csrc/sparse_head.hip and k_voxel_decode that tests/test_gpu_voxelnext_head.py does not reach, on the MI355X against the
fp64 forms of tests/voxelnext_head_cases.py (tests/test_head_edges_conditions.py asserts on the CPU that each case reaches its route).

  lvq_sparse_head   tasks of at most four branches (the four-branch kernel, both precision forms); operands pitched for eight branches
                    under five-branch tasks; a 5 % table and a structured one whose tiles and 16-row blocks lack whole offsets, against
                    fp64, for unowned zeros and under a row permutation
  lvq_voxel_decode  three tasks of 1, 2 and 3 classes in one call (g = b * n_tasks + t, the class map's offsets, the pitch of the key
                    scratch); a plateau of 700 equal scores across the K-th place of a 1300-row scene, three keys per thread, the other
                    scenes' rows in between

Measured on the MI355X on 2026-10-21: bf16x3 2.4e-6 .. 7.3e-6 over the 18 four-branch cases (bar 1e-3), 3.1e-6 / 4.0e-6 with the wide
pitch, 3.2e-6 / 3.5e-6 on the 5 % and the structured table; plain bf16 1.31e-3 .. 3.13e-3 (k_vol 1) and 1.55e-3 .. 2.52e-3 (k_vol 9)
against twice PLAIN_MEASURED = 4.2e-3 / 4.28e-3; decode scores at most 1.30e-7 and boxes 1.56e-7 relative (bar 1e-5).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_voxelnext_head as T  # noqa: E402
import voxelnext_head_cases as VC  # noqa: E402

BAR, TASK_C = T.BAR, T.TASK_C


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_sparse_head
# ---------------------------------------------------------------------------------------------------------------------------------
def check_head(c, label):
    out = T.run_head(c)
    got = out.cpu().numpy()
    err = T.rel_err(got, c["ref"])
    print(f"{label} bf16x3: {err:.3e} (max|ref| {np.abs(c['ref']).max():.2f})")
    assert got.shape == c["ref"].shape and err <= BAR
    unowned = [TASK_C * ti + ch for ti, o in enumerate(c["owner"]) for ch, b in enumerate(o) if b < 0]
    assert unowned and not got[unowned].any()                                    # exact zeros
    assert torch.equal(out, T.run_head(c))                                       # two runs give the same bits
    return got


@pytest.mark.parametrize("layout, kvol, n", VC.EDGE_SIZES)
def test_sparse_head_with_at_most_four_branches(layout, kvol, n):
    c = VC.edge_head_case(layout, n, kvol)
    assert max(c["n_br"]) <= 4 and c["bs"] == max(c["n_br"])
    check_head(c, f"{layout} N={n} k_vol={kvol}")
    plain = T.rel_err(T.run_head(c, split=False).cpu().numpy(), c["ref"])
    print(f"{layout} N={n} k_vol={kvol} bf16: {plain:.3e} (measured on the first suite's cases: {T.PLAIN_MEASURED[f'kvol{kvol}']})")
    assert plain <= 2 * T.PLAIN_MEASURED[f"kvol{kvol}"]


@pytest.mark.parametrize("kvol, n", [(1, 65), (9, 200)])
def test_sparse_head_operands_pitched_wider_than_the_branches(kvol, n):
    """br_stride = 8 under two five-branch tasks: weights, scale and shift of a task start 8 slots apart, slots 5 .. 7 hold values."""
    c = VC.edge_head_case("wide_pitch", n, kvol, 8)
    assert c["bs"] == 8 and c["n_br"] == [5, 5] and c["w1"].shape[1] == 8 and np.abs(c["w1"][:, 5:]).min() > 0
    got = check_head(c, f"wide pitch N={n} k_vol={kvol}")
    tight = dict(c, bs=5, w1=np.ascontiguousarray(c["w1"][:, :5]), scale=np.ascontiguousarray(c["scale"][:, :5]),
                 shift=np.ascontiguousarray(c["shift"][:, :5]))
    assert np.array_equal(T.run_head(tight).cpu().numpy().view(np.uint32), got.view(np.uint32))       # the pitch changes no bit


@pytest.mark.parametrize("table", ["sparse5", "structured"])
def test_sparse_head_tables_that_lack_offsets(table):
    n = 200
    c = VC.edge_head_case("three_four", n, 9, None, table)
    base = check_head(c, f"{table} N={n}")
    p = np.random.default_rng(3).permutation(n)                                  # new row j holds old row p[j]
    inv = np.empty(n, np.int64)
    inv[p] = np.arange(n)
    old = c["nbr"][p].astype(np.int64)
    nbr = np.where((old >= 0) & (old < n), inv[np.clip(old, 0, n - 1)], old).astype(np.int32)
    assert VC.tile_lacks(nbr, n)[0] != VC.tile_lacks(c["nbr"], n)[0]             # other offsets are skipped around a row now
    got = T.run_head(c, feat=c["feat"][p], nbr=nbr).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), base[:, p].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# lvq_voxel_decode
# ---------------------------------------------------------------------------------------------------------------------------------
def test_decode_three_tasks_in_one_call():
    idx, tasks = VC.multi_task_case()
    _, refs = T.check_decode_tasks(idx, tasks, 3, VC.MULTI_K, 0.1, T.CUT, VC.MULTI_IDS)          # (with decode_margins' distances)
    for t, ref in enumerate(refs):
        for d in ref:
            assert 0 < len(d["scores"]) <= VC.MULTI_K and set(d["labels"].tolist()) <= set(VC.MULTI_IDS[t])
            assert d["scores"].max() < 0.9                                       # the rows of no scene (score 0.9999) won nowhere
    assert any(len(d["scores"]) < VC.MULTI_K for ref in refs for d in ref)       # the threshold and the limit range cut


def test_decode_a_plateau_with_three_keys_per_thread():
    idx, task = VC.plateau_case()
    k = VC.PLATEAU_K
    _, ref = T.check_decode(idx, task, 3, k, 0.1, T.WIDE, [0, 1], stride=1, voxel=(0.2, 0.2), origin=(-4.0, -4.0), margins=False)
    d = ref[1]
    assert len(d["scores"]) == k and np.all(d["scores"][VC.PLATEAU_ABOVE:] == d["scores"][VC.PLATEAU_ABOVE])
    n = len(idx)
    level = np.nonzero((task["hm"] == np.float32(VC.PLATEAU_LOGIT)) & (idx[:, :1] == 1))          # (row, class) pairs
    want = np.sort(level[1] * n + level[0])[:k - VC.PLATEAU_ABOVE]
    assert np.array_equal(d["flat"][VC.PLATEAU_ABOVE:], want)                    # the lowest class * N + row
