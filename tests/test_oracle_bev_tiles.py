"""CPU checks of oracle/bev_tiles_oracle.py, the fp64 reference of tests/test_gpu_bev_tile_kernels.py, before anyone trusts it on a GPU:
against the ported model (oracle/vat_oracle.py, the unfolded chain conv -> proj -> LayerNorm -> + PE -> in_proj rows d..3d), its bf16
rounding against torch's, and the share of rows that the tie rule sends to the loose bound in every case of the GPU file."""
import numpy as np
import pytest
import torch

import bev_tile_cases as BC
from oracle import bev_tiles_oracle as BO
from oracle import vat_oracle as VO
from test_fold_algebra import _fold


def test_bf16_rounding_matches_torch():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(200000) * np.exp(rng.uniform(-30, 30, 200000))).astype(np.float32)
    x[:4] = [0.0, 1.0, 1.00390625, -3.0e-39]                     # zero, an exact value, a midpoint (tie to even), below the normal range
    want = torch.from_numpy(x).to(torch.bfloat16).double().numpy()
    assert np.array_equal(BO.bf16_round(x.astype(np.float64)), want)
    dn, up = BO.bf16_down_up(x.astype(np.float64))
    assert bool(((dn <= x) & (x < up)).all()) and np.array_equal(BO.bf16_round(dn), dn) and np.array_equal(BO.bf16_round(up), up)
    # the flagged band: exactly a midpoint, and just outside 2^-20 * mag of it
    mid = np.array([1.00390625, 1.00390625 + 3e-6, 1.00390625 - 3e-6, 1.0])
    assert BO.near_midpoint(mid, np.full(4, 2.0)).tolist() == [True, False, False, False]
    hi_lo = BO.round_t(np.array([1.0 / 3.0]), "x3")
    assert abs(float(hi_lo[0]) - 1.0 / 3.0) < 2.0 ** -17 / 3.0


def test_bookkeeping_rows_and_keys():
    """rows_of numbers the dirty cells as bookkeeping does, keys are tile-major, and the cut lists of S4 hit their remainders."""
    for name in ("S1", "S2", "S3"):
        sc = BC.prepared(name)
        B, H, W = sc["B"], sc["H"], sc["W"]
        rows = sc["rows"]
        assert len(rows["s"]) == sc["counts"][2] and bool(sc["dirty"].all())
        assert np.array_equal(rows["key"], BO.key_of(rows["y"], rows["x"], W))
        assert np.array_equal(sc["row_src"][rows["s"], rows["key"]], np.arange(len(rows["s"])))
    want = dict(S4a=(1, 5), S4b=(7, 16), S4c=(9, 63), S4d=(15, 64), S4e=(9, 65), S4z=(0, 0))
    for name, (pieces, nrows) in want.items():
        sc = BC.prepared(name)
        assert (sc["counts"][0], sc["counts"][2]) == (pieces, nrows) and len(sc["rows"]["s"]) == nrows
    assert {want[k][0] % 8 for k in want} >= {1, 7}
    s2 = BC.prepared("S2")
    assert not s2["occ"][1].any() and s2["occ"][0, 13, 5] and s2["occ"][2, 13, 5]
    perm = BO.tile_major(np.arange(40 * 16)[:, None], 40, 16)[:, 0]
    assert sorted(perm.tolist()) == list(range(640)) and perm[BO.key_of(13, 5, 16)] == 13 * 16 + 5


def test_references_equal_the_unfolded_model_chain():
    """tile_kv_ref and tile_tokens_ref with exact (unrounded) operands against the ported model on every cell, to 1e-10 relative: a
    seeded VATLiDAR (d = 256) on a 16 x 24 grid, its weights folded by the fp64 _fold of tests/test_fold_algebra.py."""
    from lidar_vision_vqa_amd import fusion, synth
    B, H, W, C, d = 2, 16, 24, 64, 256
    m = synth.load_seeded(fusion.VATLiDAR(C, d, n_queries=12, n_layers=1, n_heads=4), 71)
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(72)
    cells = rng.permutation(B * H * W)[:60]
    coords = np.stack((cells // (H * W), np.zeros_like(cells), (cells // W) % H, cells % W), 1)
    feat = rng.standard_normal((60, C))
    bev = torch.zeros(B, C, H, W, dtype=torch.float64)
    bev[coords[:, 0], :, coords[:, 2], coords[:, 3]] = torch.from_numpy(feat)
    w9, b9 = sd["refine.0.weight"].view(C, 9).numpy(), sd["refine.0.bias"].numpy()
    t, mag = BO.conv_tokens(feat, coords, B, H, W, w9, b9)
    assert bool((mag >= np.abs(b9)).all())
    pe, ve = VO.lidar_pe(H, W, sd)
    wp, bp = sd["proj.weight"].view(d, C), sd["proj.bias"]
    gam, bet = sd["norm_tokens.weight"], sd["norm_tokens.bias"]
    f = _fold(wp, bp, gam, bet, pe + ve, sd["blocks.0.ca.in_proj_weight"][d:], sd["blocks.0.ca.in_proj_bias"][d:])
    rows = BO.rows_of(*BO.bookkeeping(np.zeros((B, H, W), bool), 0, force_all=True)[:2], B, H, W)       # every cell
    cell = rows["s"] * H * W + rows["y"] * W + rows["x"]
    want_kv = VO.vat_lidar_kv(bev, sd).reshape(B * H * W, 2 * d).numpy()[cell]
    got_kv = BO.tile_kv_ref(t, f["m"].numpy(), f["m0"].numpy(), f["rt"].numpy(), f["r0"].numpy(), float(f["c0"]), d, 1e-5,
                            BO.tile_major(f["t"].numpy(), H, W), "exact")
    assert got_kv.shape == want_kv.shape
    assert float(np.abs(got_kv - want_kv).max()) <= 1e-10 * float(np.abs(want_kv).max())
    want_x = VO.vat_lidar_tokens(bev, sd).reshape(B * H * W, d).numpy()[cell]
    got_x = BO.tile_tokens_ref(t, wp.numpy(), bp.numpy(), gam.numpy(), bet.numpy(), 1e-5, BO.tile_major((pe + ve).numpy(), H, W), "exact")
    assert float(np.abs(got_x - want_x).max()) <= 1e-10 * float(np.abs(want_x).max())
    # `rows` selects and orders: the dirty rows of the scene are the same numbers
    occ = np.zeros((B, H, W), bool)
    occ[coords[:, 0], coords[:, 2], coords[:, 3]] = True
    sub = BO.rows_of(*BO.bookkeeping(occ, 0)[:2], B, H, W)
    sel = sub["s"] * H * W + sub["y"] * W + sub["x"]
    pos = {int(c): i for i, c in enumerate(cell)}
    got_sub = BO.tile_kv_ref(t, f["m"].numpy(), f["m0"].numpy(), f["rt"].numpy(), f["r0"].numpy(), float(f["c0"]), d, 1e-5,
                             BO.tile_major(f["t"].numpy(), H, W), "exact", rows=sub)
    assert np.array_equal(got_sub, got_kv[[pos[int(c)] for c in sel]])


def test_judge_rows_sees_one_ulp_and_follows_the_tie_rule():
    """judge_rows on made-up kernel rows: the exact reference passes, one bf16 ulp on one entry fails, a row whose flagged channel the
    kernel rounded the other way passes through its variant, and a row with three flagged channels is counted as loose."""
    sc = BC.prepared("S1")
    ops = BC.kv_operands(256)
    hw = sc["H"] * sc["W"]
    bf = lambda a: torch.from_numpy(a).to(torch.bfloat16).double().numpy()
    ref_fn = lambda t_op, keys: BO.kv_rows(t_op, keys, bf(ops["M"]), ops["m0"], bf(ops["R"]), ops["r0"], BC.C0, 256, BC.EPS, ops["T"][:hw])
    tol = lambda ref, scale: BO.tight_bound(ref, scale, 2e-5)
    t_rows, mag_rows, keys = sc["t_rows"].copy(), sc["mag_rows"], sc["rows"]["key"]
    t_rows[0, 5] = 1.00390625                                     # a midpoint: the kernel may hold 1.0 or 1.0078125
    t_rows[1, 3:6] = 1.00390625                                   # three flagged channels
    exact = BO.bf16_round(ref_fn(BO.round_t(t_rows, "plain"), keys))
    assert BO.judge_rows(exact, t_rows, mag_rows, keys, "plain", ref_fn, tol)["ratio"] <= 1.0
    other = BO.round_t(t_rows, "plain")
    other[0, 5] = 1.0078125
    moved = exact.copy()
    moved[0] = BO.bf16_round(ref_fn(other[:1], keys[:1]))[0]
    res = BO.judge_rows(moved, t_rows, mag_rows, keys, "plain", ref_fn, tol)
    assert res["ratio"] <= 1.0 and res["tie_rows"] >= 1 and res["share"] > 0 and res["loose_ratio"] <= 1.0
    assert float(np.abs(moved[0] - exact[0]).max()) > 0           # the flip is visible in the row
    ulp = exact.copy()
    j = int(np.argmax(np.abs(exact[7])))
    ulp[7, j] += BO._ulp(exact[7, j:j + 1])[0]
    assert BO.judge_rows(ulp, t_rows, mag_rows, keys, "plain", ref_fn, tol)["ratio"] > 1.0


@pytest.mark.parametrize("name", BC.ALL_SCENES)
def test_tie_rule_leaves_the_tight_bound_in_force(name):
    """The share of rows with three or more flagged channels (plain operands; hi + lo operands flag nothing) is below 0.5 % in every case of
    the GPU file, from the reference alone.  GELU(b9), the token of every clean cell, has no flagged channel at all."""
    sc = BC.prepared(name)
    share = BO.loose_share(sc["t_rows"], sc["mag_rows"], "plain")
    nf = BO.flag_counts(sc["t_rows"], sc["mag_rows"], "plain")
    print(f"{name}: {len(nf)} rows, {int((nf > 0).sum())} with a flagged channel, {int((nf >= 3).sum())} with three or more ({100 * share:.3f} %)")
    assert share < BO.LOOSE_SHARE, (name, share)
    assert BO.loose_share(sc["t_rows"], sc["mag_rows"], "x3") == 0.0
    _, b9 = BC.conv_weights()
    clean = BO.gelu_erf(b9.astype(np.float64))
    assert not BO.near_midpoint(clean, np.abs(b9.astype(np.float64))).any()
