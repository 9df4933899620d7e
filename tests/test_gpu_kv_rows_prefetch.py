"""k_kv_rows<J, X3, TH> (csrc/bev_tiles.hip) keeps the table rows of the next 16-row group -- and, across a tile boundary, of the next
tile's first group -- in flight behind hand-counted vector-memory waits.  A wait that is counted one too loose lets a wave
read T, key or rstd registers before they land, or still holding the previous group's rows; this file is built to see that.

  table     key k's row is T[k, c] = 16 (k % 29) + c / 128 (fp32; the fp16 form holds the same values rounded to fp16, all finite).
            The rows of one 16-row group, of neighbouring groups (keys 16 apart) and of the tiles a workgroup runs back to back (S5:
            32 tiles apart = 3 or 4 BEV tiles, keys 192 or 256 apart) all differ in k % 29, so a row built with another group's or
            another tile's T is off by at least 16 where the bound is about 1.1 (half a bf16 spacing at 480, plus a s).
  rows      the forced live list of S1 (tests/bev_tile_cases.py) cut to 1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65 and 129 dirty rows:
            both sides of every 16-row group and of the 64-row tile, a partial last tile behind full ones, and a single row.
  S5        workgroups run 3 and 2 tiles: the request that crosses the tile boundary, and the unused one of a workgroup's last tile.
  forms     n in {256, 768, 1024} x {plain, hi + lo operands} x {fp32, fp16 table}, and the fp16 K half once.
Every case: the fp64 bounds and the tie rule of tests/test_gpu_bev_tile_kernels.py (its KvRun.check, unchanged); canaries; for an fp32
table the rows equal the one-launch route (k_tile_kv) bit for bit, the V half alone under the fp16 K half; and the launch is repeated
REPS times into freshly filled buffers, every repetition equal to the first bit for bit -- a wait race is intermittent.

The share of rows that the tie rule sends to the loose bound comes from the reference alone: no row of the S1 list up to 129 rows has three
flagged channels (checked on the CPU by oracle/bev_tiles_oracle.loose_share), S5 is a case of tests/test_oracle_bev_tiles.py."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bev_tile_cases as BC  # noqa: E402
import test_gpu_bev_tile_kernels as TK  # noqa: E402
from oracle import bev_tiles_oracle as BO  # noqa: E402
from test_gpu_kernel_routes import DEV, OK, Canary, F, addr  # noqa: E402

ROW_CUTS = (1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 129)
REPS = 10


@functools.lru_cache(maxsize=None)
def prepared_cut(rows):
    """BC.prepared for the forced live list of S1 cut to ceil(rows / 8) pieces and `rows` dirty rows (the S4 mechanism, other counts)."""
    sc = dict(BC.scene("S1"), name=f"S1cut{rows}", force_all=True)
    B, H, W, nl = sc["B"], sc["H"], sc["W"], sc["n_live"]
    co = sc["coords"][:nl]
    occ = np.zeros((B, H, W), bool)
    occ[co[:, 0], co[:, 2], co[:, 3]] = True
    idx = np.full((B, H, W), -1, np.int32)
    idx[co[:, 0], co[:, 2], co[:, 3]] = np.arange(nl, dtype=np.int32)
    codes, pdirty, _, _ = BO.bookkeeping(occ, 0, force_all=True)
    codes, pdirty, counts = BC.cut_lists(codes, pdirty, -(-rows // 8), rows)
    w9, b9 = BC.conv_weights()
    t, mag = BO.conv_tokens(sc["feat"][:nl], co, B, H, W, w9, b9)
    r = BO.rows_of(codes, pdirty, B, H, W)
    assert len(r["s"]) == rows == counts[2]
    sc.update(occ=occ, idx=idx, codes=codes, pdirty=pdirty, counts=counts, rows=r, t=t, mag=mag,
              t_rows=t[r["s"], r["y"], r["x"]], mag_rows=mag[r["s"], r["y"], r["x"]])
    return sc


@functools.lru_cache(maxsize=None)
def dev_cut(rows):
    """The device side of prepared_cut, in the layout of TK.dev_scene."""
    sc = prepared_cut(rows)
    B, H, W = sc["B"], sc["H"], sc["W"]
    nt = (H // 8) * (W // 8)
    live = np.full(B * nt * 8, -1, np.int32)
    live[:len(sc["codes"])] = sc["codes"]
    dirty = np.zeros((B * nt * 8, 2), np.int32)
    dirty[:len(sc["pdirty"])] = sc["pdirty"]
    w9, b9 = BC.conv_weights()
    return dict(sc=sc, B=B, H=H, W=W, cap_tiles=B * nt, nd=rows, feat=TK.dev(sc["feat"]), idx=TK.dev(sc["idx"]), live=TK.dev(live),
                dirty=TK.dev(dirty), counts=TK.dev(np.asarray(sc["counts"], np.int32)), w9=TK.dev(w9), b9=TK.dev(b9))


@functools.lru_cache(maxsize=4)
def pattern_table(n, hw, f16):
    """T[k, c] = 16 (k % 29) + c / 128 as the kernel is given it -> (device, fp64 host)."""
    k, c = np.arange(hw, dtype=np.float32)[:, None], np.arange(2 * n, dtype=np.float32)[None, :]
    t = torch.from_numpy(np.float32(16.0) * np.mod(k, np.float32(29.0)) + c / np.float32(128.0))
    if f16:
        t = t.to(torch.float16)
        assert bool(torch.isfinite(t).all())
    return t.to(DEV).contiguous(), t.double().numpy()


class PfRun(TK.KvRun):
    """TK.KvRun on a scene dict of its own and the pattern table; check / intact / rows / values are the parent's."""

    def __init__(self, d, n, mode, form):
        self.d, self.n, self.mode, self.form = d, n, mode, form
        k = TK.kv_dev(n, mode)
        self.t16, self.k16 = form in ("t16", "both"), form in ("k16", "both")
        self.tab, self.T = pattern_table(n, d["H"] * d["W"], self.t16)
        f = F()
        L = f.lib()
        self.out = Canary(torch.bfloat16, (d["cap_tiles"] * 64, 2 * n), (2 * n, 1), 64, 4 * n + 64)
        self.ws_bytes = int(L.lvq_bev_tile_kv_workspace_bytes(f.i64(d["cap_tiles"])))
        self.ws = torch.full((self.ws_bytes + 256,), 0xA5, dtype=torch.uint8, device=DEV) if form != "one" else None
        self.rc = L.lvq_bev_tile_kv(addr(d["feat"]), addr(d["idx"]), addr(d["live"]), addr(d["dirty"]), addr(d["counts"]), f.i64(d["cap_tiles"]),
                                    f.cint(d["B"]), f.cint(d["H"]), f.cint(d["W"]), f.cint(64), addr(d["w9"]), addr(d["b9"]), addr(k["m"]),
                                    addr(k["m_lo"]), addr(k["m0"]), addr(k["r"]), addr(k["r_lo"]), addr(k["r0"]), f.cfloat(BC.C0), f.cint(n),
                                    f.cfloat(BC.EPS), addr(self.tab), f.cint(int(self.t16)), f.cint(n), f.cint(int(self.k16)), self.out.ptr(),
                                    addr(self.ws), f.csize(self.ws_bytes if form != "one" else 0), f.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()


def _case(d, n, mode, form, label, sel=None):
    """One case: fp64 bound and canaries, equality with the one-launch route where one exists, REPS repetitions equal to the first."""
    first = PfRun(d, n, mode, form)
    first.check(label, sel=sel, total_rows=d["nd"])
    whole = first.out.result().view(torch.int16)
    if not first.t16:
        one = PfRun(d, n, mode, "one")
        assert one.rc == OK and one.intact(d["nd"]), label
        cols = slice(n, 2 * n) if first.k16 else slice(0, 2 * n)      # the K half as fp16 has no one-launch form: its V half does
        assert torch.equal(first.rows()[:, cols], one.rows()[:, cols]), f"{label}: two launches != one launch"
        del one
    for rep in range(1, REPS):
        again = PfRun(d, n, mode, form)
        assert again.rc == OK and again.intact(d["nd"]), (label, rep)
        assert torch.equal(again.out.result().view(torch.int16), whole), f"{label}: repetition {rep} differs from the first launch"
        del again


@pytest.mark.parametrize("form", ["two", "t16"])
@pytest.mark.parametrize("mode", ["plain", "x3"])
@pytest.mark.parametrize("n", [256, 768, 1024])
def test_row_counts_at_every_pipeline_boundary(n, mode, form):
    for rows in ROW_CUTS:
        _case(dev_cut(rows), n, mode, form, f"prefetch {rows} rows")


def test_row_counts_with_the_fp16_k_half():
    for rows in ROW_CUTS:
        _case(dev_cut(rows), 768, "x3", "k16", f"prefetch {rows} rows")


@pytest.mark.parametrize("form", ["two", "both"])
def test_tile_boundary_and_last_tile_of_a_workgroup(form):
    """S5: workgroups run 3 and 2 tiles.  Held to the fp64 bound: the dirty rows and every 11th row (11 is odd: every lane, group and tile
    position occurs); every row takes part in the equalities."""
    d = TK.dev_scene("S5")
    groups, grid = d["cap_tiles"], 2 * min(TK.cus(), d["cap_tiles"])
    assert TK._groups_per_workgroup(groups, grid, 2) >= 2 and groups > grid // 2
    sel = np.union1d(np.nonzero(d["sc"]["dirty"])[0], np.arange(0, d["nd"], 11))
    _case(d, 768, "x3", form, "prefetch S5", sel=sel)
