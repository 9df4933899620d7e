"""The four MFMA kernels of csrc/bev_tiles.hip that produce every key and value of VATLiDAR's sparse route -- k_tile_tokens<J, X3, OLO>,
k_tile_kv<J, X3>, k_conv_rows<X3>, k_kv_rows<J, X3, TH> -- through the C ABI (lvq_bev_tile_tokens, lvq_bev_tile_kv) against the fp64
restatement of include/lvq.h in oracle/bev_tiles_oracle.py, which tests/test_oracle_bev_tiles.py pins to the ported model on the CPU.

Buffers are the test's own: outputs hold exactly cap_tiles * 64 rows plus a tail and are pre-filled with 0xA5 (the Canary of
test_gpu_kernel_routes.py); every case requires the rows at or beyond counts[2], the head and the tail to still hold the pattern, and the
same of the bytes behind the two-launch workspace.  Operands are drawn directly (tests/bev_tile_cases.py), not folded from a model:
w9 ~ 0.3, M, R ~ N(0, 1/64), Wp ~ 0.15, m0, r0, T, PE, bias, beta ~ N(0, 1), gamma ~ 1 + N(0, 1), c0 = 0.7, eps = 1e-5, d_ln = n.

Scenes S1 .. S5 are described in tests/bev_tile_cases.py; their sizes follow from the dispatch arithmetic (grid = min(CUs, cap_tiles), x 2
column halves for the K|V kernels; a grid that is a multiple of 16 (8 for the token kernel) takes the XCD-partitioned work order) with
the CU count read from the device.

Bounds (derived, never measured; every case prints its figures next to them):
  bf16 rows       |got - ref| <= ulp_bf16(|ref| + a s) / 2 + a s,  s = max(1, max|ref|), a = 2e-5 for plain operands and 2e-4 for hi + lo
                  (the project's fp32 GEMM bounds, test_gpu_kernel_routes.py: everything before the final rounding).  Half a bf16
                  spacing is 2^-9 |ref| at the top of a binade and 2^-8 |ref| at its bottom -- a correctly rounded 1.0039 is off by
                  2^-8 -- so the bound uses the spacing itself (oracle/bev_tiles_oracle.tight_bound); a row that is off by one whole
                  spacing fails wherever half a spacing exceeds a s (tests/test_oracle_bev_tiles.py checks that on the largest entry of
                  a row).
  fp16 K half     the same with the fp16 spacing (2^-12 .. 2^-11 |ref|) on columns 0 .. n-1, all values finite; the V half stays bf16
  tokens hi + lo  |hi + lo - ref| <= 2e-4 s; hi alone is held to the bf16 bound
  ties            the conv token t is rounded to bf16 from fp32 by the kernel and from fp64 by the reference: rows with one or two
                  channels within 2^-20 mag of a rounding midpoint pass against any up / down variant, rows with three or more are held
                  to 2^-6 max|ref| and must be fewer than 0.5 % of a case's rows (oracle/bev_tiles_oracle.py: judge_rows)
Equalities that follow from the code are asserted bit for bit (DESIGN.md "Numerics"): two launches == one launch, a dirty cell's row ==
the same cell's row under force_all, a clean cell's row under force_all == the empty-scene row of its key, a scene alone == the same
scene inside a batch.

profiles/bev_tiles_kernel_stats.csv is a kernel trace of this file (kernel trace and stats only, no counters): all 38 instantiations
appear in it -- 12 k_tile_tokens (4 n x {plain, x3, x3 + lo}), 8 k_tile_kv (4 n x 2 operand forms), 2 k_conv_rows, 16 k_kv_rows (4 n x 2
operand forms x {fp32, fp16} T)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bev_tile_cases as BC  # noqa: E402
from oracle import bev_tiles_oracle as BO  # noqa: E402
from test_gpu_kernel_routes import DEV, EINVAL, EUNSUPPORTED, EWORKSPACE, OK, Canary, F, addr, hi_lo  # noqa: E402

NS = BC.NS
KV_FORMS = ("one", "two", "t16", "k16", "both")                 # one launch | two launches | + fp16 T | + fp16 K half | + both
TOK_FORMS = ("plain", "x3", "x3lo")                             # plain operands | hi + lo operands, hi out | hi + lo operands, hi + lo out
A_PLAIN, A_X3 = 2e-5, 2e-4
PATTERN16 = -23131                                               # 0xA5A5


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ops():
    from lidar_vision_vqa_amd import ops as o
    return o


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------
# scenes and operands on the device
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dev_scene(name):
    """A scene of bev_tile_cases on the device.  The bookkeeping lists come from lvq_bev_tiles itself (and must equal the numpy
    restatement), except for the S4 lists that are cut on the host."""
    sc = BC.prepared(name, cus())
    B, H, W = sc["B"], sc["H"], sc["W"]
    nt = (H // 8) * (W // 8)
    d = dict(sc=sc, B=B, H=H, W=W, cap_tiles=B * nt, nd=int(sc["counts"][2]))
    feat = sc["feat"] if len(sc["feat"]) else np.zeros((1, BC.C), np.float32)
    d["feat"] = dev(feat)
    d["idx"] = dev(sc["idx"])
    if sc["cut"]:
        live = np.full(B * nt * 8, -1, np.int32)
        live[:len(sc["codes"])] = sc["codes"]
        dirty = np.zeros((B * nt * 8, 2), np.int32)
        dirty[:len(sc["pdirty"])] = sc["pdirty"]
        d["live"], d["dirty"], d["counts"] = dev(live), dev(dirty), dev(np.asarray(sc["counts"], np.int32))
    else:
        live, dirty, src, counts = ops().bev_tiles(d["idx"], B, H, W, DEV, 0, force_all=sc["force_all"])
        n = sc["counts"][0]
        assert counts.cpu().tolist() == list(sc["counts"]), name
        assert live.cpu().numpy()[:n].tolist() == list(sc["codes"]) and dirty.cpu().numpy()[:n].tolist() == [list(x) for x in sc["pdirty"]], name
        assert np.array_equal(src.cpu().numpy(), sc["row_src"].astype(np.int32)), name
        d["live"], d["dirty"], d["counts"] = live, dirty, counts
    w9, b9 = BC.conv_weights()
    d["w9"], d["b9"] = dev(w9), (dev(b9) if sc["use_b9"] else None)
    return d


def _pair(x, mode):
    """fp32 host matrix -> (device hi, device lo | None, fp64 value the kernel sees)."""
    hi, lo = hi_lo(dev(x))
    if mode == "plain":
        return hi, None, hi.double().cpu().numpy()
    return hi, lo, (hi.double() + lo.double()).cpu().numpy()


@functools.lru_cache(maxsize=8)
def kv_dev(n, mode):
    o = BC.kv_operands(n)
    m, m_lo, m_eff = _pair(o["M"], mode)
    r, r_lo, r_eff = _pair(o["R"], mode)
    return dict(m=m, m_lo=m_lo, M=m_eff, r=r, r_lo=r_lo, R=r_eff, m0=dev(o["m0"]), r0=dev(o["r0"]), m0h=o["m0"], r0h=o["r0"])


@functools.lru_cache(maxsize=4)
def kv_table(n, hw, f16):
    """T[:hw] as the kernel is given it (fp32, or the fp16 values) -> (device, fp64 host)."""
    t = torch.from_numpy(BC.kv_operands(n)["T"][:hw])
    if f16:
        t = t.to(torch.float16)
    return t.to(DEV).contiguous(), t.double().numpy()


@functools.lru_cache(maxsize=8)
def tok_dev(n, mode):
    o = BC.token_operands(n)
    w, w_lo, w_eff = _pair(o["Wp"], mode)
    return dict(w=w, w_lo=w_lo, W=w_eff, bias=dev(o["bias"]), gamma=dev(o["gamma"]), beta=dev(o["beta"]), host=o)


@functools.lru_cache(maxsize=4)
def tok_table(n, hw):
    t = torch.from_numpy(BC.token_operands(n)["PE"][:hw])
    return t.to(DEV).contiguous(), t.double().numpy()


def rows_untouched(c, nd):
    """Rows nd .. of the canary's result still hold the pattern (head and tail: Canary.untouched)."""
    torch.cuda.synchronize()
    return bool((c.result()[nd:].view(torch.int16) == PATTERN16).all())


# ------------------------------------------------------------------------------------------------
# lvq_bev_tile_kv
# ------------------------------------------------------------------------------------------------
class KvRun:
    def __init__(self, name, n, mode, form, **over):
        d = dev_scene(name)
        self.d, self.n, self.mode, self.form = d, n, mode, form
        k = kv_dev(n, mode)
        hw = d["H"] * d["W"]
        self.t16, self.k16 = form in ("t16", "both"), form in ("k16", "both")
        self.tab, self.T = kv_table(n, hw, self.t16)
        L = F().lib()
        self.out = Canary(torch.bfloat16, (d["cap_tiles"] * 64, 2 * n), (2 * n, 1), 64, 4 * n + 64)
        self.ws_bytes = int(L.lvq_bev_tile_kv_workspace_bytes(F().i64(d["cap_tiles"])))
        self.ws = torch.full((self.ws_bytes + 256,), 0xA5, dtype=torch.uint8, device=DEV) if form != "one" else None
        a = dict(feat=addr(d["feat"]), c_in=64, ny=d["H"], n_abi=n, kv=self.out.ptr(), ws=addr(self.ws), ws_bytes=self.ws_bytes if form != "one" else 0,
                 m_lo=addr(k["m_lo"]), r_lo=addr(k["r_lo"]), t16=int(self.t16), k16=int(self.k16))
        a.update(over)
        f = F()
        self.rc = L.lvq_bev_tile_kv(a["feat"], addr(d["idx"]), addr(d["live"]), addr(d["dirty"]), addr(d["counts"]), f.i64(d["cap_tiles"]), f.cint(d["B"]),
                                    f.cint(a["ny"]), f.cint(d["W"]), f.cint(a["c_in"]), addr(d["w9"]), addr(d["b9"]), addr(k["m"]), a["m_lo"], addr(k["m0"]),
                                    addr(k["r"]), a["r_lo"], addr(k["r0"]), f.cfloat(BC.C0), f.cint(n), f.cfloat(BC.EPS), addr(self.tab), f.cint(a["t16"]),
                                    f.cint(a["n_abi"]), f.cint(a["k16"]), a["kv"], a["ws"], f.csize(a["ws_bytes"]), f.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()

    def intact(self, nd):
        """Nothing outside rows 0 .. nd-1 of the output was written, nor the bytes behind the workspace."""
        ok = self.out.untouched() and rows_untouched(self.out, nd)
        if self.ws is not None:
            ok = ok and bool((self.ws[self.ws_bytes:] == 0xA5).all())
        return ok

    def rows(self):
        return self.out.result()[:self.d["nd"]]

    def values(self, sel):
        """The written rows `sel` as fp64 (the K half read as IEEE fp16 under k_fp16)."""
        got = self.rows()[torch.from_numpy(sel).to(DEV)]
        n = self.n
        if not self.k16:
            return got.double().cpu().numpy()
        k = got[:, :n].contiguous().view(torch.float16)
        assert bool(torch.isfinite(k).all()), "fp16 K half: a value that is not finite"
        return torch.cat((k.double(), got[:, n:].double()), 1).cpu().numpy()

    def check(self, label, sel=None, total_rows=None):
        """Return code, canaries and the fp64 bound on rows `sel` (default: all written rows)."""
        assert self.rc == OK, (label, self.rc)
        d, n, sc = self.d, self.n, self.d["sc"]
        assert self.intact(d["nd"]), f"{label}: a store outside rows 0 .. {d['nd'] - 1} of the [{d['cap_tiles'] * 64}, {2 * n}] output"
        k = kv_dev(n, self.mode)
        a = A_PLAIN if self.mode == "plain" else A_X3
        ref_fn = lambda t_op, keys: BO.kv_rows(t_op, keys, k["M"], k["m0h"], k["R"], k["r0h"], BC.C0, n, BC.EPS, self.T)

        def tol(ref, scale):
            if not self.k16:
                return BO.tight_bound(ref, scale, a)
            return np.concatenate((BO.tight_bound(ref[..., :n], scale, a, "fp16"), BO.tight_bound(ref[..., n:], scale, a)), -1)

        sel = np.arange(d["nd"]) if sel is None else sel
        res = BO.judge_rows(self.values(sel), sc["t_rows"][sel], sc["mag_rows"][sel], sc["rows"]["key"][sel], self.mode, ref_fn, tol)
        return report(f"kv {label} {sc['name']} n={n} {self.mode} {self.form}", res, total_rows or d["nd"])


def report(label, res, total_rows):
    share = res["loose_rows"] / total_rows if total_rows else 0.0
    print(f"{label}: {res['rows']} rows, err {res['err']:.3e} (bound {res['bound']:.3e}), worst err / bound {res['ratio']:.3f}, max|ref| {res['amax']:.3f}, "
          f"{res['tie_rows']} rows through tie variants, {res['loose_rows']} rows at the loose bound ({100 * share:.3f} %, worst {res['loose_ratio']:.3f} of it)")
    assert res["ratio"] <= 1.0, (label, res)
    assert res["loose_ratio"] <= 1.0, (label, res)
    assert share < BO.LOOSE_SHARE, (label, share)
    return res


@pytest.mark.parametrize("name", BC.ROUTE_SCENES)
@pytest.mark.parametrize("form", KV_FORMS)
@pytest.mark.parametrize("mode", ["plain", "x3"])
@pytest.mark.parametrize("n", NS)
def test_tile_kv_routes_vs_fp64(n, mode, form, name):
    """Every route of lvq_bev_tile_kv on S1 .. S4: k_tile_kv<J, X3> (one launch) or k_conv_rows<X3> + k_kv_rows<J, X3, TH> (two launches;
    TH = fp16 table; the K half as fp16 is a run-time flag of the same kernel)."""
    KvRun(name, n, mode, form).check("routes")


# ------------------------------------------------------------------------------------------------
# lvq_bev_tile_tokens
# ------------------------------------------------------------------------------------------------
class TokRun:
    def __init__(self, name, n, form, **over):
        d = dev_scene(name)
        self.d, self.n, self.form = d, n, form
        self.mode = "plain" if form == "plain" else "x3"
        k = tok_dev(n, self.mode)
        self.tab, self.PE = tok_table(n, d["H"] * d["W"])
        mk = lambda: Canary(torch.bfloat16, (d["cap_tiles"] * 64, n), (n, 1), 64, 2 * n + 64)
        self.x, self.xl = mk(), (mk() if form == "x3lo" else None)
        a = dict(c_in=64, ny=d["H"], n_abi=n, x=self.x.ptr())
        a.update(over)
        f = F()
        self.rc = f.lib().lvq_bev_tile_tokens(addr(d["feat"]), addr(d["idx"]), addr(d["live"]), addr(d["dirty"]), addr(d["counts"]), f.i64(d["cap_tiles"]),
                                              f.cint(d["B"]), f.cint(a["ny"]), f.cint(d["W"]), f.cint(a["c_in"]), addr(d["w9"]), addr(d["b9"]), addr(k["w"]),
                                              addr(k["w_lo"]), addr(k["bias"]), addr(k["gamma"]), addr(k["beta"]), f.cfloat(BC.EPS), addr(self.tab),
                                              f.cint(a["n_abi"]), a["x"], self.xl.ptr() if self.xl else addr(None), f.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()

    def outs(self):
        return [c for c in (self.x, self.xl) if c is not None]

    def intact(self, nd):
        return all(c.untouched() and rows_untouched(c, nd) for c in self.outs())

    def rows(self):
        return [c.result()[:self.d["nd"]] for c in self.outs()]

    def check(self, label, sel=None, total_rows=None):
        assert self.rc == OK, (label, self.rc)
        d, n, sc = self.d, self.n, self.d["sc"]
        assert self.intact(d["nd"]), f"{label}: a store outside rows 0 .. {d['nd'] - 1} of the [{d['cap_tiles'] * 64}, {n}] output"
        k = tok_dev(n, self.mode)
        h = k["host"]
        a = A_PLAIN if self.mode == "plain" else A_X3
        ref_fn = lambda t_op, keys: BO.tokens_rows(t_op, keys, k["W"], h["bias"], h["gamma"], h["beta"], BC.EPS, self.PE)
        sel = np.arange(d["nd"]) if sel is None else sel
        pick = torch.from_numpy(sel).to(DEV)
        hi = self.rows()[0][pick].double().cpu().numpy()
        args = (sc["t_rows"][sel], sc["mag_rows"][sel], sc["rows"]["key"][sel], self.mode, ref_fn)
        tag = f"tokens {label} {sc['name']} n={n} {self.form}"
        res = report(tag, BO.judge_rows(hi, *args, lambda ref, scale: BO.tight_bound(ref, scale, a)), total_rows or d["nd"])
        if self.xl is not None:
            both = hi + self.rows()[1][pick].double().cpu().numpy()
            report(tag + " hi + lo", BO.judge_rows(both, *args, lambda ref, scale: np.full_like(ref, A_X3 * scale)), total_rows or d["nd"])
        return res


@pytest.mark.parametrize("name", BC.ROUTE_SCENES)
@pytest.mark.parametrize("form", TOK_FORMS)
@pytest.mark.parametrize("n", NS)
def test_tile_tokens_routes_vs_fp64(n, form, name):
    """Every instantiation of k_tile_tokens<J, X3, OLO> on S1 .. S4."""
    TokRun(name, n, form).check("routes")


# ------------------------------------------------------------------------------------------------
# equalities that follow from the code
# ------------------------------------------------------------------------------------------------
def _row_index(sc):
    return {(int(s), int(k)): i for i, (s, k) in enumerate(zip(sc["rows"]["s"], sc["rows"]["key"]))}


def _assert_scene_equalities(run, label):
    """`run(scene name)` -> list of written row tensors.  S2 against its forced, empty and single-scene forms."""
    s2, s2f, s2e, s2s0 = (BC.prepared(x, cus()) for x in ("S2", "S2f", "S2e", "S2s0"))
    r2, r2f, r2e, r2s0 = run("S2"), run("S2f"), run("S2e"), run("S2s0")
    at_f, at_0 = _row_index(s2f), _row_index(s2s0)
    sk = list(zip(s2["rows"]["s"].tolist(), s2["rows"]["key"].tolist()))
    to_f = torch.tensor([at_f[x] for x in sk], device=DEV)
    clean = np.nonzero(~s2f["dirty"])[0]
    own = [i for i, (s, _) in enumerate(sk) if s == 0]
    assert len(sk) and len(clean) and len(own) == s2s0["counts"][2]
    for a, f, e, z in zip(r2, r2f, r2e, r2s0):
        assert torch.equal(a, f[to_f]), f"{label}: a dirty cell's row differs from the same cell's row under force_all"
        assert torch.equal(f[torch.from_numpy(clean).to(DEV)], e[torch.from_numpy(s2f["rows"]["key"][clean]).to(DEV)]), \
            f"{label}: a clean cell's row under force_all differs from the empty-scene row of its key"
        assert torch.equal(a[torch.tensor(own, device=DEV)], z[torch.tensor([at_0[(0, sk[i][1])] for i in own], device=DEV)]), \
            f"{label}: scene 0 alone differs from scene 0 inside the batch"


@pytest.mark.parametrize("mode", ["plain", "x3"])
@pytest.mark.parametrize("n", NS)
def test_tile_kv_equalities(n, mode):
    """Bit for bit: two launches == one launch (fp32 T, bf16 K half) on every scene; dirty row == the same cell under force_all; clean
    cell under force_all == the empty-scene row of its key (the per-model table property); a scene alone == inside a batch."""
    for name in BC.ROUTE_SCENES + ("S2f", "S2e", "S2s0"):
        one, two = KvRun(name, n, mode, "one"), KvRun(name, n, mode, "two")
        assert one.rc == OK and two.rc == OK and one.intact(one.d["nd"]) and two.intact(two.d["nd"]), name
        assert torch.equal(one.rows(), two.rows()), f"{name}: two launches != one launch"

    def run(name, form):
        r = KvRun(name, n, mode, form)
        assert r.rc == OK, name
        return [r.rows()]

    for form in KV_FORMS:
        _assert_scene_equalities(lambda name: run(name, form), f"kv n={n} {mode} {form}")


@pytest.mark.parametrize("form", TOK_FORMS)
@pytest.mark.parametrize("n", NS)
def test_tile_tokens_equalities(n, form):
    def run(name):
        r = TokRun(name, n, form)
        assert r.rc == OK, name
        return r.rows()

    _assert_scene_equalities(run, f"tokens n={n} {form}")


# ------------------------------------------------------------------------------------------------
# S5: more groups than twice the workgroups (the double-buffer paths has_nx / has_n2)
# ------------------------------------------------------------------------------------------------
def _groups_per_workgroup(groups, grid, halves):
    """Largest number of groups one workgroup runs under the work order of the kernels: a grid that is a multiple of 8 * halves deals
    ceil(groups / 8) groups to each XCD slice and walks them with grid / (8 * halves) workgroups; otherwise every workgroup strides."""
    if grid >= 8 * halves and grid % (8 * halves) == 0:
        per_x, wgs = -(-groups // 8), grid // (8 * halves)
    else:
        per_x, wgs = groups, -(-grid // halves)
    return -(-per_x // wgs)


@pytest.mark.parametrize("mode", ["plain", "x3"])
@pytest.mark.parametrize("n", [256, 768])
def test_many_groups_per_workgroup(n, mode):
    """S5, force_all on 2 CUs / 64 + 1 scenes of 64 x 64: every kernel runs workgroups with three (and two) groups.  The dirty cells are
    held to the fp64 bound directly; the clean ones must equal, bit for bit, the rows of the one-scene table (S5e), which is held to the
    fp64 bound in full."""
    d, e = dev_scene("S5"), dev_scene("S5e")
    sc = d["sc"]
    groups = d["cap_tiles"]                                         # force_all: every tile is one group of 8 pieces = 64 rows
    grid = min(cus(), d["cap_tiles"])
    assert groups > 2 * cus() and d["nd"] == 64 * groups
    assert _groups_per_workgroup(groups, grid, 1) >= 3              # k_tile_tokens
    assert -(-groups // grid) >= 3                                   # k_conv_rows: plain stride over the grid
    assert _groups_per_workgroup(groups, 2 * grid, 2) >= 2          # k_tile_kv, k_kv_rows
    dirty = np.nonzero(sc["dirty"])[0]
    clean = torch.from_numpy(np.nonzero(~sc["dirty"])[0]).to(DEV)
    keys = torch.from_numpy(sc["rows"]["key"]).to(DEV)[clean]
    assert 0 < len(dirty) < 0.05 * d["nd"]
    runs = [(KvRun, (n, mode, "one")), (KvRun, (n, mode, "two")), (KvRun, (n, mode, "both"))]
    runs += [(TokRun, (n, "plain"))] if mode == "plain" else [(TokRun, (n, "x3")), (TokRun, (n, "x3lo"))]
    for cls, args in runs:
        big, tab = cls("S5", *args), cls("S5e", *args)
        tab.check("table")
        big.check("many groups", sel=dirty, total_rows=d["nd"])
        for b, t in zip(big.rows() if cls is TokRun else [big.rows()], tab.rows() if cls is TokRun else [tab.rows()]):
            assert torch.equal(b[clean], t[keys]), (cls.__name__, args, "a clean cell's row differs from the table row of its key")
        del big, tab


# ------------------------------------------------------------------------------------------------
# rejections
# ------------------------------------------------------------------------------------------------
def test_rejections_leave_every_buffer_untouched():
    """Each documented refusal returns its code and writes nothing: the output, the workspace and its tail keep the pattern."""
    null = addr(None)
    kv_cases = [
        ("n = 384", dict(n_abi=384), "two", EUNSUPPORTED), ("c_in = 32", dict(c_in=32), "two", EUNSUPPORTED), ("ny = 20", dict(ny=20), "two", EUNSUPPORTED),
        ("k_fp16 without a workspace", dict(k16=1, ws=null, ws_bytes=0), "two", EUNSUPPORTED),
        ("t_f16 without a workspace", dict(t16=1, ws=null, ws_bytes=0), "two", EUNSUPPORTED),
        ("m_lo without r_lo", dict(r_lo=null), "two", EINVAL), ("n = 384, one launch", dict(n_abi=384), "one", EUNSUPPORTED),
    ]
    for label, over, form, code in kv_cases:
        r = KvRun("S1", 256, "x3", form, **over)
        assert r.rc == code, (label, r.rc)
        assert r.intact(0) and (r.ws is None or bool((r.ws == 0xA5).all())), label
    # the workspace: t rows hi and lo [cap_tiles * 64, 64] bf16, rstd and key [cap_tiles * 64] 4-byte words, each at a multiple of 256 bytes.
    # The query rounds that up and adds 256 bytes of slack (LvqSizer), so the refusal is at one byte short of what the layout needs.
    d = dev_scene("S1")
    need = 0
    for nbytes in (d["cap_tiles"] * 64 * 64 * 2, d["cap_tiles"] * 64 * 64 * 2, d["cap_tiles"] * 64 * 4, d["cap_tiles"] * 64 * 4):
        need = (need + 255) // 256 * 256 + nbytes
    r = KvRun("S1", 256, "x3", "two")
    assert r.rc == OK and need <= r.ws_bytes
    short = KvRun("S1", 256, "x3", "two", ws_bytes=need - 1)
    assert short.rc == EWORKSPACE and short.intact(0) and bool((short.ws == 0xA5).all())
    fits = KvRun("S1", 256, "x3", "two", ws_bytes=need)
    assert fits.rc == OK and fits.intact(d["nd"]) and bool((fits.ws[need:] == 0xA5).all()) and torch.equal(fits.rows(), r.rows())
    moved = Canary(torch.bfloat16, (d["cap_tiles"] * 64, 512), (512, 1), 65, 1024 + 64)     # the kv pointer one element off 16-byte alignment
    assert KvRun("S1", 256, "x3", "two", kv=moved.ptr()).rc == EUNSUPPORTED and moved.untouched(everything=True)
    for label, over, code in [("n = 384", dict(n_abi=384), EUNSUPPORTED), ("c_in = 32", dict(c_in=32), EUNSUPPORTED), ("ny = 20", dict(ny=20), EUNSUPPORTED)]:
        t = TokRun("S1", 256, "x3lo", **over)
        assert t.rc == code, (label, t.rc)
        assert t.intact(0), label
    moved = Canary(torch.bfloat16, (d["cap_tiles"] * 64, 256), (256, 1), 65, 512 + 64)
    assert TokRun("S1", 256, "x3", x=moved.ptr()).rc == EUNSUPPORTED and moved.untouched(everything=True)


def test_index_map_ignores_trailing_pillars():
    """S1 carries three pillar rows beyond n_live: lvq_pillar_index_map must not place them (the scenes above use the host's map)."""
    sc = BC.prepared("S1", cus())
    assert len(sc["coords"]) == sc["n_live"] + 3
    idx = ops().pillar_index_map(dev(sc["coords"]), torch.tensor([sc["n_live"]], dtype=torch.int32, device=DEV), 1, 24, 24)
    assert np.array_equal(idx.cpu().numpy(), sc["idx"])


# ------------------------------------------------------------------------------------------------
# one tie to the model: widths the pipeline never brings to the tile kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "mixed"])
@pytest.mark.parametrize("d_model", [512, 1024])
def test_model_fold_through_the_kernels(d_model, prec):
    """M, m0, R, r0, c0, T from VATLiDAR._kv_fold of a seeded module on S2 through the two-launch kernels: against tile_kv_ref on those
    same factors at the bound above, and against the unfolded chain of the ported model (conv -> proj -> LayerNorm -> + PE -> in_proj
    rows d .. 3d in fp64) at the fused-against-unfused bound of test_fused_kv_kernel_matches_token_kernel_plus_gemm (2^-7 max for
    mixed, 2^-6 max for bf16)."""
    from lidar_vision_vqa_amd import fusion, synth
    from oracle import vat_oracle as VO
    sc = BC.prepared("S2", cus())
    B, H, W, C, n = sc["B"], sc["H"], sc["W"], BC.C, d_model
    m = synth.load_seeded(fusion.VATLiDAR(C, n, n_queries=12, n_layers=1, n_heads=n // 64), 81).to(DEV).eval()
    m.precision = prec
    with torch.no_grad():
        r_bf, r0, c0, layers, _ = m._kv_fold(C, H, W, torch.device(DEV))
    m_bf, m0, tab = layers[0]
    assert tab.dtype == torch.float32
    mode = "plain" if prec == "bf16" else "x3"
    assert (m_bf[1] is not None) == (mode == "x3")
    ds = dev_scene("S2")
    nd, nl = ds["nd"], sc["n_live"]
    w9 = m.refine[0].weight.detach().reshape(C, 9).contiguous()
    b9 = m.refine[0].bias.detach().contiguous()
    t, mag = BO.conv_tokens(sc["feat"][:nl], sc["coords"][:nl], B, H, W, w9.cpu().numpy(), b9.cpu().numpy())
    rows = sc["rows"]
    t_rows, mag_rows = t[rows["s"], rows["y"], rows["x"]], mag[rows["s"], rows["y"], rows["x"]]
    share = BO.loose_share(t_rows, mag_rows, mode)
    L, f = F().lib(), F()
    out = Canary(torch.bfloat16, (ds["cap_tiles"] * 64, 2 * n), (2 * n, 1), 64, 4 * n + 64)
    ws_bytes = int(L.lvq_bev_tile_kv_workspace_bytes(f.i64(ds["cap_tiles"])))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    rc = L.lvq_bev_tile_kv(addr(ds["feat"]), addr(ds["idx"]), addr(ds["live"]), addr(ds["dirty"]), addr(ds["counts"]), f.i64(ds["cap_tiles"]), f.cint(B),
                           f.cint(H), f.cint(W), f.cint(C), addr(w9), addr(b9), addr(m_bf[0]), addr(m_bf[1]), addr(m0), addr(r_bf[0]), addr(r_bf[1]),
                           addr(r0), f.cfloat(c0), f.cint(n), f.cfloat(m.norm_tokens.eps), addr(tab), f.cint(0), f.cint(n), f.cint(0), out.ptr(),
                           addr(ws), f.csize(ws_bytes), f.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == OK and out.untouched() and rows_untouched(out, nd)
    got = out.result()[:nd].double().cpu().numpy()
    val = lambda p: (p[0].double() + (p[1].double() if p[1] is not None else 0.0)).cpu().numpy()
    M, R, T = val(m_bf), val(r_bf), tab.double().cpu().numpy()
    ref_fn = lambda t_op, keys: BO.kv_rows(t_op, keys, M, m0.double().cpu().numpy(), R, r0.double().cpu().numpy(), c0, n, m.norm_tokens.eps, T)
    a = A_PLAIN if mode == "plain" else A_X3
    res = BO.judge_rows(got, t_rows, mag_rows, rows["key"], mode, ref_fn, lambda ref, scale: BO.tight_bound(ref, scale, a))
    report(f"model fold d={n} {prec} (three-flag share of the inputs {100 * share:.3f} %)", res, nd)
    # the unfolded chain of the ported model
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    bev = torch.zeros(B, C, H, W, dtype=torch.float64)
    co = sc["coords"][:nl]
    bev[co[:, 0], :, co[:, 2], co[:, 3]] = torch.from_numpy(sc["feat"][:nl]).double()
    chain = VO.vat_lidar_kv(bev, sd).numpy()[rows["s"], rows["y"] * W + rows["x"]]
    err, amax = float(np.abs(got - chain).max()), float(np.abs(chain).max())
    bound = (2.0 ** -6 if prec == "bf16" else 2.0 ** -7) * amax
    print(f"model fold d={n} {prec}: against the unfolded fp64 chain err {err:.3e} (bound {bound:.3e}, max|ref| {amax:.3f})")
    assert err < bound, (err, bound)
