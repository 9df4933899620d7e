"""lvq_attention_relpos_bf16 (csrc/vit_attention.hip) through the C ABI against the fp64 restatement of its contract
(tests/vision_tower_cases.py: attention_ref, the shifted-table form of the decomposed relative-position bias).

Layout: the packed qkv matrix sits in an exactly sized buffer whose row stride is wider than 3 H dh, the padding filled with a large
value; the output has canary gaps behind every row, a head and a tail (the Canary / place helpers of tests/test_gpu_kernel_routes.py).

Bound, measured not assumed: on the same operands the parent's lvq_attention_bf16 is run with the bias materialised on the host
(fp64 -> fp32, [B, H, N, N]); both errors are taken against fp64 and the new kernel is held to
    err_new <= max(B, 2 err_parent)        B = 2e-4 for hi + lo operands, 2e-2 for plain ones (the bounds of test_gpu_kernel_routes.py)
The factor 2 covers the one thing the new kernel does that the parent does not: it forms the bias from 16-bit operands.  In the plain
form the reference sees the bf16-rounded operands (what the kernel multiplies), as everywhere in these tests.

Routes: k_attn_relpos<NSPLIT, STAGES> has four instantiations; check() prints which one a case launched, from the library's own route query
(lvq_attention_relpos_plan).  ROUTE_GRIDS lists every grid this file runs in both operand forms, and tests/test_vision_tower_restatements.py
holds that list to the route classes of the whole family.  Regimes beyond unit variance (VC.regime_operands, VC.one_hot_operands) use the
same RelRun and the same bound."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_kernel_routes as KR  # noqa: E402
import vision_tower_cases as VC  # noqa: E402

DEV = KR.DEV
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = KR.OK, KR.EINVAL, KR.EWORKSPACE, KR.EUNSUPPORTED
DH = 64
BOUND = {False: 2e-2, True: 2e-4}


class RelRun:
    """One lvq_attention_relpos_bf16 call on padded operands and canary outputs."""

    def __init__(self, batch, heads, gh, gw, split, *, dh=DH, seed=900, qkv=None, operands=None, expect=OK, ws_short=0, o_lo=None,
                 lo_given=None, ld_arg=None, ldo_arg=None, scale=None, shift=None):
        """`operands`: (qkv, rel_h, rel_w) host arrays in place of the seeded ones.  The deviations below change what the CALL is told,
        never the buffers, which are always real and fully sized (a refusal test's call, accepted by mistake, still runs in bounds):
          o_lo      True / False: give or withhold the lo output whatever `split` says          lo_given   per operand (qkv, rel_h, rel_w)
          ld_arg, ldo_arg, scale   passed in place of the buffers' own strides and 1 / sqrt(dh)  (strides only ever smaller)
          shift     {"qkv" | "rel_h" | "rel_w" | "o": elements}: that pointer is moved into its (enlarged) buffer by so many elements"""
        f = KR.F()
        self.dims, self.split = (batch, heads, gh, gw, dh), split
        n, d = gh * gw, heads * dh
        q32, rh32, rw32 = VC.kernel_operands(batch, heads, gh, gw, dh, seed) if operands is None else operands
        q32 = q32 if qkv is None else qkv
        self.host = tuple(torch.from_numpy(a) for a in (q32, rh32, rw32))
        dev = [t.to(DEV) for t in self.host]
        self.ld = ld = 3 * d + 40                                   # a multiple of 8, wider than the packed row
        parts = [KR.hi_lo(t) for t in dev]
        shift = shift or {}
        grow = lambda t: torch.cat((t.reshape(-1), t.new_full((16,), KR.PAD_VALUE)))            # room for a moved pointer
        self.qkv = [grow(KR.place(p, (ld, 1))) for p in parts[0]]
        self.tabs = [[grow(p.contiguous()) for p in parts[1]], [grow(p.contiguous()) for p in parts[2]]]
        given = (split,) * 3 if lo_given is None else lo_given
        at = lambda t, name, have=True: KR.addr(t if have else None, shift.get(name, 0) if have else 0)
        self.ldo = ldo = d + 24
        mk = lambda: KR.Canary(torch.bfloat16, (batch * n, d), (ldo, 1), 64, 2 * ldo + 64)
        self.o, self.ol = mk(), (mk() if (split if o_lo is None else o_lo) else None)
        L = f.lib()
        self.ws_bytes = int(L.lvq_attention_relpos_workspace_bytes(*(f.cint(v) for v in (batch, heads, gh, gw, dh, 3 if split else 1))))
        ws = torch.full((self.ws_bytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        nbytes = self.ws_bytes - ws_short
        assert (ld_arg is None or ld_arg <= ld) and (ldo_arg is None or ldo_arg <= ldo) and all(0 <= v <= 8 for v in shift.values())
        self.scale = 1.0 / math.sqrt(dh) if scale is None else scale
        self.rc = L.lvq_attention_relpos_bf16(
            at(self.qkv[0], "qkv"), at(self.qkv[1], "qkv", given[0]), f.i64(ld if ld_arg is None else ld_arg), at(self.tabs[0][0], "rel_h"),
            at(self.tabs[0][1], "rel_h", given[1]), at(self.tabs[1][0], "rel_w"), at(self.tabs[1][1], "rel_w", given[2]), f.cint(batch),
            f.cint(heads), f.cint(gh), f.cint(gw), f.cint(dh), f.cfloat(self.scale), KR.addr(self.o.t, self.o.head + shift.get("o", 0)),
            KR.addr(self.ol.t, self.ol.head + shift.get("o", 0)) if self.ol else KR.addr(None), f.i64(ldo if ldo_arg is None else ldo_arg),
            KR.addr(ws), f.csize(nbytes), f.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all()), "the workspace was written past the size that was passed"
        assert self.rc == expect, (self.dims, self.rc)
        if expect != OK:
            assert self.o.untouched(everything=True) and (self.ol is None or self.ol.untouched(everything=True)), "a refused call wrote to o"
        else:
            assert self.o.untouched() and (self.ol is None or self.ol.untouched()), "a store outside the attention result"

    def seen(self):
        """The operands as the kernel multiplies them: exact for hi + lo (to 2^-17), bf16-rounded in the plain form."""
        return tuple(t if self.split else KR.bf_round(t) for t in self.host)

    def got(self):
        g = self.o.result().float().cpu().double()
        return g + self.ol.result().float().cpu().double() if self.ol is not None else g

    def route(self):
        """What the call launched, from the library's own route query."""
        stages, lds = KR.F().attention_relpos_plan(self.dims[2], self.dims[3], 3 if self.split else 1)
        return f"k_attn_relpos<{3 if self.split else 1}, {stages}>, {lds} B LDS"

    def parent(self, bias):
        """The parent's route on the same operands: lvq_attention_bf16 with the dense fp32 bias [B, H, N, N]."""
        f = KR.F()
        batch, heads, gh, gw, dh = self.dims
        n, d, ld = gh * gw, heads * dh, self.ld
        L = f.lib()
        ws_bytes = int(L.lvq_attention_workspace_bytes(*(f.cint(v) for v in (batch, heads, n, n, dh, 3 if self.split else 1))))
        ws = torch.empty((ws_bytes + 256,), dtype=torch.uint8, device=DEV)
        o = torch.zeros((batch * n, d), dtype=torch.bfloat16, device=DEV)
        ol = torch.zeros_like(o) if self.split else None
        hi, lo = self.qkv
        part = lambda t, i: KR.addr(t, i * d) if t is not None and (self.split or t is hi) else KR.addr(None)
        st = (f.i64(n * ld), f.i64(ld), f.i64(dh))
        rc = L.lvq_attention_bf16(part(hi, 0), part(lo, 0), part(hi, 1), part(lo, 1), part(hi, 2), part(lo, 2), KR.addr(bias), f.cint(batch),
                                  f.cint(heads), f.cint(heads), f.cint(n), f.cint(n), f.cint(dh), *st, *st, *st, f.i64(n * d), f.i64(d), f.i64(dh),
                                  f.cfloat(self.scale), f.cint(0), KR.addr(o), KR.addr(ol), KR.addr(ws), f.csize(ws_bytes),
                                  f.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert rc == OK, rc
        g = o.float().cpu().double()
        return g + ol.float().cpu().double() if ol is not None else g

    def check(self, lo_carries=True):
        """`lo_carries=False`: for results that are exact in bf16 (o_lo == 0 everywhere), where hi alone is as close as hi + lo."""
        batch, heads, gh, gw, dh = self.dims
        n = gh * gw
        qkv, rh, rw = self.seen()
        scale = self.scale
        ref = torch.from_numpy(VC.attention_ref(qkv.numpy(), rh.numpy(), rw.numpy(), batch, heads, gh, gw, dh, scale))
        got = self.got()
        assert bool(torch.isfinite(got).all())
        q = qkv.view(batch, n, 3, heads, dh)[:, :, 0].permute(0, 2, 1, 3).contiguous()
        bias = torch.from_numpy(VC.dense_bias(q.numpy(), rh.numpy(), rw.numpy(), gh, gw)).float().contiguous().to(DEV)
        err_new = float((got - ref).abs().max())
        err_parent = float((self.parent(bias) - ref).abs().max())
        bound = max(BOUND[self.split], 2 * err_parent)
        print(f"relpos attention {self.dims} split={self.split} [{self.route()}]: err {err_new:.3e}, parent with dense bias {err_parent:.3e} "
              f"(bound {bound:.3e})")
        self.err, self.err_parent, self.ref = err_new, err_parent, ref
        assert err_new <= bound, (self.dims, err_new, err_parent)
        if self.ol is not None:                                     # the lo output is the residual of the hi output
            hi, lo = self.o.result(), self.ol.result()
            ulp = torch.ldexp(torch.ones_like(hi, dtype=torch.float32), torch.frexp(hi.float())[1] - 8)       # spacing of bf16 at hi
            assert bool((lo.float().abs() <= ulp / 2).all()), "o_lo exceeds half a unit in the last place of o"
            assert not lo_carries or float((hi.float().cpu().double() - ref).abs().max()) > err_new or err_new == 0.0
        return self


GRIDS = [(1, 1), (2, 3), (4, 4), (5, 7), (8, 8), (14, 14), (16, 16), (20, 20), (9, 33)]
# one grid and more per route of k_attn_relpos<NSPLIT, STAGES> (run with batch 1, one head: N up to 4032 keys)
LARGE_GRIDS = [(16, 63),        # plain: the smallest two-stage grid, waves span rows
               (50, 63),        # hi + lo: the smallest two-stage grid
               (64, 63),        # the largest LDS request of the family
               (63, 64),        # one-row waves, N not a power of two; plain two-stage
               (64, 17), (33, 50), (61, 61),
               (1, 64), (64, 1)]                # a one-entry table on one axis
# every grid this file runs in both precisions (tests/test_vision_tower_restatements.py holds it to the route classes of the family)
ROUTE_GRIDS = GRIDS + LARGE_GRIDS + [(64, 64)]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("batch,heads", [(1, 1), (3, 2)])
@pytest.mark.parametrize("gh,gw", GRIDS)
def test_grids(gh, gw, batch, heads, split):
    RelRun(batch, heads, gh, gw, split).check()


@pytest.mark.parametrize("split", [False, True])
def test_sam_window_shape(split):
    """25 windows x 12 heads of 14 x 14: one image's windowed block."""
    RelRun(25, 12, 14, 14, split).check()


@pytest.mark.parametrize("split", [False, True])
def test_global_grid_64(split):
    """The 64 x 64 grid of a global block (4096 keys, 254 table rows), batch 1, 2 heads."""
    RelRun(1, 2, 64, 64, split).check()


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("gh,gw", LARGE_GRIDS)
def test_large_grids_every_route(gh, gw, split):
    """The routes that GRIDS and the 64 x 64 grid do not reach (two K | V stages with waves that span grid rows, in both operand forms;
    the largest LDS request) and large grids whose width is no multiple of 16.  check() prints the instantiation from the route query."""
    RelRun(1, 1, gh, gw, split).check()


REGIME_GRIDS = [(14, 14), (16, 63)]             # 196 and 1008 keys: the last key tile holds 4 and 48 keys


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("gh,gw", REGIME_GRIDS)
@pytest.mark.parametrize("regime", VC.REGIMES)
def test_operand_regimes(regime, gh, gw, split):
    batch, heads = 2, 2
    ops = VC.regime_operands(regime, batch, heads, gh, gw, DH, 940)
    r = RelRun(batch, heads, gh, gw, split, operands=ops)
    qkv, rh, rw = (t.numpy() for t in r.seen())
    n, d = gh * gw, heads * DH
    if regime == "peaked_last":
        assert n % 64 != 0
        lg = VC.logits(qkv, rh, rw, batch, heads, gh, gw, DH, r.scale)
        margin = float((lg[..., -1] - lg[..., :-1].max(-1).values).min())
        print(f"{regime} {gh} x {gw}: the last key leads every row by at least {margin:.1f}")
        assert margin >= 30.0
    r.check()
    if regime == "tables_zero":                                     # fp64 plain attention, written out here
        t = torch.from_numpy(qkv).double().view(batch, n, 3, heads, DH).permute(2, 0, 3, 1, 4)
        plain = (torch.softmax((t[0] @ t[1].transpose(-1, -2)) * r.scale, -1) @ t[2]).permute(0, 2, 1, 3).reshape(batch * n, d)
        err = float((r.got() - plain).abs().max())
        print(f"{regime} {gh} x {gw} split={split}: vs plain fp64 attention {err:.3e}")
        assert err <= max(BOUND[split], 2 * r.err_parent)
    if regime == "bias_only":                                       # softmax(bias) v, written out with the dense gather
        t = torch.from_numpy(qkv).double().view(batch, n, 3, heads, DH).permute(2, 0, 3, 1, 4)
        ys, xs = torch.arange(n) // gw, torch.arange(n) % gw
        bh = torch.einsum("bhic,ijc->bhij", t[0], torch.from_numpy(rh).double()[ys[:, None] - ys[None, :] + gh - 1])
        bw = torch.einsum("bhic,ijc->bhij", t[0], torch.from_numpy(rw).double()[xs[:, None] - xs[None, :] + gw - 1])
        want = (torch.softmax(bh + bw, -1) @ t[2]).permute(0, 2, 1, 3).reshape(batch * n, d)
        err = float((r.got() - want).abs().max())
        print(f"{regime} {gh} x {gw} split={split}: vs softmax(gathered bias) v {err:.3e}")
        assert err <= max(BOUND[split], 2 * r.err_parent)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("gh,gw", REGIME_GRIDS)
def test_one_hot_offset_returns_the_key_at_that_offset(gh, gw, split):
    """VC.one_hot_operands: query (y, x) must return the v row of key (y - dy, x - dx), bit for bit in the hi output (p is exactly 1, the
    other keys' 4e-18 vanish beside it in fp32; v holds no zero in the channels it uses and is exact in bf16, so o_lo is 0), wherever
    that key exists; the other queries are held to fp64 like any case."""
    batch, heads = 2, 2
    n = gh * gw
    for dy, dx in ((0, 0), (1, -2), (-(gh - 1), gw - 1)):
        qkv, rh, rw, src = VC.one_hot_operands(batch, heads, gh, gw, DH, dy, dx)
        r = RelRun(batch, heads, gh, gw, split, operands=(qkv, rh, rw)).check(lo_carries=False)
        has = torch.from_numpy(src >= 0)
        assert int(has.sum()) == (gh - abs(dy)) * (gw - abs(dx)) >= 1
        v = torch.from_numpy(qkv).view(batch, n, 3, heads * DH)[:, :, 2].to(torch.bfloat16)
        want = v[:, torch.from_numpy(src).clamp(min=0)][:, has]
        got = r.o.result().cpu().view(batch, n, heads * DH)[:, has]
        wrong = int((got.view(torch.int16) != want.view(torch.int16)).any(-1).sum())
        print(f"one-hot ({dy}, {dx}) on {gh} x {gw} split={split}: {int(has.sum())} queries with a key, {wrong} rows differ")
        assert wrong == 0
        if split:
            assert not bool(r.ol.result().cpu().view(batch, n, -1)[:, has].float().any())


@pytest.mark.parametrize("batch,heads,gh,gw", [(3, 2, 5, 7), (3, 2, 14, 14), (1, 1, 50, 63)])
def test_hi_lo_operands_without_the_lo_output(batch, heads, gh, gw):
    """o_lo == NULL with hi + lo operands: the hi output is the one of the call that also asks for o_lo, bit for bit."""
    a, b = RelRun(batch, heads, gh, gw, True), RelRun(batch, heads, gh, gw, True, o_lo=False)
    assert a.ol is not None and b.ol is None
    assert torch.equal(a.o.result(), b.o.result())
    assert bool(a.o.result().float().abs().max() > 0.1)


@pytest.mark.parametrize("split", [False, True])
def test_invalid_and_unsupported_calls_launch_nothing(split):
    """Every refusal returns its code and writes nothing (RelRun holds both outputs' canaries, result range included), on real, fully
    sized buffers; the stream then takes a valid call."""
    g = (1, 2, 4, 4)
    d = 2 * DH
    real = RelRun(*g, split)
    RelRun(*g, split, expect=EINVAL, ld_arg=3 * d - 8)              # ld_qkv < 3 d
    RelRun(*g, split, expect=EINVAL, ldo_arg=d - 4)                 # ldo < d
    for given in ((True, False, False), (False, True, True), (True, True, False), (True, False, True)):
        RelRun(*g, split, expect=EINVAL, lo_given=given)            # lo for some of the operands only
    RelRun(*g, False, expect=EINVAL, o_lo=True)                     # o_lo without lo operands
    for scale in (0.0, -0.125, float("nan")):
        RelRun(*g, split, expect=EINVAL, scale=scale)
    RelRun(*g, split, expect=EUNSUPPORTED, ld_arg=real.ld - 4)      # ld_qkv % 8, still >= 3 d
    RelRun(*g, split, expect=EUNSUPPORTED, ldo_arg=real.ldo - 2)    # ldo % 4, still >= d
    assert (real.ld - 4) % 8 and real.ld - 4 >= 3 * d and (real.ldo - 2) % 4 and real.ldo - 2 >= d
    for name in ("qkv", "rel_h", "rel_w"):
        RelRun(*g, split, expect=EUNSUPPORTED, shift={name: 1})     # an operand pointer 2 bytes off
    RelRun(*g, split, expect=EUNSUPPORTED, shift={"o": 2})          # o (and o_lo) 4 bytes off: not 8-byte aligned
    again = RelRun(*g, split).check()
    assert torch.equal(again.o.result(), real.o.result())


@pytest.mark.parametrize("split", [False, True])
def test_refusals_launch_nothing(split):
    RelRun(1, 1, 4, 4, split, dh=80, expect=EUNSUPPORTED)
    RelRun(1, 1, 65, 2, split, expect=EUNSUPPORTED)
    RelRun(1, 1, 2, 65, split, expect=EUNSUPPORTED)
    r = RelRun(1, 2, 14, 14, split)
    if r.ws_bytes > 512:                                            # (the fused kernel keeps its table in LDS: the query is 0 today)
        RelRun(1, 2, 14, 14, split, expect=EWORKSPACE, ws_short=512)


@pytest.mark.parametrize("split", [False, True])
def test_determinism_and_batch_position(split):
    """Two identical calls are bit-equal, and a window's bits do not depend on its batch position: the same window at index 0 and at
    index 24 of a 25-window call."""
    heads, g = 2, 14
    n = g * g
    qkv = VC.kernel_operands(25, heads, g, g, DH, 900)[0].copy()
    qkv[24 * n:] = qkv[:n]
    a, b = RelRun(25, heads, g, g, split, qkv=qkv), RelRun(25, heads, g, g, split, qkv=qkv)
    for x, y in ((a.o, b.o), (a.ol, b.ol)):
        if x is not None:
            assert torch.equal(x.result(), y.result())
            assert torch.equal(x.result()[:n], x.result()[24 * n:])
            assert not torch.equal(x.result()[:n], x.result()[n:2 * n])
