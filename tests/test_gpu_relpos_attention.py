"""lvq_attention_relpos_bf16 (csrc/vit_attention.hip) through the C ABI against the fp64 restatement of its contract
(tests/vision_tower_cases.py: attention_ref, the shifted-table form of the decomposed relative-position bias).

Layout: the packed qkv matrix sits in an exactly sized buffer whose row stride is wider than 3 H dh, the padding filled with a large
value; the output has canary gaps behind every row, a head and a tail (the Canary / place helpers of tests/test_gpu_kernel_routes.py).

Bound, measured not assumed: on the same operands the parent's lvq_attention_bf16 is run with the bias materialised on the host
(fp64 -> fp32, [B, H, N, N]); both errors are taken against fp64 and the new kernel is held to
    err_new <= max(B, 2 err_parent)        B = 2e-4 for hi + lo operands, 2e-2 for plain ones (the bounds of test_gpu_kernel_routes.py)
The factor 2 covers the one thing the new kernel does that the parent does not: it forms the bias from 16-bit operands.  In the plain
form the reference sees the bf16-rounded operands (what the kernel multiplies), as everywhere in these tests."""
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

    def __init__(self, batch, heads, gh, gw, split, *, dh=DH, seed=900, qkv=None, expect=OK, ws_short=0):
        f = KR.F()
        self.dims, self.split = (batch, heads, gh, gw, dh), split
        n, d = gh * gw, heads * dh
        q32, rh32, rw32 = VC.kernel_operands(batch, heads, gh, gw, dh, seed)
        q32 = q32 if qkv is None else qkv
        self.host = tuple(torch.from_numpy(a) for a in (q32, rh32, rw32))
        dev = [t.to(DEV) for t in self.host]
        self.ld = ld = 3 * d + 40                                   # a multiple of 8, wider than the packed row
        parts = [KR.hi_lo(t) for t in dev]
        self.qkv = [KR.place(p, (ld, 1)) for p in parts[0]]
        self.tabs = [[p.contiguous() for p in parts[1]], [p.contiguous() for p in parts[2]]]
        lo = (lambda t: KR.addr(t)) if split else (lambda t: KR.addr(None))
        self.ldo = ldo = d + 24
        mk = lambda: KR.Canary(torch.bfloat16, (batch * n, d), (ldo, 1), 64, 2 * ldo + 64)
        self.o, self.ol = mk(), (mk() if split else None)
        L = f.lib()
        self.ws_bytes = int(L.lvq_attention_relpos_workspace_bytes(*(f.cint(v) for v in (batch, heads, gh, gw, dh, 3 if split else 1))))
        ws = torch.full((self.ws_bytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        nbytes = self.ws_bytes - ws_short
        self.rc = L.lvq_attention_relpos_bf16(
            KR.addr(self.qkv[0]), lo(self.qkv[1]), f.i64(ld), KR.addr(self.tabs[0][0]), lo(self.tabs[0][1]), KR.addr(self.tabs[1][0]),
            lo(self.tabs[1][1]), f.cint(batch), f.cint(heads), f.cint(gh), f.cint(gw), f.cint(dh), f.cfloat(1.0 / math.sqrt(dh)),
            self.o.ptr(), self.ol.ptr() if self.ol else KR.addr(None), f.i64(ldo), KR.addr(ws), f.csize(nbytes), f.stream_ptr(torch.device(DEV)))
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
                                  f.cfloat(1.0 / math.sqrt(dh)), f.cint(0), KR.addr(o), KR.addr(ol), KR.addr(ws), f.csize(ws_bytes),
                                  f.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert rc == OK, rc
        g = o.float().cpu().double()
        return g + ol.float().cpu().double() if ol is not None else g

    def check(self):
        batch, heads, gh, gw, dh = self.dims
        n = gh * gw
        qkv, rh, rw = self.seen()
        scale = 1.0 / math.sqrt(dh)
        ref = torch.from_numpy(VC.attention_ref(qkv.numpy(), rh.numpy(), rw.numpy(), batch, heads, gh, gw, dh, scale))
        got = self.got()
        assert bool(torch.isfinite(got).all())
        q = qkv.view(batch, n, 3, heads, dh)[:, :, 0].permute(0, 2, 1, 3).contiguous()
        bias = torch.from_numpy(VC.dense_bias(q.numpy(), rh.numpy(), rw.numpy(), gh, gw)).float().contiguous().to(DEV)
        err_new = float((got - ref).abs().max())
        err_parent = float((self.parent(bias) - ref).abs().max())
        bound = max(BOUND[self.split], 2 * err_parent)
        print(f"relpos attention {self.dims} split={self.split}: err {err_new:.3e}, parent with dense bias {err_parent:.3e} (bound {bound:.3e})")
        assert err_new <= bound, (self.dims, err_new, err_parent)
        if self.ol is not None:                                     # the lo output is the residual of the hi output
            hi, lo = self.o.result(), self.ol.result()
            ulp = torch.ldexp(torch.ones_like(hi, dtype=torch.float32), torch.frexp(hi.float())[1] - 8)       # spacing of bf16 at hi
            assert bool((lo.float().abs() <= ulp / 2).all()), "o_lo exceeds half a unit in the last place of o"
            assert float((hi.float().cpu().double() - ref).abs().max()) > err_new or err_new == 0.0
        return self


GRIDS = [(1, 1), (2, 3), (4, 4), (5, 7), (8, 8), (14, 14), (16, 16), (20, 20), (9, 33)]


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
