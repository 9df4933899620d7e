"""lvq_clip_embed through the C ABI: LayerNorm(cat(cls, feat^T) + pos) on channel-major patch features, and feat^T as a bf16 operand.

Shapes (batch, c, gh x gw): hw = 1; hw not a multiple of the 16-token tile; tiles that straddle images (5 images of 16 tokens start
at token offsets that a tile of any size up to 16 crosses only when hw is not a multiple of it -- 9 and 25 tokens per image do, and
(5, 128, 4 x 4) covers tiles smaller than an image); c at both ends of the family (64, 2048); the CLIP-L shape (1024, 16 x 16).

`hidden` against fp64 is held to  err <= max(B, 2 err_parent)  per element, where the parent is what the kernel replaces -- the same
rows assembled by torch (transpose, cat, position add) and passed to lvq_layernorm -- and B is the LayerNorm bound of
tests/test_gpu_head_kernels.py (norm_bound) at that d, evaluated on the fp64 rows.
tok_hi / tok_lo must be lvq_cast_bf16 of the permuted array bit for bit."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from lidar_vision_vqa_amd import synth  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
EPS = 1e-5
SHAPES = [(1, 64, 1, 1), (2, 128, 3, 3), (3, 192, 5, 5), (2, 2048, 2, 3), (1, 1024, 16, 16), (5, 128, 4, 4)]


def F():
    from lidar_vision_vqa_amd import _ffi
    return _ffi


def addr(t, off=0):
    return ctypes.c_void_p(0 if t is None else t.data_ptr() + off * t.element_size())


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(synth.randn(tuple(shape), seed, scale))


def inputs(b, c, hw):
    """feat with a per-image and per-channel offset (a row from the wrong image or a wrong channel moves the mean), cls ~ N(0, 1),
    pos ~ N(0, 0.5^2), gamma ~ 1 + 0.1 N, beta ~ 0.1 N."""
    feat = rnd((b, c, hw), 31) + torch.arange(b).view(b, 1, 1) * 0.5 + rnd((1, c, 1), 32)
    return dict(feat=feat, cls=rnd((c,), 33), pos=rnd((1 + hw, c), 34, 0.5), gamma=1.0 + rnd((c,), 35, 0.1), beta=rnd((c,), 36, 0.1))


def norm_bound(y, xin, gamma):
    """tests/test_gpu_head_kernels.py: norm_bound (LayerNorm form), on fp64 rows."""
    d = xin.shape[1]
    c = (d / 64 + 8) * U
    xc = xin - xin.mean(-1, keepdim=True)
    rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + EPS)
    shift = c * xin.abs().amax(-1, keepdim=True) * rstd * gamma.double().abs().max()
    return c * y.abs().amax(-1, keepdim=True) + shift + 4 * U * y.abs() + 1e-30


def call(t, b, c, hw, hidden, tok_hi=None, tok_lo=None, ld_tok=None, **over):
    f = F()
    a = dict(feat=t["feat"], cls=t["cls"], pos=t["pos"], gamma=t["gamma"], beta=t["beta"])
    a.update(over)
    rc = f.lib().lvq_clip_embed(addr(a["feat"]), addr(a["cls"]), addr(a["pos"]), addr(a["gamma"]), addr(a["beta"]), f.cfloat(EPS), f.cint(b),
                                f.cint(c), f.cint(hw), addr(hidden), addr(tok_hi), addr(tok_lo), f.i64(c if ld_tok is None else ld_tok),
                                f.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("b,c,gh,gw", SHAPES)
def test_hidden_and_operand_rows(b, c, gh, gw):
    f = F()
    hw = gh * gw
    host = inputs(b, c, hw)
    t = {k: v.to(DEV) for k, v in host.items()}
    assert f.lib().lvq_clip_embed_ok(b, c, hw) == 1
    # fp64 reference, and the rows as torch assembles them in fp32 (what lvq_layernorm is given)
    rows64 = torch.cat((host["cls"].double().expand(b, 1, c), host["feat"].double().transpose(1, 2)), 1) + host["pos"].double()
    rows64 = rows64.reshape(-1, c)
    mu = rows64.mean(-1, keepdim=True)
    ref = (rows64 - mu) * torch.rsqrt(((rows64 - mu) ** 2).mean(-1, keepdim=True) + EPS) * host["gamma"].double() + host["beta"].double()
    tokens = t["feat"].transpose(1, 2).contiguous()                                        # [b, hw, c]
    rows32 = (torch.cat((t["cls"].expand(b, 1, c), tokens), 1) + t["pos"]).reshape(-1, c).contiguous()
    parent = torch.full_like(rows32, float("nan"))
    f.check(f.lib().lvq_layernorm(addr(rows32), addr(None), 0, 1, addr(t["gamma"]), addr(t["beta"]), f.cfloat(EPS), f.i64(rows32.shape[0]),
                                  f.cint(c), addr(None), f.i64(0), addr(parent), addr(None), addr(None), f.stream_ptr(torch.device(DEV))),
            "lvq_layernorm")
    for split in (False, True):
        hidden = torch.full((b * (1 + hw), c), float("nan"), device=DEV)
        hi = torch.full((b * hw, c), float("nan"), dtype=torch.bfloat16, device=DEV)
        lo = torch.full((b * hw, c), float("nan"), dtype=torch.bfloat16, device=DEV) if split else None
        assert call(t, b, c, hw, hidden, hi, lo) == 0
        bnd = norm_bound(ref, rows64, host["gamma"])
        err = (hidden.cpu().double() - ref).abs()
        err_parent = (parent.cpu().double() - ref).abs()
        lim = torch.maximum(bnd, 2 * err_parent)
        print(f"({b}, {c}, {gh} x {gw}) split={split}: hidden max err {float(err.max()):.3e}, parent {float(err_parent.max()):.3e}, "
              f"max err / bound {float((err / bnd).max()):.3f}, class rows {float(err.view(b, 1 + hw, c)[:, 0].max()):.3e}")
        assert bool((err <= lim).all()), float((err / lim).max())
        want_hi, want_lo = torch.empty_like(hi), torch.empty_like(hi)
        f.check(f.lib().lvq_cast_bf16(addr(tokens), f.i64(tokens.numel()), addr(want_hi), addr(want_lo), f.stream_ptr(torch.device(DEV))), "lvq_cast_bf16")
        torch.cuda.synchronize()
        assert torch.equal(hi.view(torch.int16), want_hi.view(torch.int16)), "tok_hi != lvq_cast_bf16(feat^T)"
        if split:
            assert torch.equal(lo.view(torch.int16), want_lo.view(torch.int16)), "tok_lo != lvq_cast_bf16(feat^T) lo part"
    # hidden alone (no operand rows) is the same array
    h2 = torch.full_like(hidden, float("nan"))
    assert call(t, b, c, hw, h2) == 0 and torch.equal(h2, hidden)


def test_wide_operand_rows_leave_the_padding_alone():
    b, c, hw, ld = 3, 128, 9, 128 + 24
    t = {k: v.to(DEV) for k, v in inputs(b, c, hw).items()}
    hidden = torch.empty((b * (1 + hw), c), device=DEV)
    hi = torch.full((b * hw, ld), -7.0, dtype=torch.bfloat16, device=DEV)
    lo = torch.full((b * hw, ld), -7.0, dtype=torch.bfloat16, device=DEV)
    assert call(t, b, c, hw, hidden, hi, lo, ld_tok=ld) == 0
    tokens = t["feat"].transpose(1, 2).reshape(b * hw, c)
    want = tokens.to(torch.bfloat16)
    assert torch.equal(hi[:, :c], want) and torch.equal(lo[:, :c], (tokens - want.float()).to(torch.bfloat16))
    assert bool((hi[:, c:] == -7.0).all()) and bool((lo[:, c:] == -7.0).all())


@pytest.mark.parametrize("b,c,hw,ld,want", [(2, 96, 9, None, -5), (2, 2112, 4, None, -5), (2, 32, 4, None, -5), (2, 128, 9, 120, -5),
                                            (2, 128, 9, 131, -5), (0, 128, 9, None, -1), (2, 128, 0, None, -1)])
def test_refusals_leave_the_outputs_untouched(b, c, hw, ld, want):
    f = F()
    bb, hh = max(b, 1), max(hw, 1)
    t = {k: v.to(DEV) for k, v in inputs(bb, c, hh).items()}
    if want == -5 and ld is None:
        assert f.lib().lvq_clip_embed_ok(b, c, hw) == 0
    hidden = torch.full((bb * (1 + hh), c), -7.0, device=DEV)
    width = max(c, ld or c)
    hi = torch.full((bb * hh, width), -7.0, dtype=torch.bfloat16, device=DEV)
    lo = torch.full((bb * hh, width), -7.0, dtype=torch.bfloat16, device=DEV)
    assert call(t, b, c, hw, hidden, hi, lo, ld_tok=ld) == want
    assert bool((hidden == -7.0).all()) and bool((hi == -7.0).all()) and bool((lo == -7.0).all())


def test_lo_without_hi_and_misaligned_pointers_are_refused():
    b, c, hw = 2, 128, 9
    t = {k: v.to(DEV) for k, v in inputs(b, c, hw).items()}
    hidden = torch.full((b * (1 + hw), c), -7.0, device=DEV)
    lo = torch.full((b * hw, c), -7.0, dtype=torch.bfloat16, device=DEV)
    assert call(t, b, c, hw, hidden, None, lo) == -1
    big = torch.full((b * c * hw + 4,), 1.0, device=DEV)
    f = F()
    rc = f.lib().lvq_clip_embed(addr(big, 1), addr(t["cls"]), addr(t["pos"]), addr(t["gamma"]), addr(t["beta"]), f.cfloat(EPS), f.cint(b), f.cint(c),
                                f.cint(hw), addr(hidden), addr(None), addr(None), f.i64(c), f.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == -5 and bool((hidden == -7.0).all()) and bool((lo == -7.0).all())
