"""GPU tests of the decoder-head half of include/lvq.h, entry point by entry point through the C ABI, against fp64 restatements on
the host: the bf16 hand-off (lvq_cast_bf16, lvq_bf16_to_f32), lvq_rmsnorm / lvq_layernorm on all three of their paths, the rotary
embedding, SwiGLU, scale-add, cross entropy, the column sums of the per-step all-reduce, the argmax of greedy decoding, and
lvq_qwen2_decode_step at the reference decoder's geometry (oracle/decoder_oracle.py, pinned against transformers by
tests/test_oracle_decoder.py).

House rule of test_gpu_fusion.py: operands are pre-rounded to what the kernel sees, so only the order of fp32 accumulation can
differ from the reference, and the bars are bounds on that.  Outputs that one call writes in fp32 and in bf16 together are checked
against each other bit for bit (hi == RNE(y32), lo == RNE(y32 - hi)); the library builds with -ffp-contract=off, so kernels that are
one fp32 expression are checked bit for bit against the same expression in torch."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from oracle import decoder_oracle as DO  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24                       # fp32 unit roundoff
LVQ_EWORKSPACE = -2


def L():
    return F.lib()


def st():
    return F.stream_ptr(torch.device(DEV))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rne(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 round-to-nearest-even (torch's own cast), on the host."""
    return x.float().cpu().to(torch.bfloat16)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit-identical, except that any NaN matches any NaN."""
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(a.float()) & torch.isnan(b.float())
    ia = a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32)
    ib = b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32)
    return bool(((ia == ib) | nan).all())


def bf16_pair(x32: torch.Tensor):
    """(hi, lo) of an fp32 host tensor as the kernels write them: hi = RNE(x), lo = RNE(x - hi)."""
    hi = rne(x32)
    return hi, rne(x32 - hi.float())


# ------------------------------------------------------------------------------------------------
# 1. bf16 hand-off
# ------------------------------------------------------------------------------------------------
_CRAFTED = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # exact ties: to even downwards (1.0) and upwards (0x3f82)
            0x3F808001, 0x3F807FFF, 0x00000000, 0x80000000,      # just past / just short of a tie, +0, -0
            0x00000001, 0x00008000, 0x00018000, 0x807FFFFF,      # subnormals (ties among them too), largest negative subnormal
            0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001,      # +-inf, quiet and signalling NaN
            0xFFC00001, 0x7FFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF,      # NaNs with payload, largest finite (-> +-inf)
            0x7F7F7FFF, 0x7F7F8000, 0x00800000, 0x3F800000]      # below the last tie, the tie into inf, smallest normal, 1.0


def _crafted(n, seed):
    """[n] fp32 host tensors that hold every crafted value, at the start and at the end (the scalar tail) where n allows."""
    c = torch.tensor(np.array(_CRAFTED, dtype=np.uint32).view(np.int32)).view(torch.float32)
    out = []
    for i in range(0, len(c), n) if n < 2 * len(c) else [0]:
        x = torch.randn(n, generator=gen(seed + i)) * 3.0
        if n < 2 * len(c):
            k = min(n, len(c) - i)
            x[:k] = c[i:i + k]
        else:
            x[:len(c)] = c
            x[-len(c):] = c.flip(0)
        out.append(x)
    return out


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025])
def test_cast_bf16_rounding(n):
    for x in _crafted(n, n):
        xd = x.to(DEV)
        hi = torch.empty(n, dtype=torch.bfloat16, device=DEV)
        lo = torch.empty(n, dtype=torch.bfloat16, device=DEV)
        hi_only = torch.empty(n, dtype=torch.bfloat16, device=DEV)
        F.check(L().lvq_cast_bf16(F.ptr(xd), F.i64(n), F.ptr(hi), F.ptr(lo), st()), "lvq_cast_bf16")
        F.check(L().lvq_cast_bf16(F.ptr(xd), F.i64(n), F.ptr(hi_only), F.ptr(None), st()), "lvq_cast_bf16")
        want_hi, want_lo = bf16_pair(x)
        assert same_bits(hi, want_hi) and same_bits(hi_only, want_hi)
        assert bool((torch.isnan(hi.cpu().float()) == torch.isnan(x)).all())             # NaN stays NaN, nothing else becomes one
        assert same_bits(lo, want_lo)
        fin = torch.isfinite(hi.cpu().float())
        back = hi.cpu().double() + lo.cpu().double()
        err = (back - x.double()).abs()[fin]
        assert bool((err <= 2.0 ** -16 * x.double().abs()[fin] + 2.0 ** -133).all())


def test_bf16_to_f32_alpha():
    n = 1029
    x = torch.randn(n, generator=gen(3)) * 50.0
    x[:4] = torch.tensor([0.0, -0.0, 1e-39, -3e38])
    hi, lo = (t.to(DEV) for t in bf16_pair(x))
    for alpha in (0.3, -1.75):
        for use_lo in (False, True):
            out = torch.full((n,), float("nan"), device=DEV)
            F.check(L().lvq_bf16_to_f32(F.ptr(hi), F.ptr(lo if use_lo else None), F.i64(n), F.cfloat(alpha), F.ptr(out), st()), "lvq_bf16_to_f32")
            want = (hi.cpu().float() + (lo.cpu().float() if use_lo else 0.0)) * torch.tensor(alpha, dtype=torch.float32)
            assert same_bits(out, want), (alpha, use_lo)


# ------------------------------------------------------------------------------------------------
# 2. RMSNorm / LayerNorm
# ------------------------------------------------------------------------------------------------
def norm_ref(x, gamma, beta, eps, rms, add=None, add_group=1, post=None):
    x = x.double()
    r = torch.arange(x.shape[0])
    if add is not None:
        x = x + add.double()[(r // add_group) % add.shape[0]]
    if rms:
        y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * gamma.double()
        return y, x
    mu = x.mean(-1, keepdim=True)
    y = (x - mu) * torch.rsqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps) * gamma.double()
    if beta is not None:
        y = y + beta.double()
    if post is not None:
        y = y + post.double()[r % post.shape[0]]
    return y, x


def norm_bound(y, xin, gamma, rms):
    """Per-row bound on the fp32 error: lanes sum d/64 terms and a wave reduction adds 6 levels, so the mean moves by at most
    (d/64 + 8) u max|x| and the variance by (d/64 + 8) u of itself; two ulps for the output expression."""
    d = xin.shape[1]
    c = (d / 64 + 8) * U
    xc = xin if rms else xin - xin.mean(-1, keepdim=True)
    rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    shift = 0.0 if rms else c * xin.abs().amax(-1, keepdim=True) * rstd * gamma.double().abs().max()
    return c * y.abs().amax(-1, keepdim=True) + shift + 4 * U * y.abs() + 1e-30


def run_norm(rms, x, gamma, beta, eps, out32, hi, lo, add=None, add_group=1, post=None):
    rows, d = x.shape[0], gamma.shape[0]
    if rms:
        rc = L().lvq_rmsnorm(F.ptr(x), F.ptr(gamma), F.cfloat(eps), F.i64(rows), F.cint(d), F.ptr(out32), F.ptr(hi), F.ptr(lo), st())
    else:
        rc = L().lvq_layernorm(F.ptr(x), F.ptr(add), F.cint(add.shape[0] if add is not None else 0), F.cint(add_group), F.ptr(gamma), F.ptr(beta),
                               F.cfloat(eps), F.i64(rows), F.cint(d), F.ptr(post), F.i64(post.shape[0] if post is not None else 0), F.ptr(out32),
                               F.ptr(hi), F.ptr(lo), st())
    F.check(rc, "lvq_rmsnorm" if rms else "lvq_layernorm")


def check_norm(rms, x, gamma, beta, eps, add=None, add_group=1, post=None, x_dev=None, tag=""):
    """Every output form of one norm call against the fp64 reference; returns the fp32 output."""
    rows, d = x.shape
    xd = x.to(DEV) if x_dev is None else x_dev
    g, b = gamma.to(DEV), (beta.to(DEV) if beta is not None else None)
    a = add.to(DEV) if add is not None else None
    p = post.to(DEV) if post is not None else None
    nan32 = lambda: torch.full((rows, d), float("nan"), device=DEV)
    nan16 = lambda: torch.full((rows, d), float("nan"), dtype=torch.bfloat16, device=DEV)
    y32, hi, lo = nan32(), nan16(), nan16()
    run_norm(rms, xd, g, b, eps, y32, hi, lo, a, add_group, p)                    # all three outputs at once
    ref, xin = norm_ref(x, gamma, beta, eps, rms, add, add_group, post)
    got = y32.cpu()
    assert bool(((got.double() - ref).abs() <= norm_bound(ref, xin, gamma, rms)).all()), (tag, float((got.double() - ref).abs().max()))
    h, l = bf16_pair(got)
    assert same_bits(hi, h) and same_bits(lo, l), tag                             # hi == RNE(y32), lo == RNE(y32 - hi)
    o32 = nan32()
    run_norm(rms, xd, g, b, eps, o32, None, None, a, add_group, p)                # fp32 only
    ohi = nan16()
    run_norm(rms, xd, g, b, eps, None, ohi, None, a, add_group, p)                # bf16 only
    ohi2, olo2 = nan16(), nan16()
    run_norm(rms, xd, g, b, eps, None, ohi2, olo2, a, add_group, p)               # bf16 + lo
    assert same_bits(o32, y32) and same_bits(ohi, hi) and same_bits(ohi2, hi) and same_bits(olo2, lo), tag
    return got


NORM_DS = [64, 200, 768, 896, 2048, 2304, 4864]      # vector path (768, 2048), registers (64, 200, 896), re-read (2304, 4864)


@pytest.mark.parametrize("d", NORM_DS)
@pytest.mark.parametrize("rms", [True, False])
def test_norm_paths_and_output_forms(d, rms):
    g = gen(d + rms)
    gamma = 1.0 + 0.3 * torch.randn(d, generator=g)
    beta = torch.randn(d, generator=g)
    for rows in (1, 3, 4, 5, 1000):
        x = torch.randn(rows, d, generator=g) * 2.0
        x[-1] += 300.0                                          # a large common offset: the variance is centred before squaring
        check_norm(rms, x, gamma, None if rms else beta, 1e-5 if not rms else 1e-6, tag=(d, rows))


@pytest.mark.parametrize("d", [200, 768, 2304])
def test_layernorm_add_group_post_and_no_beta(d):
    g = gen(100 + d)
    rows = 37
    x = torch.randn(rows, d, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(d, generator=g)
    beta = torch.randn(d, generator=g)
    add = torch.randn(6, d, generator=g) * 3.0
    post = torch.randn(5, d, generator=g)
    for group in (1, 4, 7):
        check_norm(False, x, gamma, beta, 1e-5, add=add, add_group=group, tag=("add", group))
    check_norm(False, x, gamma, None, 1e-5, tag="no beta")
    check_norm(False, x, gamma, None, 1e-5, add=add, add_group=3, post=post, tag="add + post, no beta")
    check_norm(False, x + 500.0, gamma, beta, 1e-5, post=post, tag="offset + post")


@pytest.mark.parametrize("rms", [True, False])
def test_norm_misaligned_rows_take_the_scalar_path(rms):
    """d = 768 from a base one float past a 16-byte boundary: launch_norm_vec declines, k_norm runs; same numbers to fp32 rounding."""
    d, rows = 768, 9
    g = gen(7)
    x = torch.randn(rows, d, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(d, generator=g)
    beta = None if rms else torch.randn(d, generator=g)
    store = torch.empty(rows * d + 4, device=DEV)
    xm = store[1:1 + rows * d].view(rows, d)
    xm.copy_(x.to(DEV))
    assert xm.data_ptr() % 16 == 4
    ym = check_norm(rms, x, gamma, beta, 1e-5, x_dev=xm, tag="misaligned")
    ya = check_norm(rms, x, gamma, beta, 1e-5, tag="aligned")
    assert float((ym - ya).abs().max()) <= 64 * U * float(ya.abs().max())


# ------------------------------------------------------------------------------------------------
# 3. rotary embedding on the packed q|k|v rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("pos0", [0, 879, 32000])
@pytest.mark.parametrize("theta", [1e4, 1e6])
def test_rope_packed_qkv(dh, pos0, theta):
    H, Hk, seq, nseq = 14, 2, 5, 3
    d, dkv = H * dh, Hk * dh
    ld, rows = d + 2 * dkv, nseq * seq
    x = torch.randn(rows, ld, generator=gen(dh + pos0)) * 2.0
    pos = pos0 + torch.arange(rows) % seq
    for split in (False, True):
        h0, l0 = bf16_pair(x)
        hi, lo = h0.to(DEV), (l0.to(DEV) if split else None)
        for c0, nh in ((0, H), (d, Hk)):                 # q heads, then k heads: column slices of the same rows
            sh = ctypes.c_void_p(hi.data_ptr() + 2 * c0)
            sl = ctypes.c_void_p(lo.data_ptr() + 2 * c0) if split else F.ptr(None)
            if pos0 == 0:
                rc = L().lvq_rope_inplace(sh, sl, F.i64(rows), F.cint(seq), F.cint(nh), F.cint(dh), F.i64(ld), F.cfloat(theta), st())
            else:
                rc = L().lvq_rope_inplace_at(sh, sl, F.i64(rows), F.cint(seq), F.cint(pos0), F.cint(nh), F.cint(dh), F.i64(ld), F.cfloat(theta), st())
            F.check(rc, "lvq_rope_inplace")
        a = h0.double() + (l0.double() if split else 0.0)
        ang = DO.rope_angles(pos, dh, theta)[:, None]
        want = torch.cat((DO.rope(a[:, :d].view(rows, H, dh), ang).view(rows, d), DO.rope(a[:, d:d + dkv].view(rows, Hk, dh), ang).view(rows, dkv)), 1)
        got = hi.cpu().double()[:, :d + dkv] + (lo.cpu().double()[:, :d + dkv] if split else 0.0)
        av = a[:, :d + dkv].view(rows, H + Hk, dh)
        pair = av[..., :dh // 2].abs() + av[..., dh // 2:].abs()                 # |a| + |b| of every element's rotation pair
        pair = torch.cat((pair, pair), -1).view(rows, d + dkv)
        # plain: the bf16 rounding of the output; lo: 2^-16 of it.  Both: fp32 rotation and sincosf, a few ulps of |a| + |b|.  An ulp of
        # inv_freq away from transformers' frequencies moves the angle by pos * 6e-8: 2e-3 rad at 32000, 5e-5 rad at 879.
        bar = (2.0 ** -16 if split else 2.0 ** -8) * want.abs() + 1e-6 * pair + 1e-30
        assert bool(((got - want).abs() <= bar).all()), (split, float(((got - want).abs() / pair.clamp_min(1e-30)).max()))
        assert same_bits(hi[:, d + dkv:], h0[:, d + dkv:])                    # v columns untouched
        if split:
            assert same_bits(lo[:, d + dkv:], l0[:, d + dkv:])
    if pos0 == 0:                                                                 # _at at position 0 is the prefill form
        h1, h2 = (rne(x).to(DEV) for _ in range(2))
        F.check(L().lvq_rope_inplace(F.ptr(h1), F.ptr(None), F.i64(rows), F.cint(seq), F.cint(H), F.cint(dh), F.i64(ld), F.cfloat(theta), st()), "rope")
        F.check(L().lvq_rope_inplace_at(F.ptr(h2), F.ptr(None), F.i64(rows), F.cint(seq), F.cint(0), F.cint(H), F.cint(dh), F.i64(ld), F.cfloat(theta),
                                        st()), "rope_at")
        assert same_bits(h1, h2)


# ------------------------------------------------------------------------------------------------
# 4. SwiGLU, scale-add
# ------------------------------------------------------------------------------------------------
def test_swiglu_full_gate_range():
    rows, inter = 6, 4864
    g = gen(11)
    gate = torch.rand(rows, inter, generator=g) * 180.0 - 90.0                   # [-90, 90]: expf(-g) overflows below -88.72
    gate[0, :8] = torch.tensor([-90.0, -89.0, -88.8, -88.7, -87.0, 0.0, -0.0, 90.0])
    up = torch.randn(rows, inter, generator=g) * 2.0
    gu = torch.cat((gate, up), 1).to(DEV)
    want = DO.silu(gate.double()) * up.double()
    for split in (False, True):
        hi = torch.full((rows, inter), float("nan"), dtype=torch.bfloat16, device=DEV)
        lo = torch.full((rows, inter), float("nan"), dtype=torch.bfloat16, device=DEV) if split else None
        F.check(L().lvq_swiglu(F.ptr(gu), F.i64(rows), F.cint(inter), F.ptr(hi), F.ptr(lo), st()), "lvq_swiglu")
        got = hi.cpu().double() + (lo.cpu().double() if split else 0.0)
        assert bool(torch.isfinite(got).all())
        bar = ((2.0 ** -16 if split else 2.0 ** -8) + 8 * U) * want.abs() + 1e-35
        assert bool(((got - want).abs() <= bar).all()), split


def test_scale_add_rows_bitwise():
    rows, d, add_rows, alpha = 23, 200, 7, 0.7                                    # 7 does not divide 23
    g = gen(12)
    x = torch.randn(rows, d, generator=g) * 5.0
    add = torch.randn(add_rows, d, generator=g)
    a32 = torch.tensor(alpha, dtype=torch.float32)
    xd, ad = x.to(DEV), add.to(DEV)
    for use_add in (True, False):
        out = torch.full((rows, d), float("nan"), device=DEV)
        F.check(L().lvq_scale_add_rows(F.ptr(xd), F.ptr(ad if use_add else None), F.i64(add_rows if use_add else 0), F.cfloat(alpha),
                                       F.i64(rows), F.cint(d), F.ptr(out), st()), "lvq_scale_add_rows")
        want = x * a32 + (add[torch.arange(rows) % add_rows] if use_add else 0.0)
        assert same_bits(out, want), use_add


# ------------------------------------------------------------------------------------------------
# 5. cross entropy
# ------------------------------------------------------------------------------------------------
def run_ce(logits, labels):
    acc = torch.zeros(2, device=DEV)
    F.check(L().lvq_cross_entropy(F.ptr(logits), F.ptr(labels), F.i64(logits.shape[0]), F.cint(logits.shape[1]), F.ptr(acc), st()),
            "lvq_cross_entropy")
    return acc.cpu()


@pytest.mark.parametrize("vocab,rows", [(512, 40), (8192, 40), (151936, 48)])
def test_cross_entropy(vocab, rows):
    g = gen(vocab)
    logits = torch.randn(rows, vocab, generator=g) * 2.0
    logits[1:6] *= 25.0                                                            # peaked rows (logit scale 50)
    logits[6] = 3.0                                                                # a constant row: loss = log V
    labels = torch.randint(0, vocab, (rows,), generator=g)
    labels[[2, 9, 17]] = -100
    labels[3] = logits[3].argmax()                                                 # a peaked row whose label is its peak
    labels[4], labels[5] = 0, vocab - 1
    acc = run_ce(logits.to(DEV), labels.to(DEV))
    keep = labels >= 0
    lse = torch.logsumexp(logits.double(), -1)
    per = lse - logits.double().gather(1, labels.clamp_min(0)[:, None])[:, 0]
    want = float(per[keep].sum())
    assert float(acc[1]) == float(keep.sum())
    assert abs(float(acc[0]) - want) <= 1e-5 * abs(want), (float(acc[0]), want)
    one = run_ce(logits[6:7].contiguous().to(DEV), labels[6:7].contiguous().to(DEV))
    assert float(one[1]) == 1.0 and abs(float(one[0]) - math.log(vocab)) <= 1e-5 * math.log(vocab)
    none = run_ce(logits.to(DEV), torch.full((rows,), -100, dtype=torch.int64, device=DEV))
    assert float(none[0]) == 0.0 and float(none[1]) == 0.0                         # an all-ignored batch


# ------------------------------------------------------------------------------------------------
# 6. column sums (the per-step all-reduce payload)
# ------------------------------------------------------------------------------------------------
def colsum(x, rows, d, ws_bytes=None):
    need = int(L().lvq_colsum_workspace_bytes(F.i64(rows), F.cint(d)))
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=DEV)
    out = torch.full((d,), float("nan"), device=DEV)
    rc = L().lvq_colsum(F.ptr(x), F.i64(rows), F.cint(d), F.ptr(out), F.ptr(ws), F.csize(nb), st())
    return rc, out, need


@pytest.mark.parametrize("rows", [0, 1, 17, 4095, 4096, 18432, 100000])
def test_colsum_fixed_order(rows):
    g = torch.Generator(device=DEV).manual_seed(rows)
    for d in (1, 63, 64, 768, 1000):
        x = torch.randn(rows, d, device=DEV, generator=g) + 0.5                    # a mean: a dropped partial is visible
        rc, out, need = colsum(x, rows, d)
        F.check(rc, "lvq_colsum")
        xc = x.cpu()
        want = xc.sum(0, dtype=torch.float64)
        chain = (math.ceil(rows / 1024) + 16 + 4 + 16) if rows >= 4096 else (math.ceil(rows / 16) + 16)
        bound = chain * U * xc.abs().sum(0, dtype=torch.float64) + 1e-30
        assert bool(((out.cpu().double() - want).abs() <= bound).all()), (rows, d)
        rc2, out2, _ = colsum(x, rows, d)
        assert rc2 == 0 and same_bits(out2, out)                                   # the header promises a fixed order
        if rows >= 4096:
            rc3, _, _ = colsum(x, rows, d, need - 1)
            assert rc3 == LVQ_EWORKSPACE


def test_reduce_step_on_device():
    from lidar_vision_vqa_amd import dist as D
    g = torch.Generator(device=DEV).manual_seed(5)
    for shape in ((32, 576, 768), (0, 3, 8)):                                      # the bench batch; a rank that owns no scene
        per_scene = torch.randn(shape, device=DEV, generator=g) + 0.25
        buf = torch.full((shape[-1] + 1,), float("nan"), device=DEV)
        D.reduce_step(per_scene, buf)
        xc = per_scene.cpu().reshape(-1, shape[-1])
        want = xc.sum(0, dtype=torch.float64)
        bound = (math.ceil(xc.shape[0] / 1024) + 36) * U * xc.abs().sum(0, dtype=torch.float64)
        got = buf.cpu()
        assert bool(((got[:-1].double() - want).abs() <= bound).all()), shape
        assert float(got[-1]) == float(shape[0])


# ------------------------------------------------------------------------------------------------
# 7. argmax
# ------------------------------------------------------------------------------------------------
def test_argmax_ties_and_edges():
    from lidar_vision_vqa_amd import ops
    n = 151936
    x = torch.randn(7, n, generator=gen(9))
    x[0, 100] = x[0, 140000] = 9.0                                                 # equal maxima in different 8192-wide chunks
    x[1, 0] = 9.0                                                                  # maximum at 0
    x[2, n - 1] = 9.0                                                              # maximum at n - 1
    x[3] = float("-inf")
    x[3, 77777] = -5.0                                                             # -inf everywhere but one entry
    x[4] = float("-inf")                                                           # -inf everywhere: the first index
    x[5, 8191] = x[5, 8192] = 9.0                                                  # a tie across a chunk boundary
    x[6] = -1.0
    x[6, 3] = x[6, 12000] = 0.0
    x[6, 5] = -0.0                                                                 # -0.0 ties +0.0
    got = ops.argmax_rows(x.to(DEV)).cpu()
    assert got.tolist() == x.argmax(-1).tolist() == [100, 0, n - 1, 77777, 0, 8191, 3]
    for row in ([-0.0, 0.0, -1.0], [0.0, -0.0], [-1.0, -0.0, 0.0]):
        t = torch.tensor([row])
        assert ops.argmax_rows(t.to(DEV)).cpu().tolist() == t.argmax(-1).tolist(), row


# ------------------------------------------------------------------------------------------------
# 8. decode step at the reference decoder's geometry
# ------------------------------------------------------------------------------------------------
GEO = dict(d=896, H=14, Hk=2, inter=4864, n_layers=2, lmax=1000, eps=1e-6, theta=1e6)   # Qwen2.5-0.5B widths, 2 of its layers
CANARY = 0x4640                                                                  # bf16 12288.0: a key read from it would swamp the softmax


@pytest.fixture(scope="module")
def decoder_weights():
    """Seeded fp32 weights per layer, their hi / lo parts on the device, and the fp64 weights each precision sees."""
    c = GEO
    d, dkv, inter = c["d"], c["d"] // c["H"] * c["Hk"], c["inter"]
    ld = d + 2 * dkv
    g = gen(2024)
    layers = []
    for _ in range(c["n_layers"]):
        w32 = dict(wqkv=torch.randn(ld, d, generator=g) / d ** 0.5, wo=torch.randn(d, d, generator=g) / d ** 0.5,
                   wgu=torch.randn(2 * inter, d, generator=g) / d ** 0.5, wdown=torch.randn(d, inter, generator=g) / inter ** 0.5)
        vec = dict(ln1=1.0 + 0.2 * torch.randn(d, generator=g), ln2=1.0 + 0.2 * torch.randn(d, generator=g), bqkv=0.2 * torch.randn(ld, generator=g))
        dev = {k: tuple(t.to(DEV) for t in bf16_pair(v)) for k, v in w32.items()}
        dev.update({k: v.to(DEV) for k, v in vec.items()})
        ref = {}
        for prec in (1, 3):
            r = {k: (h.double() + (l.double() if prec == 3 else 0.0)) for k, (h, l) in ((k, bf16_pair(v)) for k, v in w32.items())}
            r.update({k: v.double() for k, v in vec.items()})
            ref[prec] = r
        layers.append((dev, ref))
    return layers


def _cache_pair(B, pos, lmax, dkv, prec, g):
    """A cache [B, lmax, dkv] (+ one guard row) of canaries with random entries at positions < pos; returns the device buffers, their
    [B, lmax, dkv] views and the fp64 values of positions < pos."""
    hi = torch.full(((B * lmax + 1) * dkv,), CANARY, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    lo = hi.clone() if prec == 3 else None
    v32 = torch.randn(B, pos, dkv, generator=g) * 1.5
    h, l = bf16_pair(v32)
    hv = hi[:B * lmax * dkv].view(B, lmax, dkv)
    hv[:, :pos] = h.to(DEV)
    val = h.double()
    if prec == 3:
        lo[:B * lmax * dkv].view(B, lmax, dkv)[:, :pos] = l.to(DEV)
        val = val + l.double()
    return hi, lo, val


@pytest.mark.parametrize("prec", [1, 3])
@pytest.mark.parametrize("batch", [1, 2, 8, 9, 12])
def test_qwen2_decode_step_reference_geometry(decoder_weights, batch, prec):
    from lidar_vision_vqa_amd import head
    c = GEO
    d, H, Hk, inter, lmax = c["d"], c["H"], c["Hk"], c["inter"], c["lmax"]
    dh = d // H
    dkv = dh * Hk
    nbytes = int(L().lvq_qwen2_decode_workspace_bytes(F.cint(batch), F.cint(d), F.cint(H), F.cint(Hk), F.cint(inter), F.cint(lmax), F.cint(prec)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rel = 1e-4 if prec == 3 else 2e-2
    for pos in (0, 1, 63, 879, lmax - 1):
        g = gen(batch * 10000 + pos * 10 + prec)
        arr = (head._Qwen2LayerPtrs * c["n_layers"])()
        caches = []
        for i, (dw, _) in enumerate(decoder_weights):
            kh, kl, kval = _cache_pair(batch, pos, lmax, dkv, prec, g)
            vh, vl, vval = _cache_pair(batch, pos, lmax, dkv, prec, g)
            caches.append((kh, kl, kval, vh, vl, vval))
            p = lambda t: None if t is None else t.data_ptr()
            lo = (lambda k: p(dw[k][1])) if prec == 3 else (lambda k: None)
            arr[i] = head._Qwen2LayerPtrs(p(dw["ln1"]), p(dw["ln2"]), p(dw["wqkv"][0]), lo("wqkv"), p(dw["bqkv"]), p(dw["wo"][0]), lo("wo"),
                                          p(dw["wgu"][0]), lo("wgu"), p(dw["wdown"][0]), lo("wdown"), p(kh), p(kl), p(vh), p(vl))
        x = torch.randn(batch, d, generator=g)
        xd = x.to(DEV)
        rc = L().lvq_qwen2_decode_step(arr, F.cint(c["n_layers"]), F.ptr(xd), F.cint(batch), F.cint(d), F.cint(H), F.cint(Hk), F.cint(inter),
                                       F.cint(pos), F.cint(lmax), F.cfloat(c["eps"]), F.cfloat(c["theta"]), F.cint(prec), F.ptr(ws),
                                       F.csize(nbytes), st())
        F.check(rc, "lvq_qwen2_decode_step")
        xr = x.double()
        for i, (_, wr) in enumerate(decoder_weights):
            kh, kl, kval, vh, vl, vval = caches[i]
            xr, k_new, v_new = DO.decode_layer(xr, wr[prec], kval, vval, pos, H, Hk, c["eps"], c["theta"])
            for hi, lo, val, want in ((kh, kl, kval, k_new), (vh, vl, vval, v_new)):
                view = lambda t: t[:batch * lmax * dkv].view(batch, lmax, dkv).cpu()
                got = view(hi)[:, pos].double() + (view(lo)[:, pos].double() if prec == 3 else 0.0)
                assert float((got - want).abs().max()) <= rel * float(want.abs().max()), ("cache row", i, pos, batch, prec)
                for part in ((hi, lo) if prec == 3 else (hi,)):
                    v = view(part)
                    assert bool((v[:, pos + 1:].view(torch.int16) == CANARY).all()), ("cache rows above pos", i, pos)
                    assert bool((part[batch * lmax * dkv:].view(torch.int16) == CANARY).all()), ("guard row", i, pos)
                lo_below = view(lo)[:, :pos].double() if prec == 3 else 0.0
                assert torch.equal(view(hi)[:, :pos].double() + lo_below, val), ("cache rows below pos", i, pos)
        err = float((xd.cpu().double() - xr).abs().max())
        assert err <= rel * float(xr.abs().max()), (pos, batch, prec, err)


@pytest.mark.parametrize("split", [False, True])
def test_gemv_rmsnorm_equals_rmsnorm_then_gemm(split):
    """lvq_gemv_rmsnorm_bf16 == lvq_rmsnorm + lvq_gemm_bf16 bit for bit (include/lvq.h), at the decode step's two fused projections."""
    k, eps = 896, 1e-6
    g = gen(31 + split)
    gamma = (1.0 + 0.2 * torch.randn(k, generator=g)).to(DEV)
    for n in (1152, 9728):
        wh, wl = (t.to(DEV) for t in bf16_pair(torch.randn(n, k, generator=g) / k ** 0.5))
        wl = wl if split else None
        bias = (0.2 * torch.randn(n, generator=g)).to(DEV) if n == 1152 else None
        for m in range(1, 9):
            x = (torch.randn(m, k, generator=g) * 3.0).to(DEV)
            outs = []
            for fused in (True, False):
                c32 = torch.full((m, n), float("nan"), device=DEV)
                ch = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device=DEV)
                cl = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device=DEV) if split else None
                if fused:
                    rc = L().lvq_gemv_rmsnorm_bf16(F.ptr(x), F.ptr(gamma), F.cfloat(eps), F.ptr(wh), F.ptr(wl), F.ptr(bias), F.cint(m), F.cint(n),
                                                   F.cint(k), F.i64(k), F.i64(n), F.ptr(c32), F.ptr(ch), F.ptr(cl), st())
                else:
                    hh = torch.empty((m, k), dtype=torch.bfloat16, device=DEV)
                    hl = torch.empty((m, k), dtype=torch.bfloat16, device=DEV) if split else None
                    F.check(L().lvq_rmsnorm(F.ptr(x), F.ptr(gamma), F.cfloat(eps), F.i64(m), F.cint(k), F.ptr(None), F.ptr(hh), F.ptr(hl), st()),
                            "lvq_rmsnorm")
                    rc = L().lvq_gemm_bf16(F.ptr(hh), F.ptr(hl), F.ptr(wh), F.ptr(wl), F.ptr(bias), F.ptr(None), F.ptr(None), F.i64(0),
                                           F.cfloat(1.0), F.cint(0), F.i64(m), F.cint(n), F.cint(k), F.i64(k), F.i64(k), F.i64(n), F.cint(1),
                                           F.i64(0), F.i64(0), F.i64(0), F.ptr(c32), F.ptr(ch), F.ptr(cl), st())
                F.check(rc, "projection")
                outs.append((c32, ch, cl))
            (a32, ah, al), (b32, bh, bl) = outs
            assert same_bits(a32, b32) and same_bits(ah, bh), (n, m)
            assert not bool(torch.isnan(a32).any())
            if split:
                assert same_bits(al, bl), (n, m)
