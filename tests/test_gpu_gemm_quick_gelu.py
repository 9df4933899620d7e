"""LVQ_GEMM_QUICK_GELU, the second activation flag of lvq_gemm_bf16: x <- x / (1 + exp(-1.702 x)) after the bias, in fp32.

One shape per kernel geometry and route through which the flag dispatches (csrc/gemm.hip: lvq_gemm_bf16; shapes as derived in
tests/test_gpu_kernel_routes.py for 256 CUs), plus the CLIP-L fc1 shape (2 x 257 rows, 4096 x 1024) in both operand forms.

Reference: fp64 QuickGELU applied to the fp32 result y0 of the SAME call with flags = 0 (same route, same accumulators), which
isolates the epilogue.  First-order fp32 bound, u = 2^-24, a = 1.702, t = -a y0, e = exp(t), g = y0 / (1 + e):
    t       the constant 1.702f and the product round once each                      |dt| <= 2 u |t|
    e       one exponential, 1 ulp = 2 u, plus the argument's error                  de / e <= 2 u + 2 u |t|
    1 + e   one add                                                                  ds / s <= u + (e / (1 + e)) de / e
    g       one divide (IEEE)                                                        dg / |g| <= 2 u + (e / (1 + e)) (2 u + 2 u |t|)
plus 1e-37 absolute where exp overflows and the quotient is -0 or subnormal.  The kernel is held to TWICE that bound; alpha, residual and
row table add one rounding each where a case uses them.  Every figure is printed before it is asserted."""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from lidar_vision_vqa_amd import synth  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
A = 1.702
SPECIALS = (0.0, -0.0, 1e-3, -1e-3, 1.0, -1.0, 20.0, -20.0, 100.0, -100.0)
GELU, QUICK = 1, 2


def F():
    from lidar_vision_vqa_amd import _ffi
    return _ffi


def addr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(synth.randn(tuple(shape), seed, scale))


@functools.lru_cache(maxsize=4)
def operands(m, n, k):
    """bf16 (hi, lo) operands on the device.  W rows 0..9 are zero and bias[0..9] holds SPECIALS: columns 0..9 of every output row are
    pre-activations of exactly those values.  The other pre-activations are ~ N(0, 2): the curved range and both tails."""
    a, w = rnd((m, k), 11).to(DEV), rnd((n, k), 12, math.sqrt(2.0 / k)).to(DEV)
    bias = rnd((n,), 13).to(DEV)
    w[:len(SPECIALS)] = 0.0
    bias[:len(SPECIALS)] = torch.tensor(SPECIALS)
    ah, wh = a.to(torch.bfloat16), w.to(torch.bfloat16)
    return ah, (a - ah.float()).to(torch.bfloat16), wh, (w - wh.float()).to(torch.bfloat16), bias


def gemm(m, n, k, mode, flags, outs=("f32",), alpha=1.0, res=None, tab=None, sentinel=None):
    """One contiguous lvq_gemm_bf16 call -> (rc, c_f32 | None, c_bf16 | None, c_lo | None)."""
    ah, al, wh, wl, bias = operands(m, n, k)
    if mode != "x3":
        al = None
    if mode == "plain":
        wl = None
    mk = lambda dt: torch.full((m, n), float("nan") if sentinel is None else sentinel, dtype=dt, device=DEV)
    c32 = mk(torch.float32) if "f32" in outs else None
    c16 = mk(torch.bfloat16) if "bf16" in outs else None
    clo = mk(torch.bfloat16) if "lo" in outs else None
    f = F()
    rc = f.lib().lvq_gemm_bf16(addr(ah), addr(al), addr(wh), addr(wl), addr(bias), addr(res), addr(tab),
                               f.i64(tab.shape[0] if tab is not None else 0), f.cfloat(alpha), f.cint(flags), f.i64(m), f.cint(n), f.cint(k),
                               f.i64(k), f.i64(k), f.i64(n), f.cint(1), f.i64(0), f.i64(0), f.i64(0), addr(c32), addr(c16), addr(clo),
                               f.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, c32, c16, clo


def quick64(y0):
    y = y0.double()
    return y / (1.0 + torch.exp(-A * y))


def bound(y0):
    y = y0.double()
    t = (A * y).abs()
    e = torch.exp(-A * y)
    frac = torch.where(torch.isinf(e), torch.ones_like(e), e / (1.0 + e))
    return quick64(y0).abs() * (2 * U + frac * (2 * U + 2 * U * t)) + 1e-37


WORST = {}


def check_quick(label, m, n, k, mode, outs_extra=True):
    """flags = 0 -> y0; flags = QUICK against fp64 QuickGELU(y0); specials; the bf16 (+ lo) outputs are the same fp32 value, rounded."""
    rc, y0, _, _ = gemm(m, n, k, mode, 0)
    assert rc == 0, (label, rc)
    rc, got, _, _ = gemm(m, n, k, mode, QUICK)
    assert rc == 0, (label, rc)
    assert bool(torch.isfinite(got).all()), f"{label}: a non-finite QuickGELU output"
    ref, b = quick64(y0), bound(y0)
    ratio = float(((got.double() - ref).abs() / b).max())
    WORST[f"{label} {mode}"] = ratio
    print(f"{label} ({m}, {n}, {k}) {mode}: max err / bound {ratio:.3f} (held to 2), max|y0| {float(y0.abs().max()):.2f}")
    assert ratio <= 2.0, (label, ratio)
    # the special pre-activations, exactly
    sp = torch.tensor(SPECIALS, device=DEV)
    assert torch.equal(y0[:, :len(SPECIALS)], sp.expand(m, -1)), f"{label}: columns 0..9 of the flag-0 result are not the special values"
    g = got[:, :len(SPECIALS)]
    for j, x in enumerate(SPECIALS):
        col = g[:, j]
        if x == 0.0:
            assert bool((col == 0).all()), (label, x)
        elif x > 0:
            assert bool((col > 0).all()), (label, x)
        else:
            assert bool((col <= 0).all()) and bool(torch.signbit(col).all()), (label, x, col[:4].tolist())
    assert float(g[0, 8]) == 100.0 and float(g[0, 9]) == 0.0 and float(g[0, 7]) < 0.0 and float(g[0, 7]) > -1e-12
    if outs_extra:
        rc, _, hi, lo = gemm(m, n, k, mode, QUICK, outs=("bf16", "lo"))
        assert rc == 0, (label, rc)
        assert torch.equal(hi, got.to(torch.bfloat16)), f"{label}: c_bf16 != bf16(c_f32)"
        assert torch.equal(lo, (got - hi.float()).to(torch.bfloat16)), f"{label}: c_lo != bf16(c_f32 - hi)"
    return y0, got


# (label, m, n, k): the instantiation each reaches is derived in tests/test_gpu_kernel_routes.py
TILE_ROUTES = [
    ("64/reg", 200, 136, 72),              # k_gemm_bf16<64, 64, 0, 2, 4>: ragged K, register staging
    ("64/dma", 200, 136, 128),             # <64, 64, 1, 2, 4>
    ("128/reg", 2000, 1600, 72),           # <128, 128, 0, 2, 4>: 16 x 13 = 208 >= 192 tiles
    ("128/dma", 2000, 1600, 128),          # <128, 128, 1, 2, 4>
    ("256x128", 16300, 1032, 128),         # <256, 128, 1, 2, 8>: 64 x 9 = 576 >= 512 tiles
    ("256x128/scalar", 16300, 1028, 128),  # n % 8 == 4: the scalar epilogue of the same kernel
]


@pytest.mark.parametrize("mode", ["plain", "x3"])
@pytest.mark.parametrize("label,m,n,k", TILE_ROUTES)
def test_quick_gelu_tile_routes(label, m, n, k, mode):
    check_quick(label, m, n, k, mode)


def test_quick_gelu_x2w_form():
    """a plain, w hi + lo (two segments) on the 64-tile ring."""
    check_quick("64/dma x2w", 200, 136, 128, "x2w")


@pytest.mark.parametrize("mode", ["plain", "x3"])
@pytest.mark.parametrize("m,n", [(512, 512), (256, 2304)])
def test_quick_gelu_256x256_tile(m, n, mode, tune):
    """k_gemm_256<2, 1> (n / 256 <= 8 column tiles: non-temporal A) and k_gemm_256<2, 0> (9 column tiles), with the tile-count
    threshold lowered through the tuning record as in tests/test_gpu_kernel_routes.py."""
    tune(gemm_256x256_min_tiles=1)
    check_quick(f"256x256 ntx={n // 256}", m, n, 64, mode)


@pytest.mark.parametrize("mode", ["plain", "x3"])
@pytest.mark.parametrize("m", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [200, 4100])
def test_quick_gelu_gemv_route(m, n, mode):
    """m <= 8: k_gemv<MM, X3, R, 0, true> for MM in {1, 2, 4, 8} (m = 3 -> 4, 5 -> 8) and R = 1 (n < 4096) / 4."""
    check_quick(f"gemv m={m} n={n}", m, n, 264, mode)


@pytest.mark.parametrize("mode", ["plain", "x3"])
def test_quick_gelu_clip_fc1_shape(mode):
    """(257 * 2, 4096, 1024): fc1 of the CLIP-L tower on two images; c_f32, and c_bf16 (+ lo) as the tower asks for it."""
    check_quick("clip fc1", 257 * 2, 4096, 1024, mode)


def test_quick_gelu_then_alpha_residual_table():
    """The rest of the epilogue runs after the activation as it does for the other flag: alpha, residual, row table."""
    m, n, k, alpha = 200, 136, 128, 0.75
    res, tab = rnd((m, n), 21).to(DEV), rnd((37, n), 22).to(DEV)
    for mode in ("plain", "x3"):
        _, y0, _, _ = gemm(m, n, k, mode, 0)
        rc, got, _, _ = gemm(m, n, k, mode, QUICK, alpha=alpha, res=res, tab=tab)
        assert rc == 0
        g = quick64(y0) * alpha
        r1 = g + res.double()
        ref = r1 + tab.double()[torch.arange(m, device=DEV) % 37]
        b = 2 * (bound(y0) * alpha) + U * (g.abs() + r1.abs() + ref.abs())
        ratio = float(((got.double() - ref).abs() / b).max())
        print(f"alpha + residual + table {mode}: max err / bound {ratio:.3f}")
        assert ratio <= 1.0, ratio


def test_both_flags_are_refused_before_any_launch():
    for outs in (("f32",), ("f32", "bf16", "lo")):
        rc, c32, c16, clo = gemm(200, 136, 128, "x3", GELU | QUICK, outs=outs, sentinel=-7.0)
        assert rc == -1, rc
        for c in (c32, c16, clo):
            assert c is None or bool((c == -7.0).all()), "a refused call wrote to an output"
    rc, c32, _, _ = gemm(2, 200, 264, "plain", GELU | QUICK, sentinel=-7.0)       # the skinny-M route
    assert rc == -1 and bool((c32 == -7.0).all())


@pytest.mark.parametrize("m,n,k", [(200, 136, 128), (3, 200, 264)])
def test_other_flags_are_unchanged_around_a_quick_gelu_call(m, n, k):
    before = [gemm(m, n, k, "x3", fl)[1] for fl in (0, GELU)]
    rc, q, _, _ = gemm(m, n, k, "x3", QUICK)
    assert rc == 0
    after = [gemm(m, n, k, "x3", fl)[1] for fl in (0, GELU)]
    for b, a in zip(before, after):
        assert torch.equal(b.view(torch.int32), a.view(torch.int32))
    assert not torch.equal(before[0], before[1]) and not torch.equal(q, before[1]) and not torch.equal(q, before[0])
    ref = 0.5 * before[0].double() * (1.0 + torch.erf(before[0].double() / math.sqrt(2.0)))
    assert float((before[1].double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))


def test_print_worst_ratio():
    """The largest err / bound over the cases above (DESIGN 3.9 quotes it); runs last in file order."""
    if WORST:
        k = max(WORST, key=WORST.get)
        print(f"largest QuickGELU err / bound: {WORST[k]:.3f} at {k}")
        assert WORST[k] <= 2.0
