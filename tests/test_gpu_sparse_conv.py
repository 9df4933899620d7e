"""lvq_sparse_conv (csrc/sparse_conv.hip: gather-form implicit GEMM on bf16 MFMA tiles + fused epilogue) through the C ABI against the
fp64 restatement of tests/sparse_conv_cases.py.  The neighbour tables come from the CPU restatement, so the kernel is the only subject.

Bounds are the ones tests/test_gpu_kernel_routes.py holds the GEMMs to, in the same regime (N(0, 1) features, weights scaled by
1 / sqrt(K C_in)):  hi + lo operands 2e-4 max(1, max|ref|);  plain bf16 with operands rounded to bf16 on the host first (the reference
sees the rounded values, so what is left is the fp32 accumulation) 2e-5 max(1, max|ref|)."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sparse_conv_cases as SC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import backbone3d as B3  # noqa: E402
from lidar_vision_vqa_amd import synth  # noqa: E402

DEV = "cuda:0"
FILL = -7.25
NS = (1, 63, 64, 65, 1000)
BOUND = {"bf16x3": 2e-4, "bf16": 2e-5}
EPILOGUES = list(itertools.product((False, True), repeat=4))                   # (bias, bn, relu, residual)


@functools.lru_cache(maxsize=None)
def table(n):
    """n distinct cells of a [8, 9, 10] grid (batch 2) in a shuffled order and their submanifold 3 x 3 x 3 table."""
    rng = np.random.default_rng(100 + n)
    cells = rng.permutation(2 * 8 * 9 * 10)[:n]
    idx = np.stack([cells // 720, cells // 90 % 8, cells // 10 % 9, cells % 10], axis=1).astype(np.int32)
    return idx, SC.rules(idx, [8, 9, 10], 2, (3, 3, 3), 1, 1, True)[1]


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def run_conv(feat, nbr, w, mode, bias=None, scale=None, shift=None, residual=None, relu=False, extra=70):
    """out [n + extra, C_out] (pre-filled), the conv over the first n rows with the count read from the device."""
    L = B3._lib()
    dev = torch.device(DEV)
    n, kvol = nbr.shape
    cout, cin = w.shape[0], w.shape[-1]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    d_feat, d_w = t(feat), t(w.reshape(cout, kvol, cin))
    ne = int(L.lvq_sparse_conv_packed_elems(F.cint(cout), F.cint(kvol), F.cint(cin)))
    assert ne == kvol * cout * max(32, cin)
    hi = torch.empty((ne,), dtype=torch.int16, device=dev)
    lo = torch.empty((ne,), dtype=torch.int16, device=dev) if mode == "bf16x3" else None
    rc = L.lvq_sparse_conv_pack_weights(F.ptr(d_w), F.cint(cout), F.cint(kvol), F.cint(cin), F.ptr(hi), F.ptr(lo), F.stream_ptr(dev))
    assert rc == 0
    cap = n + extra
    d_nbr = torch.zeros((cap, kvol), dtype=torch.int32, device=dev)             # rows behind the count point at row 0: they must not run
    d_nbr[:n] = torch.from_numpy(nbr.astype(np.int32)).to(dev)
    d_res = None
    if residual is not None:
        d_res = torch.zeros((cap, cout), dtype=torch.float32, device=dev)
        d_res[:n] = t(residual)
    out = torch.full((cap, cout), FILL, dtype=torch.float32, device=dev)
    n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    d_bias, d_scale, d_shift = t(bias), t(scale), t(shift)                      # (kept alive until the kernel has run)
    rc = L.lvq_sparse_conv(F.ptr(d_feat), F.i64(feat.shape[0]), F.cint(cin), F.ptr(d_nbr), F.cint(kvol), F.i64(cap), F.ptr(n_dev), F.ptr(hi),
                           F.ptr(lo), F.cint(cout), F.ptr(d_bias), F.ptr(d_scale), F.ptr(d_shift), F.ptr(d_res), F.cint(int(relu)),
                           F.ptr(out), F.stream_ptr(dev))
    assert rc == 0, F.lib().lvq_strerror(rc)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def operands(n, cin, cout, mode, seed, kvol=27):
    feat = synth.randn((n, cin), seed)
    w = synth.randn((cout, 3, 3, 3, cin), seed + 1, 1.0 / np.sqrt(kvol * cin))
    if mode == "bf16":
        feat, w = bf16_round(feat), bf16_round(w)
    ep = dict(bias=synth.randn((cout,), seed + 2, 0.5), scale=(0.5 + np.random.default_rng(seed + 3).random(cout)).astype(np.float32),
              shift=synth.randn((cout,), seed + 4, 0.5), residual=synth.randn((n, cout), seed + 5))
    return feat, w, ep


def compare(n, cin, cout, mode, flags, seed):
    use_bias, use_bn, relu, use_res = flags
    _, nbr = table(n)
    feat, w, ep = operands(n, cin, cout, mode, seed)
    kw = dict(bias=ep["bias"] if use_bias else None, scale=ep["scale"] if use_bn else None, shift=ep["shift"] if use_bn else None,
              residual=ep["residual"] if use_res else None, relu=relu)
    ref = SC.epilogue(SC.conv_from_table(feat, nbr, w), **kw)
    out = run_conv(feat, nbr, w, mode, **kw)
    assert (out[n:] == FILL).all(), "rows behind n_out were written"
    err = float(np.abs(out[:n] - ref).max())
    bound = BOUND[mode] * max(1.0, float(np.abs(ref).max()))
    print(f"n={n} {cin}->{cout} {mode} flags={flags}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (n, cin, cout, mode, flags, err, bound)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("cout", SC.COUT)
@pytest.mark.parametrize("cin", SC.CIN)
def test_conv_every_channel_pair_and_row_count(cin, cout, mode):
    """Every supported (C_in, C_out), both operand forms, N in {1, 63, 64, 65, 1000}; the epilogue variant rotates with the case so
    that all sixteen occur for every form (test_conv_epilogue_variants crosses them fully on two pairs)."""
    base = (SC.CIN.index(cin) * 4 + SC.COUT.index(cout)) * len(NS)
    for j, n in enumerate(NS):
        compare(n, cin, cout, mode, EPILOGUES[(base + j) % 16], 1000 + base + j)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("cin,cout", [(5, 16), (128, 128)])
def test_conv_epilogue_variants(cin, cout, mode):
    for i, flags in enumerate(EPILOGUES):
        compare(65, cin, cout, mode, flags, 2000 + i)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("cin,cout", [(4, 16), (64, 64), (128, 32)])
def test_conv_row_permutation_and_rerun_are_bit_exact(cin, cout, mode):
    """A row's bits depend on its own neighbours only: permuting the input rows of a submanifold conv permutes the outputs bit for bit
    (rows change tiles, tiles change which offsets they skip), and two runs give the same bits."""
    n = 1000
    _, nbr = table(n)
    feat, w, ep = operands(n, cin, cout, mode, 3000 + cin)
    kw = dict(bias=ep["bias"], scale=ep["scale"], shift=ep["shift"], residual=None, relu=True)
    a = run_conv(feat, nbr, w, mode, **kw)[:n]
    b = run_conv(feat, nbr, w, mode, **kw)[:n]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    perm = np.random.default_rng(9).permutation(n)                              # new row j = old row perm[j]
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    nbr2 = nbr[perm]
    nbr2 = np.where(nbr2 >= 0, inv[np.maximum(nbr2, 0)], -1)
    c = run_conv(feat[perm], nbr2, w, mode, **kw)[:n]
    assert np.array_equal(c.view(np.uint32), a[perm].view(np.uint32))
    assert float(np.abs(a).max()) > 0.5


def test_conv_2d_kernel_and_foreign_table_entries():
    """K = 9 (SparseConv2d / SubMConv2d), and a table entry outside [0, n_in) reads as absent instead of being dereferenced."""
    idx, shape, batch = SC.coords("g2a")
    _, nbr = SC.rules(idx, shape, batch, (3, 3), 1, 1, True)
    n = len(idx)
    feat = synth.randn((n, 128), 41)
    w = synth.randn((128, 3, 3, 128), 42, 1.0 / np.sqrt(9 * 128))
    ref = SC.conv_from_table(feat, nbr, w)
    bad = nbr.copy()
    holes = np.argwhere(bad < 0)[:40]
    bad[holes[::2, 0], holes[::2, 1]] = n + 5
    bad[holes[1::2, 0], holes[1::2, 1]] = -123456
    out = run_conv(feat, bad, w, "bf16x3")[:n]
    assert float(np.abs(out - ref).max()) <= 2e-4 * max(1.0, float(np.abs(ref).max()))


def test_conv_refuses_channel_counts_outside_the_family():
    L = B3._lib()
    dev = torch.device(DEV)
    z = torch.zeros((64, 64), dtype=torch.float32, device=dev)
    zi = torch.zeros((64, 27), dtype=torch.int32, device=dev)
    zw = torch.zeros((27 * 128 * 128,), dtype=torch.int16, device=dev)
    out = torch.full((64, 128), FILL, dtype=torch.float32, device=dev)
    for cin, cout in ((8, 16), (64, 48), (256, 128), (3, 16)):
        assert L.lvq_sparse_conv_packed_elems(F.cint(cout), F.cint(27), F.cint(cin)) == 0
        assert L.lvq_sparse_conv_pack_weights(F.ptr(z), F.cint(cout), F.cint(27), F.cint(cin), F.ptr(zw), F.ptr(None), F.stream_ptr(dev)) == -5
        rc = L.lvq_sparse_conv(F.ptr(z), F.i64(8), F.cint(cin), F.ptr(zi), F.cint(27), F.i64(8), F.ptr(None), F.ptr(zw), F.ptr(None), F.cint(cout),
                               F.ptr(None), F.ptr(None), F.ptr(None), F.ptr(None), F.cint(0), F.ptr(out), F.stream_ptr(dev))
        assert rc == -5                                                          # LVQ_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    m = B3.SubMConv3d(8, 16, 3, indice_key="k").to(dev).eval()
    x = B3.SparseConvTensor(torch.zeros((2, 8), device=dev), torch.tensor([[0, 1, 1, 1], [0, 1, 1, 2]], dtype=torch.int32, device=dev), [4, 4, 4], 1)
    with pytest.raises(F.LvqError), torch.no_grad():
        m(x)
