"""The SECOND / CenterPoint and PillarNet backbones on the MI355X: lvq_sparse_conv_rules at the per-axis geometries of VoxelBackBone8x /
VoxelResBackBone8x, the 256-channel layers of lvq_sparse_conv, lvq_conv2d_res, and the four backbones (backbone3d.py, backbone_pillar.py)
with their chains into HeightCompression + BaseBEVBackbone and BaseBEVBackboneV1, against the fp64 restatements of
tests/second_pillarnet_cases.py.

Bounds: the kernel tests keep those of tests/test_gpu_sparse_conv.py and tests/test_gpu_conv2d.py (hi + lo operands 2e-4 max(1, max|ref|);
plain bf16 with host-rounded operands 2e-5 max(1, max|ref|): they were set for sums 27 x 128 deep, and 9 x 256 / 27 x 256 terms at the
same weight scale 1 / sqrt(taps C_in) are of the same order).  Whole backbones in bf16x3 are held to the project's parity bar,
1e-3 max(1, max|ref|), at every stage.  The plain bf16 form over a whole backbone has no bar known in advance: its error is printed and
recorded in DESIGN 3.6 (measured on the MI355X, last stage / worst stage, of max(1, max|ref|): VoxelBackBone8x 4.2e-3 / 4.2e-3,
VoxelResBackBone8x 4.8e-3 / 5.8e-3, PillarBackBone8x 4.3e-3 / 7.1e-3, PillarRes18BackBone8x 6.7e-3 / 8.2e-3), and only its finiteness is
asserted."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bev_backbone_cases as BC  # noqa: E402
import second_pillarnet_cases as C  # noqa: E402
import sparse_conv_cases as SC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import backbone2d as B2  # noqa: E402
from lidar_vision_vqa_amd import backbone3d as B3  # noqa: E402
from lidar_vision_vqa_amd import lidar, synth  # noqa: E402

DEV = "cuda:0"
BAR = 1e-3
FILL, FILL_I, FILL16 = -7.25, 0x5A5A5A5A, 0x7B7B
NS = (1, 63, 64, 65, 1000)
BOUND = {"bf16x3": 2e-4, "bf16": 2e-5}
MODES = ("bf16x3", "bf16")
EPILOGUES = list(itertools.product((False, True), repeat=4))                   # (bias, bn, relu, residual)
WIDE = ((128, 256), (256, 256))


def dev(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def bits_to_f32(t):
    return t.view(torch.bfloat16).float()


# --------------------------------------------------------------------------------------------------------------------------------
# 1. rules at the per-axis geometries
# --------------------------------------------------------------------------------------------------------------------------------
GEOMS = {"conv4": ((3, 3, 3), (2, 2, 2), (0, 1, 1)), "conv_out": ((3, 1, 1), (2, 1, 1), (0, 0, 0)), "conv_out_last_pad": ((3, 1, 1), (2, 1, 1), (1, 1, 1))}


@pytest.mark.parametrize("case", ["edge3", "g3a", "n0", "n1"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_rules_per_axis_kernel_stride_padding(case, geom):
    """Output rows (ascending (b, z, y, x)), their count and the whole neighbour table equal the dictionary restatement; the buffers
    are larger than the result and pre-filled, and everything behind the live rows keeps the pattern."""
    k, s, p = GEOMS[geom]
    idx, shape, batch = SC.coords(case)
    want_idx, want_nbr = SC.rules(idx, shape, batch, k, s, p, False)
    L, d = B3._lib(), torch.device(DEV)
    n, kvol = len(idx), int(np.prod(k))
    kc = int(np.prod([-(-kk // ss) for kk, ss in zip(k, s)]))
    cap = min(max(n * kc, 1), batch * int(np.prod(SC.out_shape(shape, k, s, p, False)))) + 37
    out_idx = torch.full((cap, 4), FILL_I, dtype=torch.int32, device=d)
    nbr = torch.full((cap, kvol), FILL_I, dtype=torch.int32, device=d)
    n_out = torch.full((1,), FILL_I, dtype=torch.int32, device=d)
    args = (3, F.i32x(shape), batch, F.i32x(k), F.i32x(s), F.i32x(p), 0)
    nbytes = int(L.lvq_sparse_conv_rules_workspace_bytes(n, *args))
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=d)
    d_idx = dev(idx, np.int32)
    rc = L.lvq_sparse_conv_rules(F.ptr(d_idx), n, *args, cap, F.ptr(out_idx), F.ptr(nbr), F.ptr(n_out), F.ptr(ws), nbytes, F.stream_ptr(d))
    torch.cuda.synchronize()
    assert rc == 0, F.lib().lvq_strerror(rc)
    m = int(n_out.item())
    got_idx, got_nbr = out_idx.cpu().numpy(), nbr.cpu().numpy()
    assert m == len(want_idx) and (m > 0) == (n > 0)
    assert np.array_equal(got_idx[:m], want_idx) and np.array_equal(got_nbr[:m], want_nbr)
    assert (got_idx[m:].view(np.uint32) == FILL_I).all() and (got_nbr[m:].view(np.uint32) == FILL_I).all(), "rows behind the count were written"
    if n:                                                                       # and through the module's wrapper (its own capacity guess)
        oi, nb, _, oshape = B3.sparse_conv_rules(dev(idx, np.int32), shape, batch, k, s, p, False)
        assert oshape == SC.out_shape(shape, k, s, p, False)
        assert np.array_equal(oi.cpu().numpy(), want_idx) and np.array_equal(nb.cpu().numpy(), want_nbr)


# --------------------------------------------------------------------------------------------------------------------------------
# 2. the 256-channel sparse layers
# --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(n, kvol):
    """n distinct cells in a shuffled order and their submanifold table: [8, 9, 10] x batch 2 for 27 offsets, [30, 40] x batch 2 for 9."""
    rng = np.random.default_rng(200 + n + kvol)
    if kvol == 27:
        cells = rng.permutation(2 * 8 * 9 * 10)[:n]
        idx, shape = np.stack([cells // 720, cells // 90 % 8, cells // 10 % 9, cells % 10], axis=1), [8, 9, 10]
    else:
        cells = rng.permutation(2 * 30 * 40)[:n]
        idx, shape = np.stack([cells // 1200, cells // 40 % 30, cells % 40], axis=1), [30, 40]
    return SC.rules(idx.astype(np.int32), shape, 2, (3,) * len(shape), 1, 1, True)[1]


def run_sparse(feat, nbr, w, mode, bias=None, scale=None, shift=None, residual=None, relu=False, extra=70):
    """out [n + extra, C_out] (pre-filled with the canary); the table rows behind n point at row 0 and must not run."""
    L, d = B3._lib(), torch.device(DEV)
    n, kvol = nbr.shape
    cout, cin = w.shape[0], w.shape[-1]
    d_feat, d_w = dev(feat), dev(w.reshape(cout, kvol, cin))
    ne = int(L.lvq_sparse_conv_packed_elems(cout, kvol, cin))
    assert ne == kvol * cout * cin, "(128, 256) / (256, 256) are outside the kernel family"
    hi = torch.empty((ne,), dtype=torch.int16, device=d)
    lo = torch.empty((ne,), dtype=torch.int16, device=d) if mode == "bf16x3" else None
    assert L.lvq_sparse_conv_pack_weights(F.ptr(d_w), cout, kvol, cin, F.ptr(hi), F.ptr(lo), F.stream_ptr(d)) == 0
    cap = n + extra
    d_nbr = torch.zeros((cap, kvol), dtype=torch.int32, device=d)
    d_nbr[:n] = dev(nbr, np.int32)
    d_res = None
    if residual is not None:
        d_res = torch.zeros((cap, cout), dtype=torch.float32, device=d)
        d_res[:n] = dev(residual)
    out = torch.full((cap, cout), FILL, dtype=torch.float32, device=d)
    n_dev = torch.tensor([n], dtype=torch.int32, device=d)
    d_bias, d_scale, d_shift = dev(bias), dev(scale), dev(shift)
    rc = L.lvq_sparse_conv(F.ptr(d_feat), feat.shape[0], cin, F.ptr(d_nbr), kvol, cap, F.ptr(n_dev), F.ptr(hi), F.ptr(lo), cout, F.ptr(d_bias),
                           F.ptr(d_scale), F.ptr(d_shift), F.ptr(d_res), int(relu), F.ptr(out), F.stream_ptr(d))
    assert rc == 0, F.lib().lvq_strerror(rc)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def operands(n, cin, cout, kvol, mode, seed):
    feat = synth.randn((n, cin), seed)
    w = synth.randn((cout, *((3, 3, 3) if kvol == 27 else (3, 3)), cin), seed + 1, 1.0 / np.sqrt(kvol * cin))
    if mode == "bf16":
        feat, w = bf16_round(feat), bf16_round(w)
    ep = dict(bias=synth.randn((cout,), seed + 2, 0.5), scale=(0.5 + np.random.default_rng(seed + 3).random(cout)).astype(np.float32),
              shift=synth.randn((cout,), seed + 4, 0.5), residual=synth.randn((n, cout), seed + 5))
    return feat, w, ep


def compare_sparse(n, cin, cout, kvol, mode, flags, seed):
    use_bias, use_bn, relu, use_res = flags
    nbr = table(n, kvol)
    feat, w, ep = operands(n, cin, cout, kvol, mode, seed)
    kw = dict(bias=ep["bias"] if use_bias else None, scale=ep["scale"] if use_bn else None, shift=ep["shift"] if use_bn else None,
              residual=ep["residual"] if use_res else None, relu=relu)
    ref = SC.epilogue(SC.conv_from_table(feat, nbr, w), **kw)
    out = run_sparse(feat, nbr, w, mode, **kw)
    assert (out[n:] == FILL).all(), "rows behind n_out were written"
    err = float(np.abs(out[:n] - ref).max())
    bound = BOUND[mode] * max(1.0, float(np.abs(ref).max()))
    print(f"n={n} {cin}->{cout} K={kvol} {mode} flags={flags}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (n, cin, cout, kvol, mode, flags, err, bound)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kvol", [9, 27])
@pytest.mark.parametrize("cin,cout", WIDE)
def test_wide_conv_every_pair_form_kernel_and_row_count(cin, cout, kvol, mode):
    """(128, 256) and (256, 256), both operand forms, 9 and 27 offsets, N in {1, 63, 64, 65, 1000}; the epilogue variant rotates with the
    case (test_wide_conv_epilogue_variants crosses all sixteen)."""
    base = ((WIDE.index((cin, cout)) * 2 + (kvol == 27)) * 2 + MODES.index(mode)) * len(NS)
    for j, n in enumerate(NS):
        compare_sparse(n, cin, cout, kvol, mode, EPILOGUES[(base + 3 * j) % 16], 5000 + base + j)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout", WIDE)
def test_wide_conv_epilogue_variants(cin, cout, mode):
    for i, flags in enumerate(EPILOGUES):
        compare_sparse(65, cin, cout, 9 if i % 2 else 27, mode, flags, 6000 + i)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout", WIDE)
def test_wide_conv_row_permutation_and_rerun_are_bit_exact(cin, cout, mode):
    """A row's bits depend on its own neighbours only (rows change tiles, tiles change which offsets and 16-row tiles they skip), and
    two runs give the same bits."""
    n = 1000
    nbr = table(n, 27)
    feat, w, ep = operands(n, cin, cout, 27, mode, 7000 + cin)
    kw = dict(bias=ep["bias"], scale=ep["scale"], shift=ep["shift"], residual=None, relu=True)
    a = run_sparse(feat, nbr, w, mode, **kw)[:n]
    b = run_sparse(feat, nbr, w, mode, **kw)[:n]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    perm = np.random.default_rng(9).permutation(n)                              # new row j = old row perm[j]
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    nbr2 = nbr[perm]
    nbr2 = np.where(nbr2 >= 0, inv[np.maximum(nbr2, 0)], -1)
    c = run_sparse(feat[perm], nbr2, w, mode, **kw)[:n]
    assert np.array_equal(c.view(np.uint32), a[perm].view(np.uint32))
    assert float(np.abs(a).max()) > 0.5


@pytest.mark.parametrize("cin,cout", WIDE)
def test_wide_conv_foreign_table_entries_read_as_absent(cin, cout):
    n = 200
    nbr = table(n, 9)
    feat, w, _ = operands(n, cin, cout, 9, "bf16x3", 8000)
    ref = SC.conv_from_table(feat, nbr, w)
    bad = nbr.copy()
    holes = np.argwhere(bad < 0)[:40]
    assert len(holes) == 40
    bad[holes[::2, 0], holes[::2, 1]] = n + 5
    bad[holes[1::2, 0], holes[1::2, 1]] = -123456
    out = run_sparse(feat, bad, w, "bf16x3")[:n]
    assert float(np.abs(out - ref).max()) <= BOUND["bf16x3"] * max(1.0, float(np.abs(ref).max()))


def test_wide_family_is_exactly_two_pairs():
    L = B3._lib()
    assert L.lvq_sparse_conv_packed_elems(256, 27, 128) == 27 * 256 * 128 and L.lvq_sparse_conv_packed_elems(256, 9, 256) == 9 * 256 * 256
    for cin, cout in ((256, 128), (256, 64), (64, 256), (32, 256), (512, 256), (256, 512)):
        assert L.lvq_sparse_conv_packed_elems(cout, 27, cin) == 0, (cin, cout)


# --------------------------------------------------------------------------------------------------------------------------------
# 3. lvq_conv2d_res
# --------------------------------------------------------------------------------------------------------------------------------
def run_res(x, wt, mode, scale, shift, res, relu=True, use_res=True, res_lo=True, kernel=3, c_out=None, w_lo=True, res_hi=True):
    """(rc, fp32 [B, C, H, W], hi, lo planes) of lvq_conv2d_res (or lvq_conv2d with use_res = False), kernel 3, stride 1; both output
    forms, pre-filled.  `res` is Planes."""
    L, d = B2._lib(), torch.device(DEV)
    split = mode == "bf16x3"
    b, cin, h, w = x.shape
    cout = wt.shape[0]
    xp = B2.to_planes(dev(x), split)
    ne = int(L.lvq_conv2d_packed_elems(cout, cin, 3, 0))
    w_hi = torch.empty((ne,), dtype=torch.int16, device=d)
    w_l = torch.empty((ne,), dtype=torch.int16, device=d) if split else None
    assert L.lvq_conv2d_pack_weights(F.ptr(dev(wt)), cout, cin, 3, 0, F.ptr(w_hi), F.ptr(w_l), F.stream_ptr(d)) == 0
    f32 = torch.full((b, cout, h, w), FILL, dtype=torch.float32, device=d)
    p_hi = torch.full((b, h, w, cout), FILL16, dtype=torch.int16, device=d)
    p_lo = torch.full((b, h, w, cout), FILL16, dtype=torch.int16, device=d) if split else None
    d_scale, d_shift = dev(scale), dev(shift)
    head = (F.ptr(xp.hi), F.ptr(xp.lo), b, h, w, cin, F.ptr(w_hi), F.ptr(w_l if w_lo else None), c_out or cout, kernel, 1, F.ptr(d_scale), F.ptr(d_shift))
    tail = (int(relu), F.ptr(p_hi), F.ptr(p_lo), F.ptr(f32), c_out or cout, 0, F.stream_ptr(d))
    if use_res:
        rc = L.lvq_conv2d_res(*head, F.ptr(res.hi if res_hi else None), F.ptr(res.lo if res_lo else None), *tail)
    else:
        rc = L.lvq_conv2d(*head, *tail)
    torch.cuda.synchronize()
    return rc, f32, p_hi, p_lo


def res_planes(b, c, h, w, mode, seed, zero=False):
    """Residual operand planes [B, H, W, C] and the fp64 value they hold ([B, C, H, W]): hi + lo, or hi alone in the plain form."""
    r = np.zeros((b, c, h, w), np.float32) if zero else synth.randn((b, c, h, w), seed)
    p = B2.to_planes(dev(r), mode == "bf16x3")
    val = bits_to_f32(p.hi).double() + (bits_to_f32(p.lo).double() if p.lo is not None else 0.0)
    return p, val.permute(0, 3, 1, 2).cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h,w", [(4, 3), (8, 6), (9, 7)])
@pytest.mark.parametrize("c", [64, 256])
def test_conv2d_res_against_fp64(c, h, w, mode):
    """y = relu(acc * scale + shift + res) against fp64 of the same rounded planes, residual included; both output forms; with a zero
    residual the result is lvq_conv2d's bit for bit."""
    seed = 9000 + c + 16 * h + w
    x, wt, scale, shift = BC.layer_operands("conv", 2, c, c, 3, h, w, mode, seed)
    res, res_val = res_planes(2, c, h, w, mode, seed + 7)
    for relu in (True, False):
        ref = BC.conv_ref(x, wt, 3, 1, scale, shift, False) + res_val
        ref = np.maximum(ref, 0.0) if relu else ref
        rc, f32, p_hi, p_lo = run_res(x, wt, mode, scale, shift, res, relu)
        assert rc == 0, F.lib().lvq_strerror(rc)
        err = float(np.abs(f32.cpu().numpy() - ref).max())
        bound = BOUND[mode] * max(1.0, float(np.abs(ref).max()))
        print(f"conv2d_res {c}->{c} [2, {h}, {w}] {mode} relu={relu}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (c, h, w, mode, relu, err, bound)
        hi = f32.to(torch.bfloat16)
        assert torch.equal(p_hi.permute(0, 3, 1, 2), hi.view(torch.int16)), "hi plane is not the bf16 of the fp32 result"
        if p_lo is not None:
            assert torch.equal(p_lo.permute(0, 3, 1, 2), (f32 - hi.float()).to(torch.bfloat16).view(torch.int16))
    zero, _ = res_planes(2, c, h, w, mode, 0, zero=True)
    a = run_res(x, wt, mode, scale, shift, zero, True)
    b = run_res(x, wt, mode, scale, shift, None, True, use_res=False)
    assert a[0] == 0 and b[0] == 0
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2]) and (a[3] is None or torch.equal(a[3], b[3]))


def test_conv2d_res_error_paths_leave_the_outputs_untouched():
    x, wt, scale, shift = BC.layer_operands("conv", 2, 64, 64, 3, 4, 3, "bf16x3", 9900)
    res, _ = res_planes(2, 64, 4, 3, "bf16x3", 9901)
    calls = [(-1, "bf16x3", dict(res_hi=False)),                                 # NULL res_hi
             (-1, "bf16x3", dict(res_hi=False, res_lo=False)),
             (-1, "bf16", dict(res_lo=True)),                                   # res_lo in the plain form
             (-5, "bf16x3", dict(kernel=5)),                                    # outside the family: kernel, then c_out
             (-5, "bf16x3", dict(c_out=48))]
    for want, mode, kw in calls:
        xs, ws = (x, wt) if mode == "bf16x3" else (bf16_round(x), bf16_round(wt))
        r = res if mode == "bf16x3" else type("P", (), dict(hi=res.hi, lo=res.lo))
        rc, f32, p_hi, p_lo = run_res(xs, ws, mode, scale, shift, r, **kw)
        assert rc == want, (rc, want, kw)
        assert bool((f32 == FILL).all()) and bool((p_hi == FILL16).all()) and (p_lo is None or bool((p_lo == FILL16).all())), kw


# --------------------------------------------------------------------------------------------------------------------------------
# 4 - 6. whole backbones
# --------------------------------------------------------------------------------------------------------------------------------
def load(m, sd):
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(DEV).eval()


def rel_err(got, want):
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def sparse_errors(got, ref, stages):
    """{stage: relative error}; the rows are compared through their coordinates: both sides ascend in (b, z, y, x) behind a regular conv
    and keep the input's order behind a submanifold one."""
    errs = {}
    for k in stages:
        f, i, shape = ref[k]
        assert got[k].spatial_shape == list(shape), k
        assert np.array_equal(got[k].indices.cpu().numpy(), i), f"{k}: active set differs"
        errs[k] = rel_err(got[k].features.cpu().numpy(), f)
    return errs


def run_voxel(name, case, mode, last_pad=0):
    idx, feat, batch, grid, sd, ref = C.voxel_case(name, case, last_pad)
    m = load(B3.backbones_3d_all[name](BC.Cfg({"last_pad": last_pad} if last_pad else {}), 4, list(grid)), sd)
    m.precision = mode
    bd = dict(voxel_features=dev(feat), voxel_coords=dev(idx, np.int32), batch_size=batch)
    with torch.no_grad():
        bd = m(bd)
    got = dict(bd["multi_scale_3d_features"], out=bd["encoded_spconv_tensor"])
    return bd, sparse_errors(got, ref, ("x_conv1", "x_conv2", "x_conv3", "x_conv4", "out")), ref, batch


def run_pillar(name, case, mode):
    idx, feat, batch, grid, sd, ref = C.pillar_case(name, case)
    m = load(B3.backbones_3d_all[name](BC.Cfg({}), 32, list(grid)), sd)
    m.precision = mode
    bd = dict(pillar_features=dev(feat), pillar_coords=dev(idx, np.int32), batch_size=batch)
    with torch.no_grad():
        bd = m(bd)
    got = bd["multi_scale_2d_features"]
    errs = sparse_errors(got, ref, ("x_conv1", "x_conv2", "x_conv3"))
    for k, r in (("x_conv4", ref["x_conv4_dense"]), ("x_conv5", ref["x_conv5"])):
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == r.shape, k
        errs[k] = rel_err(got[k].cpu().numpy(), r)
    assert bd["multi_scale_2d_strides"] == {"x_conv1": 1, "x_conv2": 2, "x_conv3": 4, "x_conv4": 8, "x_conv5": 16}
    return bd, errs, ref, batch


@pytest.mark.parametrize("case,last_pad", [("v_a", 0), ("v_b", 0), ("v_b", 1)])
@pytest.mark.parametrize("name", list(C.VOXEL))
def test_voxel_backbones_bf16x3_meet_the_parity_bar_at_every_stage(name, case, last_pad):
    bd, errs, ref, batch = run_voxel(name, case, "bf16x3", last_pad)
    print(f"{name} {case} last_pad={last_pad} bf16x3: {errs}")
    assert bd["encoded_spconv_tensor_stride"] == 8 and bd["multi_scale_3d_strides"] == {"x_conv1": 1, "x_conv2": 2, "x_conv3": 4, "x_conv4": 8}
    assert max(errs.values()) <= BAR, errs
    # through HeightCompression: [B, 128 * D, H, W], channel c * D + z
    sf = lidar.map_to_bev_all["HeightCompression"](BC.Cfg(NUM_BEV_FEATURES=256))(bd)["spatial_features"]
    want = C.height_compression(ref["out"], batch)
    assert tuple(sf.shape) == want.shape and rel_err(sf.cpu().numpy(), want) <= BAR


@pytest.mark.parametrize("case", ["p_a", "p_b"])
@pytest.mark.parametrize("name", list(C.PILLAR))
def test_pillar_backbones_bf16x3_meet_the_parity_bar_at_every_stage(name, case):
    bd, errs, ref, batch = run_pillar(name, case, "bf16x3")
    print(f"{name} {case} bf16x3: {errs}")
    assert max(errs.values()) <= BAR, errs


@pytest.mark.parametrize("name,calls", [("VoxelBackBone8x", 8), ("VoxelResBackBone8x", 9), ("PillarBackBone8x", 7), ("PillarRes18BackBone8x", 7)])
def test_tables_are_shared_by_indice_key(name, calls):
    """One lvq_sparse_conv_rules call per indice_key and forward: subm1 (shared by conv_input and conv1 in VoxelBackBone8x) / res1, then
    spconvN + submN / resN for N = 2 .. 4, and spconv_down2 in the 3-D pair."""
    seen, real = [], B3.sparse_conv_rules
    B3.sparse_conv_rules = lambda *a, **k: (seen.append(1), real(*a, **k))[1]
    try:
        run_voxel(name, "v_b", "bf16x3") if name in C.VOXEL else run_pillar(name, "p_b", "bf16x3")
    finally:
        B3.sparse_conv_rules = real
    assert len(seen) == calls


def test_second_chain_end_to_end():
    """voxel features (as MeanVFE leaves them) -> VoxelResBackBone8x -> HeightCompression -> BaseBEVBackbone, against the fp64 chain."""
    bd, errs, ref, batch = run_voxel("VoxelResBackBone8x", "v_a", "bf16x3")
    bd = lidar.map_to_bev_all["HeightCompression"](BC.Cfg(NUM_BEV_FEATURES=256))(bd)
    cfg, cin, _ = C.SECOND_2D
    assert bd["spatial_features"].shape[1] == cin and bd["spatial_features_stride"] == 8
    m2 = load(B2.BaseBEVBackbone(BC.Cfg(cfg), cin), C.second_2d_state())
    with torch.no_grad():
        out = m2(bd)["spatial_features_2d"]
    want = C.second_chain()
    assert tuple(out.shape) == want.shape == (3, 512, 6, 8)
    err = rel_err(out.cpu().numpy(), want)
    print(f"SECOND chain: err {err:.3e} (max|ref| {np.abs(want).max():.3f})")
    assert float(np.abs(want).max()) > 1e-2 and err <= BAR


def test_pillarnet_chain_end_to_end():
    """pillars -> PillarRes18BackBone8x -> BaseBEVBackboneV1, against the fp64 chain."""
    bd, errs, ref, batch = run_pillar("PillarRes18BackBone8x", "p_a", "bf16x3")
    m2 = load(B2.BaseBEVBackboneV1(BC.Cfg(C.PILLARNET_2D[0])), C.pillarnet_2d_state())
    with torch.no_grad():
        out = m2(bd)["spatial_features_2d"]
    want = C.pillarnet_chain()
    assert tuple(out.shape) == want.shape == (2, 256, 8, 6)
    err = rel_err(out.cpu().numpy(), want)
    print(f"PillarNet chain: err {err:.3e} (max|ref| {np.abs(want).max():.3f})")
    assert float(np.abs(want).max()) > 1e-2 and err <= BAR


@pytest.mark.parametrize("name", [*C.VOXEL, *C.PILLAR])
def test_plain_bf16_over_a_whole_backbone_is_recorded(name):
    """No bar is known in advance for plain bf16 operands over twelve to twenty layers: the error is printed (DESIGN 3.6 and the
    module docstring record what the MI355X gave) and only its finiteness is asserted."""
    bd, errs, ref, batch = run_voxel(name, "v_a", "bf16") if name in C.VOXEL else run_pillar(name, "p_a", "bf16")
    print(f"{name} plain bf16: {errs}")
    assert all(np.isfinite(v) for v in errs.values())


# --------------------------------------------------------------------------------------------------------------------------------
# 7. a weight update is seen
# --------------------------------------------------------------------------------------------------------------------------------
def test_weight_update_reaches_the_wide_and_the_residual_conv():
    """After an in-place update of a 256 -> 256 sparse weight and of a dense BasicBlock's conv2 (weight and bias: the bias lives in the
    folded shift), the next forward equals a fresh module's with the new values, bit for bit -- and differs from the one before."""
    name = "PillarRes18BackBone8x"
    idx, feat, batch, grid, sd, _ = C.pillar_case(name, "p_a")
    bd = lambda: dict(pillar_features=dev(feat), pillar_coords=dev(idx, np.int32), batch_size=batch)
    m = load(B3.backbones_3d_all[name](BC.Cfg({}), 32, list(grid)), sd)
    with torch.no_grad():
        before = m(bd())["multi_scale_2d_features"]
        new = dict(sd)
        for key, seed in (("conv4.1.conv1.weight", 61), ("conv5.1.conv2.weight", 62), ("conv5.1.conv2.bias", 63)):
            new[key] = (synth.seeded_array(key, sd[key].shape, seed) * (np.sqrt(2.0) if sd[key].ndim > 1 else 1.0)).astype(np.float32)
            dict(m.named_parameters())[key].copy_(torch.from_numpy(new[key]))
        after = m(bd())["multi_scale_2d_features"]
        fresh = load(B3.backbones_3d_all[name](BC.Cfg({}), 32, list(grid)), new)(bd())["multi_scale_2d_features"]
    for k in ("x_conv4", "x_conv5"):
        assert torch.equal(after[k], fresh[k]), k
        assert not torch.equal(after[k], before[k]), k
    assert torch.equal(after["x_conv3"].features, before["x_conv3"].features)
