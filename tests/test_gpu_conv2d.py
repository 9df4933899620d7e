"""lvq_conv2d / lvq_deconv2d / lvq_conv2d_to_planes (csrc/conv2d.hip: implicit GEMM on bf16 MFMA tiles over an LDS tile with its halo, fused
epilogue, strided-channel outputs) through the C ABI against the fp64 restatement of tests/bev_backbone_cases.py.

Regime and bounds are those of tests/test_gpu_sparse_conv.py (whose sums, 27 x 128 deep, are deeper than the 9 x 256 here): N(0, 1)
features, weights scaled by 1 / sqrt(taps C_in);  hi + lo operands 2e-4 max(1, max|ref|);  plain bf16 with operands rounded to bf16 on the
host first (the reference sees the rounded values, so what is left is the fp32 accumulation) 2e-5 max(1, max|ref|).

Every run (but those that ask for one form, as the image encoder does) writes BOTH output forms into a concat buffer 64 channels wider than the layer (channel offset 32) with a pre-filled tail: the
fp32 [B, C, H, W] result is held to the bound, the operand planes must be the bf16 hi / lo split of exactly those fp32 values, and
everything outside the layer's channel and pixel range must keep the fill bit for bit.  The tile is 8 x 8 output pixels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bev_backbone_cases as BC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import backbone2d as B2  # noqa: E402
from lidar_vision_vqa_amd import backbone3d as B3  # noqa: E402
from lidar_vision_vqa_amd import synth  # noqa: E402

DEV = "cuda:0"
FILL = -7.25
FILL16 = 0x7B7B
TAIL = 4096
BOUND = {"bf16x3": 2e-4, "bf16": 2e-5}
GEOMS = ((3, 1), (3, 2), (1, 1), (2, 2), (4, 4))                               # (kernel, stride)
SIZES = ((1, 1), (2, 3), (7, 9), (8, 8), (9, 17), (16, 24), (17, 33), (9, 7), (15, 16))
PAIRS = ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (40, 64))   # the three configs' pairs and a padded C_in


def dev(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def bf16_bits(t):
    """fp32 tensor -> int16 storage of its round-to-nearest-even bf16."""
    return t.to(torch.bfloat16).view(torch.int16)


def bits_to_f32(t):
    return t.view(torch.bfloat16).float()


def out_hw(kind, k, s, h, w):
    if kind == "deconv":
        return h * s, w * s
    return ((h - 1) // s + 1, (w - 1) // s + 1) if k == 3 else (h // s, w // s)


def run_layer(kind, x, wt, k, s, mode, scale=None, shift=None, relu=False, pad_c=64, c_off=32, outputs="both"):
    """-> fp32 [B, C_out, OH, OW] of the layer's own channel range, after the stray-write and plane checks (see run_forms)."""
    return run_forms(kind, x, wt, k, s, mode, scale, shift, relu, pad_c, c_off, outputs)["f32"].cpu().numpy()


def run_forms(kind, x, wt, k, s, mode, scale=None, shift=None, relu=False, pad_c=64, c_off=32, outputs="both"):
    """One call that asks for `outputs`: "both" forms, the operand "planes" only (out_f32 == NULL) or "f32" only (out_hi == out_lo == NULL).
    The buffers of a form that is not requested exist all the same and must keep their fill.  -> {"f32": [B, C_out, OH, OW] | None,
    "hi", "lo": int16 [B, OH, OW, C_out] | None}: device tensors of the layer's own channel range, after the stray-write checks."""
    assert outputs in ("both", "planes", "f32")
    L = B2._lib()
    d = torch.device(DEV)
    split = mode == "bf16x3"
    b, cin, h, w = x.shape
    cout = wt.shape[1] if kind == "deconv" else wt.shape[0]
    xp = B2.to_planes(dev(x), split)
    ne = int(L.lvq_conv2d_packed_elems(F.cint(cout), F.cint(cin), F.cint(k), F.cint(int(kind == "deconv"))))
    assert ne == B2.pad32(cin) * k * k * cout
    d_w = dev(wt)
    w_hi = torch.empty((ne,), dtype=torch.int16, device=d)
    w_lo = torch.empty((ne,), dtype=torch.int16, device=d) if split else None
    assert L.lvq_conv2d_pack_weights(F.ptr(d_w), F.cint(cout), F.cint(cin), F.cint(k), F.cint(int(kind == "deconv")), F.ptr(w_hi), F.ptr(w_lo),
                                     F.stream_ptr(d)) == 0
    oh, ow = out_hw(kind, k, s, h, w)
    ct = cout + pad_c
    n = b * ct * oh * ow
    f32 = torch.full((n + TAIL,), FILL, dtype=torch.float32, device=d)
    p_hi = torch.full((n + TAIL,), FILL16, dtype=torch.int16, device=d)
    p_lo = torch.full((n + TAIL,), FILL16, dtype=torch.int16, device=d) if split else None
    d_scale, d_shift = dev(scale), dev(shift)
    head = (F.ptr(xp.hi), F.ptr(xp.lo), F.cint(b), F.cint(h), F.cint(w), F.cint(cin), F.ptr(w_hi), F.ptr(w_lo), F.cint(cout))
    want_planes, want_f32 = outputs != "f32", outputs != "planes"
    tail = (F.ptr(d_scale), F.ptr(d_shift), F.cint(int(relu)), F.ptr(p_hi if want_planes else None), F.ptr(p_lo if want_planes else None),
            F.ptr(f32 if want_f32 else None), F.cint(ct), F.cint(c_off), F.stream_ptr(d))
    if kind == "deconv":
        rc = L.lvq_deconv2d(*head, F.cint(s), *tail)
    else:
        rc = L.lvq_conv2d(*head, F.cint(k), F.cint(s), *tail)
    assert rc == 0, F.lib().lvq_strerror(rc)
    torch.cuda.synchronize()
    # fp32 [B, ct, OH, OW]: only channels c_off .. c_off + cout - 1 are written
    assert bool((f32[n:] == FILL).all()), "fp32 tail written"
    o = f32[:n].view(b, ct, oh, ow)
    assert bool((o[:, :c_off] == FILL).all()) and bool((o[:, c_off + cout:] == FILL).all()), "fp32 channels outside the range written"
    mine = o[:, c_off:c_off + cout]
    if not want_f32:
        assert bool((mine == FILL).all()), "fp32 written by a call that did not ask for it"
    forms = {"f32": mine if want_f32 else None, "hi": None, "lo": None}
    # planes [B, OH, OW, ct]: the hi / lo split of exactly the fp32 values, nothing else touched
    for name, plane in (("hi", p_hi), ("lo", p_lo)):
        if plane is None:
            continue
        assert bool((plane[n:] == FILL16).all()), "plane tail written"
        pv = plane[:n].view(b, oh, ow, ct)
        assert bool((pv[..., :c_off] == FILL16).all()) and bool((pv[..., c_off + cout:] == FILL16).all()), "plane channels outside the range written"
        own = pv[..., c_off:c_off + cout]
        if not want_planes:
            assert bool((own == FILL16).all()), "planes written by a call that did not ask for them"
            continue
        forms[name] = own
        if want_f32:
            want = bf16_bits(mine) if name == "hi" else bf16_bits(mine - bits_to_f32(bf16_bits(mine)))
            assert torch.equal(own.permute(0, 3, 1, 2), want), "planes are not the bf16 split of the fp32 result"
    return forms


def reference(kind, x, wt, k, s, scale, shift, relu):
    return BC.deconv_ref(x, wt, s, scale, shift, relu) if kind == "deconv" else BC.conv_ref(x, wt, k, s, scale, shift, relu)


def compare(kind, batch, cin, cout, k, s, h, w, mode, seed, relu=True):
    x, wt, scale, shift = BC.layer_operands(kind, batch, cin, cout, k, h, w, mode, seed)
    ref = reference(kind, x, wt, k, s, scale, shift, relu)
    out = run_layer(kind, x, wt, k, s, mode, scale, shift, relu)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err = float(np.abs(out - ref).max())
    bound = BOUND[mode] * max(1.0, float(np.abs(ref).max()))
    print(f"{kind} {cin}->{cout} k{k} s{s} [{batch}, {h}, {w}] {mode}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (kind, cin, cout, k, s, h, w, mode, err, bound)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_conv_every_channel_pair_and_geometry(cin, cout, mode):
    """Every (C_in, C_out) of the three configs and a padded C_in, both operand forms, all five (kernel, stride) pairs, batch 2 with
    different content per scene; two spatial sizes per geometry, rotating with the case so that every size meets every geometry."""
    base = PAIRS.index((cin, cout))
    for g, (k, s) in enumerate(GEOMS):
        for j in range(2):
            h, w = SIZES[(2 * base + 3 * g + j) % len(SIZES)]
            if min(h, w) < s and k != 3:
                h, w = h + s, w + s                                             # kernel = stride needs one whole window
            compare("conv", 2, cin, cout, k, s, h, w, mode, 100 * base + 10 * g + j)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("k,s", GEOMS)
def test_conv_every_size_around_the_tile(k, s, mode):
    """One below, at and one above the 8-pixel tile in each axis, the degenerate canvases, and stride 2 on odd and even H / W (input 15, 16,
    17 -> output 8, 8, 9); the epilogue without BatchNorm and without ReLU on the odd cases."""
    for i, (h, w) in enumerate(SIZES):
        if k != 3 and min(h, w) < s:
            continue
        x, wt, scale, shift = BC.layer_operands("conv", 2, 64, 64, k, h, w, mode, 500 + i)
        plain = i % 3 == 1
        ref = BC.conv_ref(x, wt, k, s, None if plain else scale, None if plain else shift, not plain)
        out = run_layer("conv", x, wt, k, s, mode, None if plain else scale, None if plain else shift, not plain)
        err, bound = float(np.abs(out - ref).max()), BOUND[mode] * max(1.0, float(np.abs(ref).max()))
        print(f"conv k{k} s{s} [{h}, {w}] {mode}: err {err:.3e} bound {bound:.3e}")
        assert out.shape == ref.shape and err <= bound, (k, s, h, w, err, bound)


# the image encoder's calls (vision_tower._conv): ONE output form, no scale / shift, no ReLU, c_in = 256 and 512 (the widest the kernel
# takes), c_out = 512, and net_3's second half written at channel offset 512 of 1024
TOWER_CALLS = ((256, 512, 64, 32), (512, 512, 64, 32), (512, 512, 512, 512))     # (c_in, c_out, pad_c, c_off)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("cin,cout,pad_c,c_off", TOWER_CALLS)
def test_conv_as_the_image_encoder_calls_it(cin, cout, pad_c, c_off, s, mode):
    """Held to fp64 with both forms requested; then planes only and fp32 only, each bit-equal to the same form of the call for both."""
    for i, (h, w) in enumerate(((9, 17), (16, 16))):
        x, wt, _, _ = BC.layer_operands("conv", 2, cin, cout, 3, h, w, mode, 1300 + 10 * TOWER_CALLS.index((cin, cout, pad_c, c_off)) + i)
        ref = BC.conv_ref(x, wt, 3, s)
        both = run_forms("conv", x, wt, 3, s, mode, pad_c=pad_c, c_off=c_off)
        out = both["f32"].cpu().numpy()
        err, bound = float(np.abs(out - ref).max()), BOUND[mode] * max(1.0, float(np.abs(ref).max()))
        print(f"conv {cin}->{cout} at {c_off} of {cout + pad_c} k3 s{s} [2, {h}, {w}] {mode}: err {err:.3e} bound {bound:.3e}")
        assert out.shape == ref.shape and err <= bound, (cin, cout, s, h, w, mode, err, bound)
        planes = run_forms("conv", x, wt, 3, s, mode, pad_c=pad_c, c_off=c_off, outputs="planes")
        f32 = run_forms("conv", x, wt, 3, s, mode, pad_c=pad_c, c_off=c_off, outputs="f32")
        assert planes["f32"] is None and f32["hi"] is None and f32["lo"] is None
        assert torch.equal(f32["f32"].view(torch.int32), both["f32"].view(torch.int32))
        assert torch.equal(planes["hi"], both["hi"]) and (both["lo"] is None) == (mode == "bf16")
        assert both["lo"] is None or torch.equal(planes["lo"], both["lo"])


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("s", [1, 2, 4])
def test_deconv(s, mode):
    for i, (cin, cout) in enumerate(((64, 128), (128, 128), (256, 128), (256, 256))):
        for j, (h, w) in enumerate(((1, 1), (3, 5), (8, 8), (9, 17))):
            compare("deconv", 2, cin, cout, s, s, h, w, mode, 700 + 10 * i + j, relu=(i + j) % 2 == 0)


def test_to_planes_is_the_bf16_split_with_zero_padding():
    for (b, c, h, w) in ((2, 64, 7, 9), (1, 5, 3, 3), (2, 40, 8, 8), (1, 384, 1, 1), (1, 70, 9, 17)):
        x = dev(synth.randn((b, c, h, w), 900 + c))
        p = B2.to_planes(x, True)
        cp = B2.pad32(c)
        assert tuple(p.hi.shape) == (b, h, w, cp)
        xc = x.permute(0, 2, 3, 1)
        assert torch.equal(p.hi[..., :c], bf16_bits(xc)) and torch.equal(p.lo[..., :c], bf16_bits(xc - bits_to_f32(bf16_bits(xc))))
        assert bool((p.hi[..., c:] == 0).all()) and bool((p.lo[..., c:] == 0).all())
        assert torch.equal(B2.to_planes(x, False).hi, p.hi)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_locality_bits_depend_on_the_receptive_field_only(mode):
    """The same 5 x 5 patch at two positions of a zero canvas, in batch slot 0 or 1: the pixels whose 3 x 3 field lies inside the patch get
    identical bits.  A canvas embedded in a larger zero canvas gives, cropped, the bits of the canvas alone (its border sees zeros either
    way)."""
    cin, cout = 128, 128
    _, wt, scale, shift = BC.layer_operands("conv", 1, cin, cout, 3, 1, 1, mode, 1100)
    patch = synth.randn((cin, 5, 5), 1101)
    outs = []
    for slot, (y0, x0) in ((0, (1, 2)), (1, (6, 7)), (1, (10, 19))):
        x = np.zeros((2, cin, 17, 26), np.float32)
        x[slot, :, y0:y0 + 5, x0:x0 + 5] = patch
        out = run_layer("conv", x, wt, 3, 1, mode, scale, shift, True)
        outs.append(out[slot, :, y0 + 1:y0 + 4, x0 + 1:x0 + 4].copy())
    assert float(np.abs(outs[0]).max()) > 0.5
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32))
    for s in (1, 2):
        small = synth.randn((1, cin, 9, 11), 1102)
        alone = run_layer("conv", small, wt, 3, s, mode, scale, shift, True)
        big = np.zeros((2, cin, 24, 32), np.float32)
        big[1, :, 8:17, 16:27] = small[0]                                       # an even offset: stride 2 samples the same input pixels
        emb = run_layer("conv", big, wt, 3, s, mode, scale, shift, True)
        oh, ow = alone.shape[2:]
        crop = emb[1, :, 8 // s:8 // s + oh, 16 // s:16 // s + ow]
        assert np.array_equal(crop.view(np.uint32), alone[0].view(np.uint32)), s


def test_convention_agrees_with_the_sparse_backbone_s_submconv2d():
    """backbone3d.SubMConv2d on an all-active grid and the dense kernel, same weights after [C_out, C_in, ky, kx] -> [C_out, ky, kx, C_in]:
    they agree within the sum of the two kernels' bounds."""
    b, c, h, w = 2, 128, 9, 13
    x, wt, _, _ = BC.layer_operands("conv", b, c, c, 3, h, w, "bf16x3", 1200)
    ref = BC.conv_ref(x, wt, 3, 1)
    dense = run_layer("conv", x, wt, 3, 1, "bf16x3")
    m = B3.SubMConv2d(c, c, 3, bias=False).to(DEV).eval()
    with torch.no_grad():
        m.weight.copy_(dev(wt.transpose(0, 2, 3, 1)))
        bb, yy, xx = np.meshgrid(np.arange(b), np.arange(h), np.arange(w), indexing="ij")
        idx = np.stack([bb.ravel(), yy.ravel(), xx.ravel()], axis=1).astype(np.int32)
        feats = x.transpose(0, 2, 3, 1).reshape(-1, c)
        out = m(B3.SparseConvTensor(dev(feats), dev(idx, np.int32), [h, w], b)).features
    sparse = out.cpu().numpy().reshape(b, h, w, c).transpose(0, 3, 1, 2)
    bound = 2 * BOUND["bf16x3"] * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(sparse - dense).max())
    print(f"SubMConv2d vs dense: {err:.3e} (bound {bound:.3e}); dense vs fp64 {np.abs(dense - ref).max():.3e}")
    assert err <= bound
