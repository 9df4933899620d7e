"""Every public module of vision_tower.py through its own forward -- PatchEmbed, LayerNorm2d, MLPBlock, Attention, Block and
ImageEncoderViT(use_abs_pos=False) -- against the fp64 restatements of tests/vision_tower_cases.py, on small seeded states
(VC.seeded: relative-position tables ~ N(0, 0.25^2)), and the per-module cache of packed weights and resized tables.

Bounds.  bf16x3 (hi + lo operands): the sum of the bounds the suite holds the launched kernels to, times max(1, max|ref|) -- 2e-4 per GEMM,
attention or conv, VC.K_LN per LayerNorm (VC.BLOCK_BOUND spells out a block's seven launches); the weights are unit-gain, so the kernels'
errors add and are not amplified.  LayerNorm2d alone is held elementwise to norm_bound of tests/test_gpu_head_kernels.py with the module's
eps.  Plain bf16 has no bound known in advance: PLAIN_MEASURED holds max|out - ref| / max(1, max|ref|) measured on the MI355X, and the test
asserts twice that value as a regression guard (as tests/test_gpu_vision_tower.py does).  Both errors are printed in every run."""
import functools
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vision_tower_cases as VC  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402
from lidar_vision_vqa_amd import vision_tower as VT  # noqa: E402

DEV = "cuda:0"
D, HEADS = VC.MOD_D, VC.MOD_HEADS
U = 2.0 ** -24
# max |out - ref| / max(1, max|ref|) in the plain bf16 form, measured on the MI355X
PLAIN_MEASURED = {
    "patch_embed_48x80": 2.11e-3, "patch_embed_50x83": 2.37e-3, "mlp": 3.47e-3,                     # (bf16x3: 3.7e-6, 4.3e-6, 5.6e-6)
    "attention_tables_5x7": 8.10e-3, "attention_tables_10x10": 7.68e-3,                             # (1.52e-5, 1.53e-5)
    "block_global_5x7": 5.25e-3, "block_win4_5x7": 4.21e-3, "block_win14_5x7": 3.21e-3, "block_win14_20x20": 3.59e-3,     # (7.4e-6, 7.7e-6, 5.2e-6, 7.1e-6)
    "encoder_no_pos": 8.15e-3,                                                                      # (1.65e-5)
}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def load(m, sd):
    m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV).eval()


def seeded_module(m, seed):
    """m with VC.seeded weights -> (m on the device in eval mode, the state as numpy)."""
    sd = VC.seeded_state([(k, v.shape) for k, v in m.state_dict().items()], seed)
    return load(m, sd), sd


def run(m, x, mode):
    m.precision = mode
    with torch.no_grad():
        return m(x if torch.is_tensor(x) else t(x).to(DEV))


def rel(out, ref):
    return float(np.abs(out - ref).max()) / max(1.0, float(np.abs(ref).max()))


def hold(case, m, x, ref, bound):
    """Both precisions of module m on x against ref: bf16x3 at `bound`, plain bf16 at twice its measured error."""
    x = t(x).to(DEV)
    out3, out1 = run(m, x, "bf16x3"), run(m, x, "bf16")
    assert out3.dtype == torch.float32 and tuple(out3.shape) == ref.shape == tuple(out1.shape)
    e3, e1 = rel(out3.cpu().numpy(), ref), rel(out1.cpu().numpy(), ref)
    print(f"MODULE {case}: bf16x3 {e3:.3e} (bound {bound:.1e}), bf16 {e1:.3e} (measured {PLAIN_MEASURED[case]:.2e}), max|ref| {np.abs(ref).max():.3f}")
    assert e3 <= bound, (case, e3)
    assert e1 <= 2 * PLAIN_MEASURED[case], (case, e1)
    assert e3 < e1
    return out3, out1


# ------------------------------------------------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(48, 80), (50, 83)])
def test_patch_embed(h, w):
    """A 3 x 5 patch grid (not square); 50 x 83 leaves 2 rows and 3 columns that belong to no patch."""
    m, sd = seeded_module(VT.PatchEmbed(embed_dim=D), 61)
    x = VC.synth.randn((2, 3, h, w), 161)
    ref = VC.patch_embed_ref(sd, x)
    assert ref.shape == (2, 3, 5, D)
    hold(f"patch_embed_{h}x{w}", m, x, ref, VC.K_GEMM)


def test_layernorm2d():
    """[2, 256, 5, 7]: N(0, 1); a per-pixel mean of 1e3; and one pixel constant over the channels, whose variance is 0 -- eps alone keeps
    its output finite, and it is the bias.  Elementwise bound: norm_bound of tests/test_gpu_head_kernels.py with this module's eps."""
    c = 256
    m, sd = seeded_module(VT.LayerNorm2d(c), 62)
    assert m.eps == VC.LN_EPS
    base = VC.synth.randn((2, c, 5, 7), 162)
    const = base.copy()
    const[1, :, 2, 3] = 3.0
    for name, x in (("unit", base), ("offset", base + np.float32(1e3)), ("constant pixel", const)):
        xd = torch.from_numpy(x).double()
        ref = VC.ln2d(xd, sd["weight"], sd["bias"])
        k = (c / 64 + 8) * U
        xc = xd - xd.mean(1, keepdim=True)
        rstd = torch.rsqrt((xc * xc).mean(1, keepdim=True) + m.eps)
        gmax = float(np.abs(sd["weight"]).max())
        bound = k * ref.abs().amax(1, keepdim=True) + k * xd.abs().amax(1, keepdim=True) * rstd * gmax + 4 * U * ref.abs() + 1e-30
        outs = [run(m, x, mode) for mode in VT.MODES]
        assert torch.equal(outs[0], outs[1])                                    # fp32 in, fp32 out: no operand is rounded in either mode
        err = (outs[0].cpu().double() - ref).abs()
        print(f"MODULE layernorm2d {name}: err {float(err.max()):.3e}, largest bound {float(bound.max()):.3e}, worst ratio {float((err / bound).max()):.3f}")
        assert bool(torch.isfinite(outs[0]).all()) and bool((err <= bound).all())
        if name == "constant pixel":
            assert torch.equal(outs[0][1, :, 2, 3].cpu(), t(sd["bias"]))


def test_mlp_block():
    m, sd = seeded_module(VT.MLPBlock(D, 4 * D), 63)
    x = VC.synth.randn((37, D), 163)
    hold("mlp", m, x, VC.mlp_ref(sd, x), 2 * VC.K_GEMM)


@pytest.mark.parametrize("size", [(5, 7), (10, 10)])
def test_attention(size):
    """[2, 5, 7, 128], 2 heads: tables made for the grid, and tables of 19 rows resized to 9 and to 13."""
    m, sd = seeded_module(VT.Attention(D, HEADS, use_rel_pos=True, input_size=size), 64)
    assert tuple(m.rel_pos_h.shape) == (2 * size[0] - 1, D // HEADS)
    x = VC.synth.randn((2, 5, 7, D), 164)
    hold(f"attention_tables_{size[0]}x{size[1]}", m, x, VC.attention_module_ref(sd, x, HEADS), 2 * VC.K_GEMM + VC.K_ATTN)


@functools.lru_cache(maxsize=None)
def block_module(name):
    b, gh, gw, ws = VC.BLOCK_CASES[name][:4]
    m = VT.Block(D, HEADS, use_rel_pos=True, window_size=ws, input_size=(gh, gw), norm_layer=partial(torch.nn.LayerNorm, eps=VC.LN_EPS))
    return load(m, VC.block_case(name)[0])


@pytest.mark.parametrize("name", list(VC.BLOCK_CASES))
def test_block(name):
    """Global, padded by different amounts on the two axes, one window larger than the grid, and several padded windows.  That pad keys
    are live is pinned on the CPU (test_vision_tower_restatements.py: masking them moves these references by 100 x this bound)."""
    hold(f"block_{name}", block_module(name), VC.block_case(name)[1], VC.block_ref(name), VC.BLOCK_BOUND)


def no_pos_model(sd):
    m = VT.ImageEncoderViT(**VC.NO_POS, qkv_bias=True, use_rel_pos=True, use_abs_pos=False, norm_layer=partial(torch.nn.LayerNorm, eps=VC.LN_EPS))
    assert m.pos_embed is None and "pos_embed" not in m.state_dict()
    return load(m, sd)


def test_encoder_without_pos_embed_on_a_non_square_grid():
    """ImageEncoderViT(use_abs_pos=False): the patch GEMM has no row table, the patch grid is 4 x 8, block 0's windows of 3 pad it to 6 x 9,
    block 1's rel_pos_h is resized from 15 to 7 rows, net_3 emits 1 x 2.  15 GEMM / attention / conv launches and 6 LayerNorms."""
    sd, x, ref = VC.no_pos_case()
    m = no_pos_model(sd)
    assert ref.shape == (3, 1024, 1, 2)
    bound = (2 * 5 + 2) * VC.K_GEMM + 3 * VC.K_CONV + 6 * VC.K_LN           # patch, 2 x (qkv, attention, proj, lin1, lin2), neck GEMM; 3 convs
    hold("encoder_no_pos", m, x, ref, bound)
    xd = t(x).to(DEV)
    for mode in VT.MODES:                                                       # a batch of 3 equals three batches of 1 bit for bit
        whole = run(m, xd, mode)
        for i in range(3):
            assert torch.equal(whole[i:i + 1], run(m, xd[i:i + 1].contiguous(), mode)), (mode, i)
    with pytest.raises(F.LvqError, match="square"), torch.no_grad():            # with pos_embed the same image is refused
        VT.ImageEncoderViT(**VC.NO_POS, use_rel_pos=True).to(DEV).eval()(xd)


def test_every_module_refuses_cpu_tensors_train_mode_and_gradients():
    mods = [(VT.PatchEmbed(embed_dim=D), (1, 3, 32, 32)), (VT.LayerNorm2d(64), (1, 64, 2, 2)), (VT.MLPBlock(D, 4 * D), (3, D)),
            (VT.Attention(D, HEADS, use_rel_pos=True, input_size=(2, 2)), (1, 2, 2, D)),
            (VT.Block(D, HEADS, use_rel_pos=True, input_size=(2, 2)), (1, 2, 2, D))]
    for m, shape in mods:
        m = m.to(DEV).eval()
        x = torch.randn(shape, device=DEV)
        with torch.no_grad():
            good = m(x)                                                         # the call that is refused below is a valid one
        assert tuple(good.shape)[0] == shape[0] and bool(torch.isfinite(good).all())
        with pytest.raises(F.LvqError), torch.no_grad():
            m(x.cpu())                                                          # CPU input: no fallback
        m.train()
        with pytest.raises(F.LvqError), torch.no_grad():
            m(x)                                                                # train() mode
        m.eval()
        with pytest.raises(F.LvqError):
            m(x)                                                                # gradients in reach (the parameters require them)
        for p in m.parameters():
            p.requires_grad_(False)
        with pytest.raises(F.LvqError):
            m(x.clone().requires_grad_(True))                                   # ... or the input does
        assert torch.equal(m(x), good)                                          # nothing in reach: the call runs outside no_grad too


# ------------------------------------------------------------------------------------------------------------------------------------
# the cache of packed weights, resized tables and conv packs (vision_tower._cached): keyed by parameter version
# ------------------------------------------------------------------------------------------------------------------------------------
CACHED_KINDS = ("patch_embed.proj.weight", "pos_embed", "blocks.0.attn.rel_pos_h", "blocks.1.attn.rel_pos_w", "blocks.0.attn.qkv.weight",
                "neck.2.weight", "net_3.weight")


def pad_model(sd):
    m = VT.ImageEncoderViT(**VC.CASES["pad"][0], qkv_bias=True, use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=VC.LN_EPS))
    return load(m, sd)


def test_weight_cache_follows_in_place_changes_and_load_state_dict():
    """The `pad` geometry on its own input (10 x 10 grid: pos_embed and tables as stored) and on the `resized` input (8 x 8: pos_embed
    resized, the global block's tables resized from 19 to 15 rows).  After a forward has filled the caches, one parameter of every cached
    kind is scaled in place; the next forward must equal a fresh model built from the modified state_dict, bit for bit, in both
    precisions -- and differ from the forward before.  The same after load_state_dict of a second seeded state.  Switching the
    precision back and forth returns each mode's earlier bits."""
    cfg = VC.CASES["pad"][0]
    assert cfg["global_attn_indexes"] == (1,) and cfg["window_size"] > 0
    inputs = {n: t(VC.case_input(n)).to(DEV) for n in ("pad", "resized")}
    m = pad_model(VC.case_state("pad"))
    names = dict(m.named_parameters())
    forward = lambda model: {(n, mode): run(model, x, mode) for mode in VT.MODES for n, x in inputs.items()}
    first = forward(m)
    again = forward(m)
    assert all(torch.equal(first[k], again[k]) for k in first)                  # (modes were switched back and forth in between)
    with torch.no_grad():
        for k in CACHED_KINDS:
            names[k].mul_(1.25)
    second = forward(m)
    fresh = forward(pad_model({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}))
    for k in first:
        assert torch.equal(second[k], fresh[k]), f"{k}: a stale cached operand"
        assert not torch.equal(second[k], first[k]), k
    for kind in CACHED_KINDS:                                                   # each kind on its own: the output follows it, and comes back
        with torch.no_grad():
            saved = names[kind].clone()
            names[kind].mul_(0.5)
            moved = run(m, inputs["resized"], "bf16x3")
            names[kind].copy_(saved)
        assert not torch.equal(moved, second[("resized", "bf16x3")]), f"{kind}: a change in place did not reach the output"
    assert all(torch.equal(v, second[k]) for k, v in forward(m).items())
    other = VC.state(cfg, 77)
    m.load_state_dict({k: t(v) for k, v in other.items()}, strict=True)
    third, fresh3 = forward(m), forward(pad_model(other))
    for k in first:
        assert torch.equal(third[k], fresh3[k]), f"{k}: a stale cached operand after load_state_dict"
        assert not torch.equal(third[k], second[k]), k
